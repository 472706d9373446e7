"""The model of rotated block-wise quantisation (wire v6) — a helper, not a test.

The contract in numpy, float32 throughout. A unit of exactly 4096 elements, its first at flat position c0, becomes
    s[e] = a[e] with its sign bit inverted where bit 23 of tests/sr_model.sr_u24(rot_seed, c0 + e) is set
    for h = 1, 2, 4, ..., 2048 in this order: (t[i], t[i + h]) <- (t[i] + t[i + h], t[i] - t[i + h]) where i & h == 0
    y[e] = t[e] * 2^-6
and y is quantised as tests/blockwise_model (round to nearest) or tests/sr_model.encode_block (stochastic, the draw of
position c0 + e under the separate seed) quantise a unit's values; a shorter unit is theirs unchanged. The decode
dequantises, applies the same transform and the same signs to a full unit, and adds the base. RotOracleBackend puts the
model behind the plan interface (encode_block_rot / decode_block_rot), so the host code runs on the CPU.
"""
import numpy as np
import torch

from tests import blockwise_model as BM
from tests import sr_model as SM
from tests.dense_aggregate_model import DenseAggOracleBackend, DenseAggOraclePlan

UNIT = 4096
F32 = np.float32
NORM = F32(0.015625)


def signs(t, rot_seed, c0):
    """The sign diagonal over full units: t float32[..., 4096], the first element of unit j at flat position c0[j]."""
    t = np.ascontiguousarray(t, dtype=F32).reshape(-1, UNIT)
    c = np.asarray(c0, dtype=np.uint64).reshape(-1, 1) + np.arange(UNIT, dtype=np.uint64)  # (wraps mod 2^64, as uint64_t)
    flip = (SM.sr_u24(rot_seed, c) & np.uint32(0x800000)) << np.uint32(8)
    return (t.view(np.uint32) ^ flip).view(F32)


def hadamard(t):
    """The twelve stages and the 2^-6 over full units: float32[..., 4096] -> float32[N, 4096]."""
    t = np.array(t, dtype=F32).reshape(-1, UNIT)
    with np.errstate(all="ignore"):
        h = 1
        while h < UNIT:
            v = t.reshape(-1, UNIT // (2 * h), 2, h)
            a, b = v[:, :, 0, :], v[:, :, 1, :]
            t = np.stack([a + b, a - b], axis=2).astype(F32).reshape(-1, UNIT)
            h *= 2
        return t * NORM


def unit_rows(segs):
    """(in_off + 4096 u_s, len) of every unit, in unit order."""
    return BM.split_table(segs)[:, :2]


def _full(segs):
    rows = unit_rows(segs)
    return rows[rows[:, 1] == UNIT, 0]


def forward(flat, segs, rot_seed, base=None):
    """flat (- base, fp32) with every full unit replaced by its coefficients: what the unrotated models then quantise."""
    y = np.array(flat, dtype=F32)
    if base is not None:
        with np.errstate(all="ignore"):
            for off, n, _, _ in np.asarray(segs, dtype=np.int64).reshape(-1, 4).tolist():
                y[off:off + n] = y[off:off + n] - np.asarray(base, dtype=F32)[off:off + n]
    offs = _full(segs)
    if offs.size:
        at = offs[:, None] + np.arange(UNIT)
        y[at] = hadamard(signs(y[at], rot_seed, offs))
    return y


def encode(flat, segs, bits, rot_seed, seed=None, base=None):
    """-> (bmn fp32[U], bscale fp32[U], codes uint8, stream uint32[P]); seed: None rounds to nearest."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    y = forward(flat, segs, rot_seed, base)
    return BM.encode(y, segs, bits) if seed is None else SM.encode_block(y, segs, bits, seed)


def decode(stream, mn, scale, segs, bits, span, rot_seed, base=None):
    """-> fp32[span]: positions outside the segments hold the base's values (0 without one)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    y = BM.decode(stream, mn, scale, segs, bits, span)
    offs = _full(segs)
    if offs.size:
        at = offs[:, None] + np.arange(UNIT)
        y[at] = signs(hadamard(y[at]), rot_seed, offs)
    if base is None:
        return y
    out = np.array(base, dtype=F32)
    with np.errstate(all="ignore"):
        for off, n, _, _ in segs.tolist():
            out[off:off + n] = out[off:off + n] + y[off:off + n]
    return out


def rms_error(x, bits, rot_seed=None, seed=None):
    """RMS of x - decode(encode(x)) for one dense segment holding x; rot_seed None: unrotated, 4096-element blocks."""
    x = np.asarray(x, dtype=F32)
    return float(np.sqrt(np.mean((roundtrip(x, bits, rot_seed, seed).astype(np.float64) - x) ** 2)))


def roundtrip(x, bits, rot_seed=None, seed=None):
    x = np.asarray(x, dtype=F32)
    segs = np.array([[0, x.size, x.size, 0]], dtype=np.int64)
    if rot_seed is None:
        mn, sc, _, stream = BM.encode(x, segs, bits) if seed is None else SM.encode_block(x, segs, bits, seed)
        return BM.decode(stream, mn, sc, segs, bits, x.size)
    mn, sc, _, stream = encode(x, segs, bits, rot_seed, seed)
    return decode(stream, mn, sc, segs, bits, x.size, rot_seed)


def same_bits(got, want):
    """Bit-identical float32 arrays, a NaN equal to any NaN (the contract leaves a NaN's sign and payload open)."""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    nan = np.isnan(want)
    return (got.shape == want.shape and np.array_equal(np.isnan(got), nan)
            and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


class RotOraclePlan(SM.SROraclePlan, DenseAggOraclePlan):
    has_block_rot = True

    def encode_block_rot(self, flat=None, tensors=None, base=None, rot_seed=0, seed=None, **_):
        x, segs, b = self._input(flat, tensors, base)
        mn, sc, _, stream = encode(x, segs, self.bits, rot_seed, seed, base=b)
        return torch.from_numpy(mn), torch.from_numpy(sc), torch.from_numpy(stream)

    def decode_block_rot(self, packed, bmn, bscale, rot_seed, base=None, out=None, **_):
        b = None if base is None else base.detach().cpu().numpy()
        res = decode(packed.numpy(), bmn.numpy(), bscale.numpy(), self.table.segs.astype(np.int64), self.bits,
                     self.table.span, rot_seed, base=b)
        if out is not None:
            out[:res.size].copy_(torch.from_numpy(res))
            return out
        return torch.from_numpy(res)


class RotOracleBackend(DenseAggOracleBackend):
    name = "rot-oracle"

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        return RotOraclePlan(sizes, ratio, bits, clients)
