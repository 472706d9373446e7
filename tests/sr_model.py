"""The model of stochastic (unbiased) rounding for the dense quantisers — a helper, not a test.

The contract in numpy, element by element: the ranges are the oracle's (oracle.codec_oracle.quantize over a segment, or
over each 4096-element block of tests/blockwise_model.split_table); the element at flat position c = in_off + e draws
24 uniform bits from three rounds of the lowbias32 mixer over the call's 64-bit seed and c, and its code is floor(t) or
floor(t) + 1 with t the IEEE fp32 quotient (v - mn) / scale. SROracleBackend puts the model behind the plan interface
(encode_sr / encode_block_sr), so the host code runs on the CPU.
"""
import numpy as np
import torch

from coala_amd.compression import wire
from coala_amd.compression.plan import Encoded
from oracle import codec_oracle as O
from tests.blockwise_model import BlockOracleBackend, BlockOraclePlan, split_table

F32 = np.float32
U32 = np.uint32
M32 = 0xFFFFFFFF


def lb(x):
    """lowbias32 on uint32 arrays (wrapping)."""
    x = np.asarray(x, dtype=np.uint64) & M32  # (in 64 bits: a 32 x 32-bit product fits, the mask wraps it)
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def sr_u24(seed, c):
    """The 24 uniform bits of position(s) c under `seed`: uint32, in [0, 2^24)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = np.asarray(c, dtype=np.uint64)
    ks = lb(lb((c >> 32) ^ (seed >> 32) ^ 0x9E3779B9) ^ (seed & M32))
    return (lb((c & M32) ^ ks) >> 8).astype(U32)


def quotient(v, mn, scale):
    """t of the contract: the IEEE fp32 quotient (float32 arrays: numpy's subtract and divide)."""
    with np.errstate(all="ignore"):
        return ((np.asarray(v, dtype=F32) - F32(mn)) / F32(scale)).astype(F32)


def codes_of(t, u24, levels):
    """sr_code of the contract over arrays: t fp32, u24 uint32, levels = 2^bits - 1."""
    t, L = np.asarray(t, dtype=F32), F32(levels)
    with np.errstate(all="ignore"):
        f = np.floor(t)
        u = np.asarray(u24).astype(F32) * F32(2.0 ** -24)  # exact
        up = u < (t - f)  # (t - f is exact)
        code = np.where(t >= L, L, f + up.astype(F32))
        code = np.where(t > 0, code, F32(0))  # NaN, v == mn
    return code.astype(np.uint8)


def sr_codes(v, mn, scale, bits, seed, c0):
    """The codes of one range's values v, the first at flat position c0."""
    v = np.ascontiguousarray(v, dtype=F32)
    if not (scale > 0):
        return np.zeros(v.size, dtype=np.uint8)
    c = np.uint64(c0) + np.arange(v.size, dtype=np.uint64)
    return codes_of(quotient(v, mn, scale), sr_u24(seed, c), (1 << bits) - 1)


def _encode(flat, rows, bits, seed, base):
    total = int((rows[:, 3] + rows[:, 2]).max()) if len(rows) else 0
    vals = np.zeros(total, dtype=np.uint8)
    mn, sc = np.zeros(len(rows), dtype=F32), np.zeros(len(rows), dtype=F32)
    for s, (off, n, k, oo) in enumerate(rows.tolist()):
        assert k == n, "stochastic rounding is defined for dense plans"
        if n == 0:
            continue
        x = flat[off:off + n] if flat is not None else None
        if base is not None:
            with np.errstate(all="ignore"):
                x = x - base[off:off + n]
        _, mn[s], sc[s] = O.quantize(x, bits)
        vals[oo:oo + n] = sr_codes(x, mn[s], sc[s], bits, seed, off)
    return vals, mn, sc


def encode(flat, segs, bits, seed, base=None):
    """Per-tensor ranges -> (codes uint8[max(out_off + n)], mn fp32[T], scale fp32[T])."""
    return _encode(flat, np.asarray(segs, dtype=np.int64).reshape(-1, 4), bits, seed, base)


def encode_block(flat, segs, bits, seed, base=None):
    """Block-wise ranges -> (bmn fp32[U], bscale fp32[U], codes uint8[max(out_off + n)], stream uint32[P])."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    vals, mn, sc = _encode(flat, split_table(segs), bits, seed, base)
    total = int((segs[:, 3] + segs[:, 2]).max()) if len(segs) else 0
    codes = np.zeros(total, dtype=np.uint8)
    codes[:vals.size] = vals
    return mn, sc, codes, wire.pack_dense_codes(codes, segs[:, 1], bits, out_off=segs[:, 3])


class SROraclePlan(BlockOraclePlan):
    def _input(self, flat, tensors, base):
        segs = self.table.segs.astype(np.int64)
        if tensors is not None:
            x = np.zeros(self.table.span, dtype=F32)
            for (off, n, _, _), t in zip(segs.tolist(), tensors):
                x[off:off + n] = t.detach().cpu().numpy().reshape(-1)
        else:
            x = flat.detach().cpu().numpy()
        return x, segs, None if base is None else base.detach().cpu().numpy()

    def encode_sr(self, flat=None, tensors=None, base=None, seed=0, **_):
        x, segs, b = self._input(flat, tensors, base)
        vals, mn, sc = encode(x, segs, self.bits, seed, base=b)
        return Encoded(torch.zeros(0, dtype=torch.int32), torch.from_numpy(vals), torch.from_numpy(mn),
                       torch.from_numpy(sc), None)

    def encode_block_sr(self, flat=None, tensors=None, base=None, seed=0, **_):
        x, segs, b = self._input(flat, tensors, base)
        mn, sc, _, stream = encode_block(x, segs, self.bits, seed, base=b)
        return torch.from_numpy(mn), torch.from_numpy(sc), torch.from_numpy(stream)


class SROracleBackend(BlockOracleBackend):
    name = "sr-oracle"

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        return SROraclePlan(sizes, ratio, bits, clients)
