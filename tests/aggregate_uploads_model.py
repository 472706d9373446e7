"""A numpy model of coalac_aggregate_uploads: tests/aggregate_model.py's arithmetic over uploads that each live in
their own buffers — the idx / vals arrays of an upload (kind ENTRIES), or its wire v3 stream, decoded unit by unit and
field by field as include/coalac.h defines it (kind COMPACT).

A tests/aggregate_inputs.py Payload (the batched, concatenated form coalac_aggregate takes) is cut into its clients'
uploads by split(); pack() makes an upload's stream with wire.pack_entries. aggregate() below then defines the result,
for corrupt starts and corrupt field words too, except where a client's unit range applies one position twice
(aggregate_model.RacyPayload, as there).

UploadsOraclePlan / UploadsOracleBackend put the model behind the plan interface (CodecPlan.aggregate_uploads), for the
host-routing tests. Test infrastructure only (no GPU)."""
from dataclasses import dataclass

import numpy as np
import torch

from coala_amd.compression import wire
from oracle import codec_oracle as O
from tests import aggregate_model as M
from tests.oracle_backend import OracleBackend, OraclePlan

F32 = np.float32
UNIT = M.UNIT


@dataclass
class Upload:
    idx: np.ndarray      # int32[K]  (None once only the stream is kept)
    vals: np.ndarray     # uint8[K] codes, or float32[K] at bits 32
    mn: np.ndarray       # float32[T]
    scale: np.ndarray
    ustart: np.ndarray   # int32[U0]
    packed: np.ndarray = None  # uint32[ceil(K w / 32)]: the wire v3 stream


def split(p):
    """The Payload's clients as separate uploads of the ONE layout (copies: nothing aliases the batched arrays)."""
    t = p.table
    C, K, T, U0 = t.clients, t.total_k_per_client, len(t.sizes), t.units_per_client
    return [Upload(p.idx[c * K:(c + 1) * K].copy(), p.vals[c * K:(c + 1) * K].copy(), p.mn[c * T:(c + 1) * T].copy(),
                   p.scale[c * T:(c + 1) * T].copy(), p.ustart[c * U0:(c + 1) * U0].copy()) for c in range(C)]


def pack(u, bits):
    """The upload with its wire v3 stream (wire.pack_entries of its idx / vals)."""
    u.packed = np.ascontiguousarray(wire.pack_entries(u.idx, u.vals, bits)).astype(np.uint32)
    return u


def one_layout_segs(p):
    """int64[T, 4] (in_off, n, k, out_off) of one client's layout: the batched table's first T rows."""
    return p.segs[:len(p.table.sizes)].copy()


def fields(packed, j, w):
    """Fields j (an int64 array) of a stream as the kernel reads them: the word that holds the field's first bit, and
    the next word only where the field straddles and the word lies inside the stream (else zeros)."""
    bit = np.asarray(j, dtype=np.int64) * w
    wd, sh = bit >> 5, (bit & 31).astype(np.uint64)
    words = np.concatenate([np.asarray(packed, dtype=np.uint32), np.zeros(1, np.uint32)]).astype(np.uint64)
    two = words[wd] | np.where(sh + np.uint64(w) > 32, words[wd + 1] << np.uint64(32), np.uint64(0))
    return ((two >> sh) & np.uint64((1 << w) - 1)).astype(np.int64)


def decode_client_segment_stream(u, t, g0, n_units, n, k, oo, bits, base, counts, racy=None):
    """x_i of one client's segment from its stream, unit by unit: for every entry position oo + e of the unit's
    clamped range the field's low 12 bits are the position inside the unit (dropped when >= the unit's length) and
    the rest its code (bits 32: the value is vals[oo + e]). racy: a bool[n] in which a unit whose range applies one
    position twice is marked, whole, instead of raising RacyPayload (the last such entry wins here)."""
    w = wire.field_bits(bits)
    d = np.zeros(n, dtype=F32)
    nu = M.units_of(n)
    us = np.asarray(u.ustart).astype(np.int64) & M.M32
    for j in range(nu):
        start = j * UNIT
        length = min(UNIT, n - start)
        lo, hi = M.unit_range(us, g0 + j, n_units, k, length, j == nu - 1)
        e = np.arange(oo + lo, oo + hi)
        f = fields(u.packed, e, w)
        pos = f & 0xFFF
        ok = pos < length
        p = pos[ok]
        if np.unique(p).size != p.size:
            if racy is None:
                raise M.RacyPayload(f"unit {g0 + j}: entries [{lo}, {hi}) apply a position twice")
            racy[start:start + length] = True
        if bits == O.RAW_BITS:
            d[start + p] = u.vals[e[ok]]
        else:
            d[start + p] = O.dequantize((f[ok] >> 12).astype(np.uint8), u.mn[t], u.scale[t])
        counts[j] = (int(ok.sum()), int((~ok).sum()))
    if base is None:
        return d
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(base, dtype=F32) + d


def aggregate(uploads, segs, bits, weights, total, mode, out, base=None, avg_mask=None, kind="entries", racy=None):
    """coalac_aggregate_uploads into `out` (fp32, any fill): only the layout's segment elements are written. segs:
    the ONE layout's int64[T, 4]; kind "entries" reads u.idx / u.vals, "compact" u.packed (and u.vals at bits 32).
    Returns aggregate_model.Counts; raises RacyPayload where the GPU result is undefined — or (kind "compact"), given
    racy, a bool array like `out`, marks there every unit in which some client applies a position twice."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    T, C = len(segs), len(uploads)
    nus = [M.units_of(segs[t, 1]) for t in range(T)]
    ubeg = np.concatenate([[0], np.cumsum(nus)]).astype(np.int64)
    U0 = int(ubeg[-1])
    w = np.asarray(weights, dtype=np.float64).astype(F32)
    tot = F32(total)
    units = np.zeros((C, U0, 2), dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(T):
            off0, n, k, oo = (int(v) for v in segs[t])
            b = None if base is None else base[off0:off0 + n]

            def x_of(c):
                u, cnt = uploads[c], units[c, ubeg[t]:ubeg[t + 1]]
                assert u.ustart.size == U0
                if kind == "compact":
                    return decode_client_segment_stream(u, t, int(ubeg[t]), U0, n, k, oo, bits, b, cnt,
                                                        None if racy is None else racy[off0:off0 + n])
                return M.decode_client_segment(np.asarray(u.idx).astype(np.int64) & M.M32, u.vals, u.mn[t], u.scale[t],
                                               np.asarray(u.ustart).astype(np.int64) & M.M32, int(ubeg[t]), U0, n, k,
                                               oo, bits, b, cnt)

            if avg_mask is not None and not avg_mask[t]:
                out[off0:off0 + n] = x_of(0)
                for c in range(1, C):
                    x_of(c)
                continue
            acc = None
            for c in range(C):
                term = x_of(c) * w[c]
                acc = term if acc is None else acc + term
            if mode == O.AGG_SUM:
                out[off0:off0 + n] = acc
            else:
                out[off0:off0 + n] = acc / tot if mode == O.AGG_DIV else acc * (F32(1.0) / tot)
    return M.Counts(int(units[:, :, 0].sum()), int(units[:, :, 1].sum()), units)


MODES = {"div": O.AGG_DIV, "recip": O.AGG_RECIP, "sum": O.AGG_SUM}


class UploadsOraclePlan(OraclePlan):
    calls = []  # (class-wide: the routing tests read the kinds of the launches)

    def aggregate_uploads(self, idxs, packeds, vals, mns, scales, ustarts, weights, total=None, base=None, out=None,
                          mode="div", avg_mask=None, kind="entries", **_):
        type(self).calls.append(kind)
        total = float(sum(weights)) if total is None else float(total)
        np_ = lambda t: None if t is None else t.numpy()  # noqa: E731
        ups = [Upload(np_(idxs[i]), np_(vals[i]), np_(mns[i]), np_(scales[i]), np_(ustarts[i]),
                      None if kind == "entries" else packeds[i].numpy().view(np.uint32)) for i in range(len(weights))]
        res = np.zeros(self.table.span, dtype=np.float32)
        aggregate(ups, self.table.segs.astype(np.int64), self.bits, weights, total, MODES[mode], res,
                  base=None if base is None else base.detach().cpu().numpy(), avg_mask=avg_mask, kind=kind)
        if out is not None:
            out[:res.size].copy_(torch.from_numpy(res))
            return out
        return torch.from_numpy(res)


class UploadsOracleBackend(OracleBackend):
    name = "uploads-oracle"

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        return UploadsOraclePlan(sizes, ratio, bits, clients)
