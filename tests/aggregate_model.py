"""A plain numpy model of coalac_aggregate (k_aggregate) that honours the payload's per-unit starts.

oracle.codec_oracle.aggregate decodes whole segments from their idx lists and never looks at the starts. The kernels
decode unit by unit: a unit's entry range [lo, hi) comes from the (untrusted) starts, clamped, and an entry of that
range is applied only where its position lies inside the unit. This model restates exactly that, with the oracle's
arithmetic (oracle/codec_oracle.py aggregate, line by line) on top, so it defines the result for corrupt starts and
indices too — everything except a range that applies two entries to one position, which is a race on the GPU and has
no expected value: the model raises RacyPayload there.

Test infrastructure only (numpy; no torch, no GPU)."""
from collections import namedtuple

import numpy as np

from oracle import codec_oracle as O

F32 = np.float32
UNIT = O.UNIT
M32 = np.int64(0xFFFFFFFF)

# applied / dropped: entries of some unit's clamped range whose position lies inside / outside that unit, over the
# whole payload; units: the same two counts per (client, unit of the client's layout), int64[clients, U0, 2]
Counts = namedtuple("Counts", "applied dropped units")


class RacyPayload(ValueError):
    """A (client, unit) range applies two entries to the same position: the kernel's result is a race."""


def units_of(n):
    return (int(n) + UNIT - 1) // UNIT


def unit_range(ustart, g, n_units, k, length, last):
    """The clamped entry range of unit g (index into the whole plan's starts, read as uint32), as the kernels
    compute it: the next start is read at min(g + 1, n_units - 1), a segment's last unit ends at k."""
    lo = min(int(ustart[g]), k)
    nxt = k if last else int(ustart[min(g + 1, n_units - 1)])
    hi = max(lo, min(min(nxt, k), lo + length))
    return lo, hi


def decode_client_segment(idx, vals, mn, scale, ustart, g0, n_units, n, k, oo, bits, base, counts):
    """x_i of one client's segment, unit by unit: base + d_i where an entry is applied, base + 0.0f (or +0.0f
    without a base) elsewhere. idx / ustart: int64 arrays holding the uint32 values the kernel reads; g0: the
    segment's first unit in the plan's starts; counts: int64[units of the segment, 2] to fill."""
    d = np.zeros(n, dtype=F32)
    nu = units_of(n)
    for j in range(nu):
        start = j * UNIT
        length = min(UNIT, n - start)
        lo, hi = unit_range(ustart, g0 + j, n_units, k, length, j == nu - 1)
        e = np.arange(oo + lo, oo + hi)
        pos = (idx[e] - start) & M32  # uint32 wrap-around
        ok = pos < length
        p = pos[ok]
        if np.unique(p).size != p.size:
            raise RacyPayload(f"unit {g0 + j}: entries [{lo}, {hi}) apply a position twice")
        v = vals[e[ok]]
        d[start + p] = v if bits == O.RAW_BITS else O.dequantize(v, mn, scale)
        counts[j] = (int(ok.sum()), int((~ok).sum()))
    if base is None:
        return d
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(base, dtype=F32) + d


def decode(idx, vals, mn, scale, ustart, segs, bits, out, base=None, segments=None):
    """coalac_decode (k_decode_lds) of a payload with the given starts into `out` (fp32, any fill): only the
    segments' elements are written, so a sentinel-filled `out` becomes the expected whole buffer. segs: the plan's
    [T, 4] rows; base: fp32 indexed like out, or None; segments: the rows to decode (default: all — the others' units
    are still counted past, their elements and counts left as they are). Returns Counts (units: int64[n_units, 2]);
    raises RacyPayload where the GPU result is undefined."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    idx = np.asarray(idx).astype(np.int64) & M32
    ustart = np.asarray(ustart).astype(np.int64) & M32
    n_units = int(ustart.size)
    nus = [units_of(n) for n in segs[:, 1]]
    ubeg = np.concatenate([[0], np.cumsum(nus)]).astype(np.int64)
    assert int(ubeg[-1]) == n_units, "starts do not match the layout"
    units = np.zeros((n_units, 2), dtype=np.int64)
    for s in range(len(segs)) if segments is None else segments:
        off, n, k, oo = (int(v) for v in segs[s])
        b = None if base is None else base[off:off + n]
        out[off:off + n] = decode_client_segment(idx, vals, mn[s], scale[s], ustart, int(ubeg[s]), n_units, n, k, oo,
                                                 bits, b, units[ubeg[s]:ubeg[s + 1]])
    return Counts(int(units[:, 0].sum()), int(units[:, 1].sum()), units)


def aggregate(idx, vals, mn, scale, ustart, segs, bits, clients, weights, total, mode, out, base=None,
              avg_mask=None):
    """coalac_aggregate of a payload with the given starts into `out` (fp32, any fill): only the elements of client
    0's segments are written, so a sentinel-filled `out` becomes the expected whole buffer. Arguments as
    oracle.codec_oracle.aggregate, plus ustart (int32[n_units], the clients' per-unit starts concatenated).
    Returns Counts; raises RacyPayload where the GPU result is undefined."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    T = len(segs) // clients
    idx = np.asarray(idx).astype(np.int64) & M32
    ustart = np.asarray(ustart).astype(np.int64) & M32
    n_units = int(ustart.size)
    U0 = n_units // clients
    nus = [units_of(segs[t, 1]) for t in range(T)]
    ubeg = np.concatenate([[0], np.cumsum(nus)]).astype(np.int64)
    assert int(ubeg[-1]) == U0 and U0 * clients == n_units, "starts do not match the layout"
    w = np.asarray(weights, dtype=np.float64).astype(F32)
    tot = F32(total)
    units = np.zeros((clients, U0, 2), dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(T):
            off0, n = int(segs[t, 0]), int(segs[t, 1])
            b = None if base is None else base[off0:off0 + n]

            def x_of(c):
                _, n_, k, oo = (int(v) for v in segs[c * T + t])
                s = c * T + t
                return decode_client_segment(idx, vals, mn[s], scale[s], ustart, c * U0 + int(ubeg[t]), n_units, n, k,
                                             oo, bits, b, units[c, ubeg[t]:ubeg[t + 1]])

            if avg_mask is not None and not avg_mask[t]:
                out[off0:off0 + n] = x_of(0)
                for c in range(1, clients):  # (counted, though the kernel never reads them)
                    x_of(c)
                continue
            acc = None
            for c in range(clients):
                term = x_of(c) * w[c]
                acc = term if acc is None else acc + term
            if mode == O.AGG_SUM:
                out[off0:off0 + n] = acc
            else:
                out[off0:off0 + n] = acc / tot if mode == O.AGG_DIV else acc * (F32(1.0) / tot)
    return Counts(int(units[:, :, 0].sum()), int(units[:, :, 1].sum()), units)
