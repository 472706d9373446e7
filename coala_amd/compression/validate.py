"""Validation of an untrusted COALAQ1 blob's header and index lists (numpy only: a process that only checks
blobs does not load torch)."""
import numpy as np

from ._cache import IdentityCache
from .spec import UNIT, VALID_BITS, SegmentTable, k_for
from .wire import check_header, is_dense

MODES = ("delta", "weights")

_VALIDATED = IdentityCache(32)  # (entries; ratio, n_segments, total_k) -> (ns_rep, first, units) of a layout


def validate(header, idx, ustart=None):
    """Check an (untrusted) blob's index lists: per fp32 segment, k = k_for(n, ratio) entries, strictly
    increasing, inside [0, n); and (wire v2) the per-unit starts: exactly the lower bounds of every unit's
    first element in its segment's list. The decode kernels are bounds-safe anyway; this turns a corrupt
    upload into an error instead of a silently wrong model. The header's structure is checked once per layout
    (headers of one layout share their entries list: wire._parse_header); the indices every call."""
    if header.get("bits") not in VALID_BITS or header.get("mode") not in MODES:
        raise ValueError("COALAQ1: bad bits/mode")
    ns_rep, first, units = _VALIDATED.get(
        header["entries"], (float(header["ratio"]), int(header["n_segments"]), int(header["total_k"])),
        lambda: _validate_layout(header))
    check_header(header, on_wire=True)  # its format's own rules (wire v5: one range per block of this layout)
    if is_dense(header, on_wire=True):  # implied indices (0..n-1 per segment): nothing to check beyond the layout
        if idx.size != 0 or ustart is not None:
            raise ValueError("COALAQ1: a dense update carries no indices or starts")
        return
    if idx.size != int(header["total_k"]):
        raise ValueError("COALAQ1: kept-entry count mismatch")
    if ustart is not None and (units is None or int(header.get("n_units", -1)) != units[0].size
                               or ustart.size != units[0].size):
        raise ValueError("COALAQ1: per-unit start count mismatch")
    if ns_rep is None:
        return
    if idx.size and (int(idx.min()) < 0 or np.any(idx >= ns_rep)):
        raise ValueError("COALAQ1: index out of range")
    d = np.diff(idx, prepend=np.int32(-1))
    if np.any((d <= 0) & ~first):
        raise ValueError("COALAQ1: indices not strictly increasing")
    if ustart is not None:
        # every entry's global unit (non-decreasing, the indices being sorted per segment): a unit starts where
        # the first entry of that unit or a later one sits, relative to its segment's first entry
        unit_seg_out, unit_base_rep, arange_u = units
        gu = unit_base_rep + (idx >> 12)
        if not np.array_equal(np.searchsorted(gu, arange_u) - unit_seg_out, ustart):
            raise ValueError("COALAQ1: per-unit starts inconsistent with the indices")


def _validate_layout(header):
    segs = [e for e in header["entries"] if e["kind"] == "seg"]
    if len(segs) != int(header["n_segments"]):
        raise ValueError("COALAQ1: segment count mismatch")
    # the decoder slices its output with the offsets it derives itself (SegmentTable of the sizes); a
    # header whose own offsets / sizes disagree with that, or with the tensor shapes, is corrupt
    table = SegmentTable([e["n"] for e in segs], header["ratio"], 1) if segs else None
    for i, e in enumerate(segs):
        if int(e["seg"]) != i or int(e["n"]) != int(np.prod(e["shape"], dtype=np.int64)) or \
                int(e["off"]) != table.offsets[i]:
            raise ValueError(f"COALAQ1: segment entry {e.get('name')!r} has inconsistent seg/n/off/shape")
    ks = np.array([k_for(e["n"], header["ratio"]) for e in segs], dtype=np.int64)
    if int(ks.sum()) != int(header["total_k"]):
        raise ValueError("COALAQ1: kept-entry count mismatch")
    if not ks.size:
        return None, None, None
    ns = np.array([e["n"] for e in segs], dtype=np.int32)
    ns_rep = np.repeat(ns, ks)  # each entry's segment size
    first = np.zeros(int(ks.sum()), dtype=bool)  # each segment's first entry (no predecessor to compare)
    first[np.cumsum(ks)[:-1][ks[1:] > 0] if ks.size > 1 else []] = True
    first[0] = True
    # wire v2: per unit its segment's first entry; per entry its segment's first global unit
    nu = (ns.astype(np.int64) + UNIT - 1) // UNIT
    seg_out = np.concatenate([[0], np.cumsum(ks)[:-1]]).astype(np.int64)
    unit_base = np.concatenate([[0], np.cumsum(nu)[:-1]]).astype(np.int32)
    units = (np.repeat(seg_out, nu), np.repeat(unit_base, ks), np.arange(int(nu.sum()), dtype=np.int32))
    return ns_rep, first, units
