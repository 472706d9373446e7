"""Hand-built payloads for the sparse decode (coalac_decode: k_decode_lds) and for k_ef_commit: the generators shared by
tests/test_decode_model_cpu.py (which proves every claim made here on the finished payloads, and the model equal to the
oracle) and tests/test_gpu_decode_structure.py (which feeds them to the kernels). numpy only.

k_decode_lds is compiled 16 ways: raw fp32 values or codes x base or none x high_ratio (8 entry chunks of 64 in
registers, or 1) x latency plan (2 waves per unit) or batch plan (1 wave per unit, XCD block order, non-temporal
stores). A tile pass covers 1024 elements of a unit with a base and 2048 without; a latency plan's two waves split the
unit at 2048. What picks the variant:

  raw         bits == 32
  base        a base is passed
  high_ratio  the largest k / n over the segments of more than 1024 elements is > 0.02. k = ceil(n * ratio) rounds up,
              so ratio 0.02 itself IS a high_ratio plan for every size used here (41 / 2048 > 0.02): the class without
              it is built at RATIO_LOW = 0.019, and RATIO_TINY; ratio 0.02 runs as a third ratio
  batch       more than LATENCY_PLAN_UNITS units: the structured segments (16 units) before and after one filler segment
              of 8194 x 4096 elements, n_units = 8226 (n_units % 4 == 2: the last block has idle waves;
              ceil(n_units / 4) % 8 == 1: the XCD remap has a remainder)"""
from dataclasses import dataclass, replace
from functools import lru_cache

import numpy as np

from coala_amd.compression.spec import LATENCY_PLAN_UNITS, UNIT, SegmentTable, k_for, units_of
from tests import aggregate_inputs as I
from tests import aggregate_model as M
from tests.aggregate_inputs import F32, PAD, S6, S7, S8, SENTINEL, SIZES, even, pour, unit_lens

FILLER_UNITS = 8194  # 16 + 8194 + 16 = 8226 units
FILLER = FILLER_UNITS * UNIT
RATIO_LOW = 0.019    # ks 1, 6, 39, 39, 78, 78, 117, 234, 195: no large segment above 0.02
RATIO_EDGE = I.RATIO  # 0.02: every k rounds up past 0.02 n, a high_ratio plan with at most 246 entries per segment
RATIO_HIGH = 0.1     # ks 1, 30, 205, 205, 410, 410, 615, 1229, 1025: a unit can hold 513 entries
RATIO_TINY = I.RATIO_TINY
HIGH_RATIO = 0.02    # mirrors coalac.hip
TILE = 1024          # elements of the smallest tile pass (4 rows); the 8-row pass and the 2-wave split are 2048
S4, S5 = 4, 5        # 4096 (one full unit) and 4097 (a full unit and a unit of 1)
FULL_SIZES = SIZES + [53 * UNIT + 1]  # k = 4125 / 21709: room for a unit with every position kept; len % 4 == 1
LAST_SIZES = SIZES + [2 * UNIT + 2]   # a last unit with len % 4 == 2
FILLER_FULL, FILLER_EMPTY = 5, 7      # filler units with every position kept / with no entry (where k allows)


@dataclass
class DecodePayload(I.Payload):
    filler_key: tuple = None  # batch: (ratio, bits, base given) while the filler's entries are the cached ones


def plan_sizes(batch, sizes=SIZES):
    return list(sizes) + [FILLER] + list(sizes) if batch else list(sizes)


def is_batch(table):
    return table.n_units > LATENCY_PLAN_UNITS


def is_high_ratio(table):
    return max(k / n for n, k in zip(table.sizes, table.ks) if n > 1024) > HIGH_RATIO


def inside(table, size):
    m = np.zeros(size, bool)
    for off, n in zip(table.offsets, table.sizes):
        m[off:off + n] = True
    return m


@lru_cache(maxsize=None)
def filler_entries(ratio):
    """(idx int64[k], starts int64[FILLER_UNITS]) of the filler segment, placed in one vectorised step: per-unit counts around
    k / FILLER_UNITS (spread over both sides of 64 at the low ratios and of 512 at the high one), unit FILLER_FULL with every
    position kept and unit FILLER_EMPTY with none; the j-th of a unit's c entries at a random position of the j-th of c
    equal stretches of the unit (ascending, unique)."""
    k, nu = k_for(FILLER, ratio), FILLER_UNITS
    rng = np.random.default_rng([77, int(ratio * 1e6)])
    cnt = np.full(nu, k // nu, np.int64)
    cnt[:k % nu] += 1
    if k // nu >= 8:
        d = rng.integers(0, (150 if ratio >= 0.05 else 40) + 1, nu // 2)
        cnt[0::2] += d
        cnt[1::2] -= d
        cnt[FILLER_EMPTY + 1] += cnt[FILLER_EMPTY]
        cnt[FILLER_EMPTY] = 0
        need = UNIT - cnt[FILLER_FULL]
        cnt[FILLER_FULL] = UNIT
        cnt[16:16 + need] -= 1
    assert cnt.sum() == k and cnt.min() >= 0 and cnt.max() <= UNIT
    start = np.cumsum(cnt) - cnt
    j = np.arange(k) - np.repeat(start, cnt)
    c = np.repeat(cnt, cnt)
    lo = j * UNIT // c
    pos = lo + (rng.random(k) * ((j + 1) * UNIT // c - lo)).astype(np.int64)
    idx = np.repeat(np.arange(nu), cnt) * UNIT + pos
    for a in (idx, start):
        a.flags.writeable = False
    return idx, start


@lru_cache(maxsize=None)
def _filler_vals(ratio, bits):
    k = k_for(FILLER, ratio)
    rng = np.random.default_rng([78, bits])
    v = (rng.standard_normal(k) * 0.1).astype(F32) if bits == 32 else rng.integers(0, 1 << bits, k).astype(np.uint8)
    v.flags.writeable = False
    return v


@lru_cache(maxsize=1)
def _filler_base():
    b = np.random.default_rng([79]).standard_normal(FILLER).astype(F32)
    b.flags.writeable = False
    return b


def _base(table):
    """A random base over the whole span, pads included; a batch plan's filler always gets the same stretch."""
    span, rng = table.span_per_client, np.random.default_rng([79, len(table.sizes)])
    if not is_batch(table):
        return rng.standard_normal(span).astype(F32)
    b = np.empty(span, F32)
    off = table.offsets[table.sizes.index(FILLER)]
    b[:off] = rng.standard_normal(off)
    b[off:off + FILLER] = _filler_base()
    b[off + FILLER:] = rng.standard_normal(span - off - FILLER)
    return b


def make(bits, ratio, batch, seed, sizes=SIZES, counts=None, style=None, base=False):
    """A valid one-client payload of the plan plan_sizes(batch, sizes). counts(t, lens, k) / style(t, u): as
    aggregate_inputs.build's, t counting inside one copy of `sizes` (a batch plan's two copies get the same structure
    from different seeds)."""
    cf = None if counts is None else (lambda c, t, lens, k: counts(t, lens, k))
    sf = None if style is None else (lambda c, t, u: style(t, u))
    parts = [I.build(bits, 1, seed, ratio=ratio, sizes=sizes, counts=cf, style=sf)]
    if batch:
        fi, fs = filler_entries(ratio)
        fm, fsc = (0.0, 0.0) if bits == 32 else (-0.05, 3e-4)
        parts.append(I.Payload(None, bits, fi.astype(np.int32), _filler_vals(ratio, bits),
                               np.array([fm], F32), np.array([fsc], F32), fs.astype(np.int32), [1]))
        parts.append(I.build(bits, 1, seed + 1000, ratio=ratio, sizes=sizes, counts=cf, style=sf))
    table = SegmentTable(plan_sizes(batch, sizes), ratio, 1)
    cat = lambda name: np.concatenate([getattr(q, name) for q in parts])  # noqa: E731
    p = DecodePayload(table, bits, cat("idx"), cat("vals"), cat("mn"), cat("scale"), cat("ustart"), [1],
                      _base(table) if base else None, None,
                      (ratio, bits, bool(base)) if batch else None)
    assert p.idx.size == table.total_k and p.ustart.size == table.n_units
    return p


def structured(table):
    """Indices of the plan's structured (non-filler) segments."""
    return [t for t, n in enumerate(table.sizes) if n != FILLER]


def copy_of(table, t):
    """Segment t of one copy of the sizes -> the plan's segment indices holding it (one, or two in a batch plan)."""
    T = (len(table.sizes) - 1) // 2 if is_batch(table) else len(table.sizes)
    return [t, T + 1 + t] if is_batch(table) else [t]


def unit_positions(p, t, u):
    """Positions (relative to the unit, in payload order) of the entries of unit u of segment t, from the starts."""
    g = I.unit_begin(p.table)[t] + u
    oo, k = p.table.out_offsets[t], p.table.ks[t]
    lo = int(p.ustart[g])
    hi = k if u == units_of(p.table.sizes[t]) - 1 else int(p.ustart[g + 1])
    return p.idx[oo + lo:oo + hi].astype(np.int64) - u * UNIT


# ------------------------------------------------------------------------------------------------------------------
# valid cases: name -> Case. What each is built to reach is in its comment; tests/test_decode_model_cpu.py asserts it
# on the finished payloads.
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    ratios: tuple
    sizes: list = None
    counts: object = None
    style: object = None
    post: object = None      # post(p, rng) -> p: changes applied to the finished payload
    base_only: bool = False
    commit: bool = True      # run through k_ef_commit too (not the special values: the commit model leaves them out)
    seed: int = 0


def _counts_64(t, lens, k):
    """NCH = 1 seam: units of 64, 65, 63, 1, 129 and 0 entries; segment 7's last unit is empty (lo == hi == k)."""
    if t == S6:
        return pour(lens, k, [64, None])
    if t == S7:
        return pour(lens, k, [65, 63, None, 0])
    if t == S8:
        return pour(lens, k, [1, 129, None])
    return even(lens, k)


def _counts_128(t, lens, k):
    """k_ef_commit's step of 128: units of 127, 128, 0 and 1 entries; segment 8's last unit is empty."""
    if t == S6:
        return pour(lens, k, [0, None])
    if t == S7:
        return pour(lens, k, [127, 0, None, 1])
    if t == S8:
        return pour(lens, k, [128, None, 0])
    return even(lens, k)


def _counts_512(t, lens, k):
    """NCH = 8 seam (ratio 0.1 only): units of 512, 511, 513, 512 and 576 entries."""
    if t == S6:
        return pour(lens, k, [576, None])
    if t == S7:
        return pour(lens, k, [512, 511, None, 1])
    if t == S8:
        return pour(lens, k, [513, None, 0])
    return even(lens, k)


def _counts_full(t, lens, k):
    """Segment 9 of FULL_SIZES: its first unit keeps all 4096 positions, its last (one element) that element."""
    if t == 9:
        return pour(lens, k, [UNIT] + [None] * (len(lens) - 2) + [1])
    return even(lens, k)


def _counts_tiny(t, lens, k):
    """RATIO_TINY: k below the unit count; even segments keep their k in the first units, odd ones in the last."""
    nu = len(lens)
    return pour(lens, k, [None] * nu, dump=range(nu) if t % 2 == 0 else reversed(range(nu)))


def _counts_last(t, lens, k):
    """Every last unit keeps at least one entry (where k allows): its last element, by the style."""
    if len(lens) == 1:
        return [k]
    return pour(lens, k, [None] * (len(lens) - 1) + [min(lens[-1], 3)])


def _style_last(sizes):
    return lambda t, u: "last" if u == units_of(sizes[t]) - 1 else "any"


def _permute(p, rng):
    """Entries shuffled inside every unit's range (idx and values together): starts and positions stay valid."""
    t = p.table
    seg = np.repeat(np.arange(len(t.sizes)), t.ks)
    g = np.asarray(I.unit_begin(t))[seg] + (p.idx.astype(np.int64) >> 12)
    order = np.lexsort((rng.random(p.idx.size), g))
    assert np.array_equal(g[order], g)
    return replace(p, idx=p.idx[order], vals=p.vals[order], filler_key=None)


RAW_SPECIALS = [-0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-45, 3e-39]
BASE_SPECIALS = [-0.0, np.nan, np.inf, -np.inf, 1e-40, -1e-45]


def _special_values(rot):
    def post(p, rng):
        """Codes: mn / scale of aggregate_inputs.SPECIAL_RANGES, rotated over the structured segments from `rot` on.
        Raw: every fifth value of a structured segment one of -0.0, NaN, +-Inf and denormals."""
        t = p.table
        if p.bits != 32:
            mn, scale = p.mn.copy(), p.scale.copy()
            for j, s in enumerate(structured(t)):
                mn[s], scale[s] = I.SPECIAL_RANGES[(rot + j) % len(I.SPECIAL_RANGES)]
            return replace(p, mn=mn, scale=scale)
        vals = p.vals.copy()
        for s in structured(t):
            e = np.arange(t.out_offsets[s] + (rot + s) % 5, t.out_offsets[s] + t.ks[s], 5)
            vals[e] = np.asarray(RAW_SPECIALS, F32)[(np.arange(e.size) + s) % len(RAW_SPECIALS)]
        return replace(p, vals=vals)
    return post


def _special_base(p, rng):
    """-0.0, NaN, +-Inf and denormal bases in every structured segment: under every third kept entry and at every
    seventh position that is not kept (base + 0.0f: a -0.0 base comes out as +0.0)."""
    t = p.table
    b = p.base
    sp = np.asarray(BASE_SPECIALS, F32)
    for s in structured(t):
        off, n = t.offsets[s], t.sizes[s]
        kept = p.idx[t.out_offsets[s]:t.out_offsets[s] + t.ks[s]].astype(np.int64)
        free = np.setdiff1d(np.arange(n), kept)
        for pos in (kept[s % 3::3], free[s % 7::7]):
            b[off + pos] = sp[(np.arange(pos.size) + s) % sp.size]
    return replace(p, base=b)


BOTH = (RATIO_LOW, RATIO_HIGH)
CASES = {
    "counts_64": Case((RATIO_LOW, RATIO_EDGE, RATIO_HIGH), counts=_counts_64, seed=1),
    "counts_128": Case(BOTH, counts=_counts_128, seed=2),
    "counts_512": Case((RATIO_HIGH,), counts=_counts_512, seed=3),
    # latency plans; a batch plan's filler has such a unit in every payload (FILLER_FULL)
    "full_unit": Case(BOTH, sizes=FULL_SIZES, counts=_counts_full, seed=4),
    "empty_tiny": Case((RATIO_TINY,), counts=_counts_tiny, seed=5),
    # 0, every multiple of 1024 with its predecessor, len - 1: the tile sizes of both passes and the 2-wave split
    "seams": Case(BOTH, style=lambda t, u: "seams", seed=6),
    # p kept in the first pass, p + 1024 m never: a tile that is not zeroed between passes shows p's value again
    "slot_twins": Case(BOTH, style=lambda t, u: "twins", seed=7),
    # only the last 1024-element stretch keeps entries
    "slot_twins_inverse": Case(BOTH, style=lambda t, u: "twins_last", seed=8),
    # all of a unit's entries in the one pass (t + u) % 4
    "one_pass_only": Case(BOTH, style=lambda t, u: f"pass{(t + u) % 4}", seed=9),
    # len % 4 = 1, 2, 3 with len - 1 kept: the dword-store path
    "last_element": Case(BOTH, sizes=LAST_SIZES, counts=_counts_last, style=_style_last(LAST_SIZES), seed=10),
    "permuted_within_unit": Case(BOTH, counts=_counts_64, post=_permute, seed=11),
    "special_values_a": Case(BOTH, post=_special_values(0), commit=False, seed=12),
    "special_values_b": Case((RATIO_LOW,), post=_special_values(6), commit=False, seed=13),
    "special_base": Case(BOTH, post=_special_base, base_only=True, seed=14),
}
ALL_BITS_CASE = "counts_64"  # the case run at widths 1 and 5 too
LATENCY_ONLY = ("full_unit",)


def valid(name, ratio, batch, bits, base):
    c = CASES[name]
    p = make(bits, ratio, batch, c.seed, sizes=SIZES if c.sizes is None else c.sizes, counts=c.counts, style=c.style,
             base=base)
    if c.post is not None:
        p = c.post(p, np.random.default_rng([c.seed, bits, int(batch)]))
    return p


def _valid_cases():
    out = []
    for batch in (False, True):
        for ratio in (RATIO_LOW, RATIO_TINY, RATIO_EDGE, RATIO_HIGH):
            for bits in (8, 32, 1, 5):
                for base in (True, False):  # (one (ratio, bits, base) of a batch plan after the other: the filler's
                    for name, c in CASES.items():  # expected elements are computed once per such group)
                        if ratio not in c.ratios or (batch and name in LATENCY_ONLY) or (c.base_only and not base):
                            continue
                        if bits in (1, 5) and (name != ALL_BITS_CASE or ratio == RATIO_EDGE or not base):
                            continue
                        if ratio == RATIO_EDGE and batch:
                            continue
                        out.append((name, ratio, batch, bits, base))
    return out


# every (name, ratio, batch, bits, base) the GPU file runs
VALID_CASES = _valid_cases()


# ------------------------------------------------------------------------------------------------------------------
# corrupt payloads of the batch plan whose result the model defines
# ------------------------------------------------------------------------------------------------------------------
def pos_ge_len(p, rng):
    """Half the entries of every partial last unit moved to len <= pos < 4096 (len, len + 1, ...: the alignment pad
    after the segment and the next segment's first elements, were they not dropped)."""
    t = p.table
    idx = p.idx.copy()
    for s in structured(t):
        n, u = t.sizes[s], units_of(t.sizes[s]) - 1
        L = n - u * UNIT
        if L == UNIT:
            continue
        lo = t.out_offsets[s] + int(p.ustart[I.unit_begin(t)[s] + u])
        m = (t.out_offsets[s] + t.ks[s] - lo + 1) // 2
        idx[lo:lo + m] = u * UNIT + L + np.arange(m)
        assert m == 0 or L + m <= UNIT
    return replace(p, idx=idx)


CORRUPTIONS = dict(I.CORRUPTIONS, pos_ge_len=pos_ge_len)
CORRUPT_CASES = [(kind, ratio, bits, base) for kind in CORRUPTIONS
                 for ratio, bits, base in ((RATIO_LOW, 8, True), (RATIO_HIGH, 32, False))]
APPLIES_NOTHING = I.APPLIES_NOTHING
CORRUPT_ORIGINAL = "counts_128"  # (every partial last unit but segment 8's holds entries)


def corrupt(kind, ratio, bits, base):
    seed = 300 + list(CORRUPTIONS).index(kind)
    p = valid(CORRUPT_ORIGINAL, ratio, True, bits, base)
    return replace(CORRUPTIONS[kind](p, np.random.default_rng([seed, bits])), filler_key=None)


# ------------------------------------------------------------------------------------------------------------------
# the expected buffers
# ------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=1)
def _filler_expected(ratio, bits, base):
    """The model's elements and unit counts of the (cached) filler segment of a valid batch payload."""
    p = make(bits, ratio, True, 0, base=base)
    s = len(SIZES)
    assert p.table.sizes[s] == FILLER
    out = np.empty(p.table.span_per_client, F32)
    counts = M.decode(p.idx, p.vals, p.mn, p.scale, p.ustart, p.segs, p.bits, out, base=p.base, segments=[s])
    off, g = p.table.offsets[s], I.unit_begin(p.table)[s]
    return out[off:off + FILLER].copy(), counts.units[g:g + FILLER_UNITS].copy()


def expected_decode(p):
    """(the whole expected buffer of span + PAD elements, Counts) of decoding p into a sentinel-filled buffer. A valid
    batch payload's filler elements are the model's too, computed once per (ratio, bits, base) and reused while the
    filler's entries are the cached ones."""
    t = p.table
    out = np.full(t.span_per_client + PAD, SENTINEL, F32)
    if p.filler_key is None:
        return out, M.decode(p.idx, p.vals, p.mn, p.scale, p.ustart, p.segs, p.bits, out, base=p.base)
    s = (len(t.sizes) - 1) // 2
    fe, fu = _filler_expected(*p.filler_key)
    out[t.offsets[s]:t.offsets[s] + FILLER] = fe
    c = M.decode(p.idx, p.vals, p.mn, p.scale, p.ustart, p.segs, p.bits, out, base=p.base, segments=structured(t))
    units = c.units
    g = I.unit_begin(t)[s]
    units[g:g + FILLER_UNITS] = fu
    return out, M.Counts(int(units[:, 0].sum()), int(units[:, 1].sum()), units)


@lru_cache(maxsize=2)
def _residual(sizes, batch):
    t = SegmentTable(plan_sizes(batch, sizes), 1.0, 1)
    r = np.random.default_rng([80, len(sizes)]).standard_normal(t.span_per_client + PAD).astype(F32)
    r[~inside(t, r.size)] = SENTINEL
    r.flags.writeable = False
    return r


def residual(table):
    """A random residual memory over span + PAD elements with the sentinel in every pad and in the tail (read-only)."""
    T = (len(table.sizes) - 1) // 2 if is_batch(table) else len(table.sizes)
    return _residual(tuple(table.sizes[:T]), is_batch(table))
