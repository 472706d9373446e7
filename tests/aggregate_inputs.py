"""Hand-built uploads for the fused sparse aggregate (coalac_aggregate): the payload generators shared by
tests/test_aggregate_model_cpu.py (which proves them race-free and non-vacuous on the model) and
tests/test_gpu_aggregate_structure.py (which feeds them to the kernel). numpy only.

A payload is placed entry by entry: per client, segment and 4096-element unit a count and a set of positions, so a
case decides which of k_aggregate's branches each (unit, 64-client chunk, wave) takes. The plan fixes k per segment
(SegmentTable.ks); every generator places exactly that many entries."""
from dataclasses import dataclass, replace

import numpy as np

from coala_amd.compression.spec import UNIT, SegmentTable, units_of

F32 = np.float32
SENTINEL = F32(12345.0)
PAD = 64  # elements after span_per_client in every output buffer

# unit lengths: 1, 300, 2048, 2049 (the second wave owns one element), 4096, 4096 + 1, 4096 + 2049, 3 x 4096 + 1 and
# 2 x 4096 + 2051 (n % 4 == 3 in the last unit): full-row and partial-row bodies, one-wave and two-wave units
SIZES = [1, 300, 2048, 2049, 4096, 4097, 6145, 12289, 10243]
RATIO = 0.02        # ks 1, 6, 41, 41, 82, 82, 123, 246, 205: light (<= 64 per unit) and heavy units both possible
RATIO_TINY = 0.0002  # ks 1, 1, 1, 1, 1, 1, 2, 3, 3: k below the unit count of segment 7 (4 units)
S6, S7, S8 = 6, 7, 8  # the multi-unit segments 6145 (4096 + 2049), 12289 (3 x 4096 + 1), 10243 (2 x 4096 + 2051)


@dataclass
class Payload:
    table: SegmentTable
    bits: int
    idx: np.ndarray      # int32[K]
    vals: np.ndarray     # uint8[K] codes, or float32[K] at bits 32
    mn: np.ndarray       # float32[clients * T]
    scale: np.ndarray
    ustart: np.ndarray   # int32[clients * U0]
    weights: list
    base: np.ndarray = None   # float32[span_per_client] or None
    mask: list = None

    @property
    def clients(self):
        return self.table.clients

    @property
    def segs(self):
        return self.table.segs.astype(np.int64)


def unit_lens(n):
    return [min(UNIT, n - j * UNIT) for j in range(units_of(n))]


def unit_begin(table):
    """First unit (within one client's layout) of every segment."""
    nu = [units_of(n) for n in table.sizes]
    return [int(v) for v in np.cumsum([0] + nu[:-1])]


def pour(lens, k, wish, dump=None):
    """Per-unit counts summing to k: wish[u] (None: no wish) capped by the unit's length, the remainder poured into
    the units without a wish, in `dump` order if given (then into any unit with room). The cases' claims about the
    counts are asserted on the finished payload by the CPU tests, not here."""
    cnt = [0 if w is None else min(int(w), L) for w, L in zip(wish, lens)]
    over = sum(cnt) - k
    for u in reversed(range(len(lens))):
        d = min(max(over, 0), cnt[u])
        cnt[u] -= d
        over -= d
    rest = k - sum(cnt)
    order = list(dump) if dump is not None else [u for u, w in enumerate(wish) if w is None]
    for u in order + list(range(len(lens))):
        d = min(rest, lens[u] - cnt[u])
        cnt[u] += d
        rest -= d
    assert rest == 0 and sum(cnt) == k
    return cnt


def even(lens, k):
    """Counts in proportion to the unit lengths."""
    n = sum(lens)
    return pour(lens, k, [k * L // n for L in lens], dump=range(len(lens)))


def place(style, length, cnt, rng, c, C):
    """cnt ascending unique positions of a unit of `length` elements. Styles: any; upper / lower (one wave's half
    only, where it has room); edges (0, 2047, 2048, length - 1 first, client c starting at the c-th of them);
    disjoint (client c owns the positions c mod C, where they suffice). For the decode's tile passes
    (tests/decode_inputs.py): seams (0, every multiple of 1024 with its predecessor, length - 1 first); last
    (length - 1 first); passQ (only [1024 Q, 1024 (Q + 1)), where it has room); twins (pass0); twins_last (only the
    1024-element stretch that holds length - 1, where it has room)."""
    if cnt == 0:
        return np.zeros(0, np.int64)
    pool = np.arange(length)
    if style in ("seams", "last"):
        e = [length - 1] if style == "last" else [0] + [p for m in range(1024, length, 1024) for p in (m - 1, m)] + [length - 1]
        e = list(dict.fromkeys(e))[:cnt]
        more = rng.choice(np.setdiff1d(pool, e), cnt - len(e), replace=False) if cnt > len(e) else []
        return np.sort(np.concatenate([e, more]).astype(np.int64))
    if style in ("twins", "twins_last") or style.startswith("pass"):
        q = 0 if style == "twins" else (length - 1) // 1024 if style == "twins_last" else int(style[4:])
        if min(length, 1024 * (q + 1)) - 1024 * q >= cnt:
            pool = np.arange(1024 * q, min(length, 1024 * (q + 1)))
    elif style == "upper" and length - 2048 >= cnt:
        pool = np.arange(2048, length)
    elif style == "lower" and min(length, 2048) >= cnt:
        pool = np.arange(min(length, 2048))
    elif style == "disjoint" and len(range(c, length, C)) >= cnt:
        pool = np.arange(c, length, C)
    elif style == "edges":
        e = [p for p in dict.fromkeys((0, 2047, 2048, length - 1)) if 0 <= p < length]
        e = (e[c % len(e):] + e[:c % len(e)])[:cnt]
        more = rng.choice(np.setdiff1d(pool, e), cnt - len(e), replace=False) if cnt > len(e) else []
        return np.sort(np.concatenate([e, more]).astype(np.int64))
    return np.sort(rng.choice(pool, cnt, replace=False)).astype(np.int64)


def default_weights(C):
    return [(7 * i) % 23 for i in range(C)]


def build(bits, clients, seed, ratio=RATIO, sizes=SIZES, counts=None, style=None, same=False, base=False,
          weights=None, mask=None):
    """A valid payload with correct starts. counts(c, t, lens, k) -> per-unit counts (default: even);
    style(c, t, u) -> a place() style (default "any"); same: every client draws the same positions."""
    table = SegmentTable(sizes, ratio, clients)
    T, C = len(sizes), clients
    K, U0 = table.total_k_per_client, table.units_per_client
    rng = np.random.default_rng([seed, bits, clients])
    idx = np.zeros(C * K, np.int32)
    ustart = np.zeros(C * U0, np.int32)
    ub = unit_begin(table)
    for c in range(C):
        for t, (n, k) in enumerate(zip(sizes, table.ks)):
            lens = unit_lens(n)
            cnt = even(lens, k) if counts is None else counts(c, t, lens, k)
            assert len(cnt) == len(lens) and sum(cnt) == k and all(0 <= a <= L for a, L in zip(cnt, lens)), (c, t, cnt)
            oo, e = c * K + table.out_offsets[t], 0
            for u, (L, a) in enumerate(zip(lens, cnt)):
                prng = np.random.default_rng([seed, t, u] + ([] if same else [c]))
                pos = place("any" if style is None else style(c, t, u), L, a, prng, c, C)
                assert pos.size == a and np.all(np.diff(pos) > 0) and (a == 0 or (pos[0] >= 0 and pos[-1] < L))
                ustart[c * U0 + ub[t] + u] = e
                idx[oo + e:oo + e + a] = u * UNIT + pos
                e += a
    if bits == 32:
        vals = (rng.standard_normal(C * K) * 0.1).astype(F32)
        vals[::11] = F32(-0.0)  # kept -0.0 values
        mn, scale = np.zeros(C * T, F32), np.zeros(C * T, F32)
    else:
        vals = rng.integers(0, 1 << bits, C * K).astype(np.uint8)
        mn = (-np.abs(rng.standard_normal(C * T)) * 0.1).astype(F32)
        scale = (np.abs(rng.standard_normal(C * T)) * 1e-3 + 1e-5).astype(F32)
    b = (rng.standard_normal(table.span_per_client)).astype(F32) if base else None
    return Payload(table, bits, idx, vals, mn, scale, ustart, default_weights(C) if weights is None else weights, b,
                   mask)


def unit_counts(p):
    """int[clients, U0]: entries per client and unit, from the payload's (correct) starts."""
    t = p.table
    U0, ub = t.units_per_client, unit_begin(t)
    s = p.ustart.reshape(t.clients, U0).astype(np.int64)
    out = np.zeros_like(s)
    for ti, (n, k) in enumerate(zip(t.sizes, t.ks)):
        nu = units_of(n)
        ends = np.concatenate([s[:, ub[ti] + 1:ub[ti] + nu], np.full((t.clients, 1), k)], axis=1)
        out[:, ub[ti]:ub[ti] + nu] = ends - s[:, ub[ti]:ub[ti] + nu]
    return out


# ------------------------------------------------------------------------------------------------------------------
# structure cases: name -> builder(bits, base, seed) -> Payload. What each is built to reach in k_aggregate is in its
# docstring; tests/test_aggregate_model_cpu.py asserts those claims on the finished payloads.
# ------------------------------------------------------------------------------------------------------------------
HEAVY_J = (0, 15, 16, 63)  # heavy clients of the first chunk (AGG_DEPTH seam 15 | 16, chunk seam 63 | 64); 64 is chunk 1's


def mixed(bits, base, seed=1):
    """70 clients. Segment 8, unit 0: clients 0..63 light (0..64 entries, varying), client 64 heavy -> chunk 0 on the
    fast path, chunk 1 generic, in one unit. Segment 8, unit 1: clients 0, 15, 16, 63 heavy, 64..69 light -> chunk 0
    generic, chunk 1 fast: the tile must be base + 0.0f again between the two. Segment 7 the same with ONE heavy
    client per unit (64 in unit 0, 15 in unit 1). The rest goes to each segment's last full unit (all heavy)."""
    def counts(c, t, lens, k):
        light = (c * 7 + t) % 65
        if t == S8:
            a = 70 if c == 64 else light
            b = 65 + c % 7 if c in HEAVY_J else (c * 3) % 65
            return pour(lens, k, [a, b, None])
        if t == S7:
            a = 80 if c == 64 else light
            b = 90 if c == 15 else (c * 5) % 65
            return pour(lens, k, [a, b, None, c % 2])
        if t == S6:
            return pour(lens, k, [light, None])
        return even(lens, k)
    return build(bits, 70, seed, counts=counts, base=base)


def threshold(bits, base, seed=2):
    """3 clients, exactly 64 and exactly 65 entries in a unit: (64, 64, 64) all fast; (64, 65, 64), (65, 64, 64) and
    (64, 64, 65) one client over the threshold -> generic; lo + 64 / lo + 65 entry loops."""
    def counts(c, t, lens, k):
        if t == S8:
            return pour(lens, k, [64, 65 if c == 1 else 64, None])
        if t == S7:
            return pour(lens, k, [65 if c == 0 else 64, 65 if c == 2 else 64, None, 1])
        if t == S6:
            return pour(lens, k, [64 + (c == 2), None])
        return even(lens, k)
    return build(bits, 3, seed, counts=counts, base=base)


def empty_ranges(bits, base, seed=3, ratio=RATIO):
    """5 clients. Even clients keep their whole k in the segment's first unit (later units: lo == hi == k, fetch's
    `hi > lo ? hi - 1 : lo` and min(e, kseg - 1) clamps), odd clients in its last units (earlier units: lo == hi ==
    0). At RATIO_TINY, segment 7 has k = 3 < 4 units and every other multi-unit segment units without entries."""
    def counts(c, t, lens, k):
        nu = len(lens)
        return pour(lens, k, [None] * nu, dump=range(nu) if c % 2 == 0 else reversed(range(nu)))
    return build(bits, 5, seed, ratio=ratio, counts=counts, base=base)


def empty_ranges_tiny(bits, base, seed=4):
    return empty_ranges(bits, base, seed, ratio=RATIO_TINY)


def half_edges(bits, base, seed=5, ratio=RATIO):
    """4 clients; which wave of a unit owns an entry. Segment 6, unit 1 (len 2049: the second wave owns one
    element): entries only at 0, 2047, 2048 = len - 1. Segment 8: unit 0 upper half only, unit 1 only at 0, 2047,
    2048, 4095, unit 2 (len 2051) upper half only (3 entries at most) — the rest lower half. Segment 7: unit 0 upper
    half only, unit 1 lower half only, unit 3 (len 1) its one element for odd clients. Segment 4 (one full unit):
    upper half only. At RATIO_TINY (k = 1 per single-unit segment) client c's one entry sits at the c-th of 0, 2047,
    2048, len - 1."""
    tiny = ratio == RATIO_TINY

    def counts(c, t, lens, k):
        if tiny:
            return pour(lens, k, [None] * len(lens), dump=np.roll(range(len(lens)), -c))
        if t == S6:
            return pour(lens, k, [None, 3])
        if t == S8:
            return pour(lens, k, [None, 4, 3])
        if t == S7:
            return pour(lens, k, [150, None, 0, c % 2])
        return even(lens, k)

    def style(c, t, u):
        if tiny or (t, u) in ((S6, 1), (S8, 1)):
            return "edges"
        if (t, u) == (S7, 1):
            return "lower"
        return "upper"
    return build(bits, 4, seed, ratio=ratio, counts=counts, style=style, base=base)


def half_edges_tiny(bits, base, seed=6):
    return half_edges(bits, base, seed, ratio=RATIO_TINY)


def same_positions(bits, base, seed=7):
    """37 clients keeping the same positions in every unit (every client's put-back hits the same tile slots)."""
    return build(bits, 37, seed, same=True, base=base)


def disjoint_positions(bits, base, seed=8):
    """37 clients, client c keeping only positions c mod 37 (no two clients share a slot) wherever a unit has room."""
    return build(bits, 37, seed, style=lambda c, t, u: "disjoint", base=base)


def mask_passthrough(bits, base, seed=9):
    """70 clients, avg_mask False on segments 1, 4, 6 and 8 (client 0's value passes through, nclients = 1: only
    client 0 decides the path). Segment 6: client 0 heavy in unit 0 (others light) and light in unit 1 (others
    heavy). Segment 8 the reverse in unit 0 / unit 1. Segment 7 is averaged with the same counts as segment 8."""
    def counts(c, t, lens, k):
        if t == S6:
            return pour(lens, k, [100 if c == 0 else 30, None])
        if t in (S7, S8):
            return pour(lens, k, [20 if c == 0 else 70, 80 if c == 0 else 10] + [None] * (len(lens) - 2), dump=[2])
        return even(lens, k)
    mask = [True, False, True, True, False, True, False, True, False]
    return build(bits, 70, seed, counts=counts, base=base, mask=mask)


def odd_base_half(bits, base, seed=10):
    """5 clients, a base with -0.0 / NaN in ONE 2048-element half of a unit: that wave is odd (generic path, base
    from global memory), its sibling wave takes the fast path. Segment 8 unit 0 (all clients light): -0.0 and NaN in
    the lower half. Segment 7 unit 1 (all light): NaN and -0.0 in the upper half. Segment 6 unit 0 (client 1 heavy,
    the others light): -0.0 in the lower half. Segment 4 (single unit, every client heavy): NaN in the upper half.
    Odd values sit both under kept entries and where nothing is kept."""
    def counts(c, t, lens, k):
        if t == S8:
            return pour(lens, k, [10 + c, None, None], dump=[1, 2])
        if t == S7:
            return pour(lens, k, [None, 20 + c, None, 0], dump=[0, 2])
        if t == S6:
            return pour(lens, k, [100 if c == 1 else 40, None])
        return even(lens, k)
    p = build(bits, 5, seed, counts=counts, base=True, weights=[0, 3, 5, 1, 2])
    off = p.table.offsets
    K = p.table.total_k_per_client

    def kept(t, c, lo, hi):  # a position of segment t kept by client c in [lo, hi)
        oo = c * K + p.table.out_offsets[t]
        i = p.idx[oo:oo + p.table.ks[t]]
        return int(i[(i >= lo) & (i < hi)][0])
    b = p.base
    b[off[S8] + kept(S8, 0, 0, 2048)] = F32(-0.0)
    b[off[S8] + kept(S8, 1, 0, 2048)] = F32(np.nan)
    b[off[S8] + 5:off[S8] + 2048:331] = F32(-0.0)
    b[off[S7] + UNIT + 2048 + 7] = F32(np.nan)
    b[off[S7] + UNIT + 2048:off[S7] + 2 * UNIT:257] = F32(-0.0)
    b[off[S6] + kept(S6, 1, 0, 2048)] = F32(-0.0)
    b[off[S6] + 1000] = F32(-0.0)
    b[off[4] + 3000] = F32(np.nan)
    return p


SPECIAL_RANGES = [(np.inf, 1.0), (-np.inf, 1.0), (0.0, np.inf), (0.0, -np.inf), (np.nan, 1.0), (1.0, np.nan),
                  (-0.0, 0.0), (-0.0, -0.0), (1e-40, 1e-42), (-1e-39, 3e-45), (0.25, 0.0), (3e38, 3e36)]
SPECIAL_WEIGHTS = [3, 0, -2, 9, 1, 7, 0, 5, 2, 11, 1e-3, 1e6]


def special_ranges(bits, base, seed=11):
    """12 clients whose segments carry mn / scale of +-Inf, NaN, -0.0, denormals (1e-40 / 1e-42: the product
    q * scale and the sum stay denormal) and scale = 0, rotated over the segments so every unit body meets every
    range; weights with 0, a negative, a fraction and 1e6 (the 3e38 range overflows to Inf under it). All determinate: compared NaN for NaN."""
    p = build(bits, len(SPECIAL_RANGES), seed, base=base, weights=SPECIAL_WEIGHTS)
    if bits != 32:
        T = len(p.table.sizes)
        for c in range(p.clients):
            for t in range(T):
                p.mn[c * T + t], p.scale[c * T + t] = SPECIAL_RANGES[(c + t) % len(SPECIAL_RANGES)]
    return p


STRUCTURE = {f.__name__: f for f in (mixed, threshold, empty_ranges, empty_ranges_tiny, half_edges, half_edges_tiny,
                                     same_positions, disjoint_positions, mask_passthrough, odd_base_half,
                                     special_ranges)}
ALL_BITS_CASE = "mixed"  # the one structure case run across bits 1 / 5 / 8 / 32 and all three modes


# ------------------------------------------------------------------------------------------------------------------
# corrupt uploads whose result the model defines (no range applies a position twice)
# ------------------------------------------------------------------------------------------------------------------
def _valid(bits, clients, base, seed):
    """The valid upload the corruptions start from: light and heavy units, units without entries."""
    def counts(c, t, lens, k):
        if t == S8:
            return pour(lens, k, [(c * 11) % 90, None, (c * 5) % 40])
        if t == S7:
            return pour(lens, k, [None, 0 if c % 3 == 0 else 70, (c * 13) % 80, c % 2])
        return even(lens, k)
    return build(bits, clients, seed, counts=counts, base=base)


def _seg_of_unit(table):
    return np.repeat(np.arange(len(table.sizes)), [units_of(n) for n in table.sizes])


def _entry_segment(table):
    return np.tile(np.repeat(np.arange(len(table.sizes)), table.ks), table.clients)


def starts_plus1(p, rng):
    return replace(p, ustart=p.ustart + 1)


def starts_random(p, rng):
    k = np.tile(np.asarray(p.table.ks)[_seg_of_unit(p.table)], p.clients)
    return replace(p, ustart=rng.integers(0, k + 1).astype(np.int32))


def starts_garbage(p, rng):
    """Random int32 garbage of every magnitude: 32 random bits shifted right by 0..31, so small in-range values,
    values far past k and negative ones (top bit set) all occur."""
    g = rng.integers(0, 1 << 32, p.ustart.size, dtype=np.uint64) >> rng.integers(0, 32, p.ustart.size).astype(np.uint64)
    return replace(p, ustart=g.astype(np.uint32).view(np.int32))


def starts_ones(p, rng):
    return replace(p, ustart=np.full_like(p.ustart, -1))  # 0xFFFFFFFF


def _half(p, rng):
    return rng.random(p.idx.size) < 0.5


def idx_neighbour(p, rng):
    """Half the entries moved one unit up or down (correct starts): they stay in their unit's range but point into
    the neighbouring unit (or before the segment: a wrapped position), where the bounds test drops them."""
    h = _half(p, rng)
    shift = np.where(rng.random(p.idx.size) < 0.5, UNIT, -UNIT)
    return replace(p, idx=np.where(h, p.idx.astype(np.int64) + shift, p.idx).astype(np.int32))


def idx_topbit(p, rng):
    h = _half(p, rng)
    return replace(p, idx=np.where(h, p.idx.view(np.uint32) | np.uint32(0x80000000), p.idx.view(np.uint32)).view(np.int32))


def idx_ge_n(p, rng):
    h = _half(p, rng)
    n = np.asarray(p.table.sizes, np.int64)[_entry_segment(p.table)]
    return replace(p, idx=np.where(h, n + rng.integers(0, 5000, p.idx.size), p.idx).astype(np.int32))


CORRUPTIONS = {f.__name__: f for f in (starts_plus1, starts_random, starts_garbage, starts_ones, idx_neighbour,
                                       idx_topbit, idx_ge_n)}
# every (kind, clients, bits, base) the GPU file runs; the seed of a case follows from it (corrupt())
CORRUPT_CASES = [(kind, C, bits, base) for kind in CORRUPTIONS for C in (3, 70) for bits in (8, 32)
                 for base in (True, False)]
# starts of all 0xFFFFFFFF clamp every range to [k, k): such an upload applies no entry at all, by construction
APPLIES_NOTHING = ("starts_ones",)


def corrupt(kind, clients, bits, base):
    seed = 100 + list(CORRUPTIONS).index(kind)
    p = _valid(bits, clients, base, seed)
    return CORRUPTIONS[kind](p, np.random.default_rng([seed, clients, bits]))


# ------------------------------------------------------------------------------------------------------------------
# racy corrupt uploads (duplicate positions inside a range): one client, weight 1, mn 1, scale 0.5, bits 8
# ------------------------------------------------------------------------------------------------------------------
RACY = ("zero_idx", "reversed_idx")


def racy(kind, base, seed=200):
    p = _valid(8, 1, base, seed)
    t = p.table
    if kind == "zero_idx":
        idx = np.zeros_like(p.idx)
    else:
        idx = np.concatenate([p.idx[oo:oo + k][::-1] for oo, k in zip(t.out_offsets, t.ks)])
    return replace(p, idx=idx, mn=np.full_like(p.mn, 1.0), scale=np.full_like(p.scale, 0.5), weights=[1])
