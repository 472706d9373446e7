"""The start-honouring model of the fused sparse aggregate (tests/aggregate_model.py) and the hand-built uploads
(tests/aggregate_inputs.py), without a GPU: the model equals the oracle on valid payloads, its clamp is pinned by
hand-computed cases, every structure case has the per-unit counts its docstring claims, and every corrupt upload
the GPU file runs is race-free on the model and not vacuous."""
import numpy as np
import pytest

from coala_amd.compression.spec import SegmentTable, units_of
from oracle import codec_oracle as O
from tests import aggregate_inputs as I
from tests import aggregate_model as M

F32 = np.float32
MODES = (O.AGG_RECIP, O.AGG_DIV, O.AGG_SUM)


def run_model(p, mode, mask="own"):
    out = np.full(p.table.span_per_client + I.PAD, I.SENTINEL, F32)
    counts = M.aggregate(p.idx, p.vals, p.mn, p.scale, p.ustart, p.segs, p.bits, p.clients, p.weights,
                         sum(p.weights), mode, out, base=p.base, avg_mask=p.mask if mask == "own" else mask)
    return out, counts


def same_bits(a, b):
    nan = np.isnan(b)
    np.testing.assert_array_equal(np.isnan(a), nan)
    np.testing.assert_array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def inside(table, size):
    m = np.zeros(size, bool)
    for off, n in zip(table.offsets, table.sizes):
        m[off:off + n] = True
    return m


@pytest.mark.parametrize("base", [True, False])
@pytest.mark.parametrize("bits", [1, 5, 8, 32])
@pytest.mark.parametrize("name", list(I.STRUCTURE))
def test_model_equals_oracle_on_valid_payloads(name, bits, base):
    """Correct starts: unit-by-unit decoding is whole-segment decoding, so the model must equal
    oracle.codec_oracle.aggregate bit for bit (NaN for NaN where a case puts NaN in) — and leave the sentinel in
    every pad. All three modes, without and with a mask, for the all-bits case and the mask case; recip for the rest."""
    p = I.STRUCTURE[name](bits, base)
    np.testing.assert_array_equal(p.ustart, O.unit_starts(p.idx, p.segs))
    T = len(p.table.sizes)
    masks = [p.mask] if name not in (I.ALL_BITS_CASE, "mask_passthrough") else [None, [t % 3 != 1 for t in range(T)]]
    ins = inside(p.table, p.table.span_per_client + I.PAD)
    for mode in MODES if len(masks) > 1 else MODES[:1]:
        for mask in masks:
            out, counts = run_model(p, mode, mask)
            ref = O.aggregate(p.idx, p.vals, p.mn, p.scale, p.segs, bits, p.clients, p.weights, sum(p.weights), mode,
                              base=p.base, out_span=p.table.span_per_client, avg_mask=mask)
            same_bits(out[:ref.size][ins[:ref.size]], ref[ins[:ref.size]])
            assert np.all(out[~ins] == I.SENTINEL)
            assert (counts.applied, counts.dropped) == (p.idx.size, 0)


def test_structure_cases_have_the_counts_they_claim():
    """The per-unit entry counts each structure case was built for (light: <= 64, heavy: >= 65), read back from the
    finished payloads: what decides k_aggregate's path per unit and 64-client chunk."""
    ub = I.unit_begin(SegmentTable(I.SIZES, I.RATIO, 1))
    u6, u7, u8 = ub[I.S6], ub[I.S7], ub[I.S8]
    light, heavy = (lambda a: np.all(a <= 64)), (lambda a: np.all(a >= 65))

    n = I.unit_counts(I.mixed(8, False))
    for u in (u8, u7):  # chunk 0 fast, chunk 1 generic
        assert light(n[:64, u]) and heavy(n[64, u]) and light(n[65:, u]) and len(set(n[:64, u])) > 16
    assert heavy(n[list(I.HEAVY_J), u8 + 1]) and light(n[64:, u8 + 1])  # chunk 0 generic, chunk 1 fast
    assert light(np.delete(n[:64, u8 + 1], I.HEAVY_J))
    assert heavy(n[15, u7 + 1]) and light(np.delete(n[:, u7 + 1], 15))
    assert n[:, u6].max() <= 64 and n[:, u7 + 3].tolist() == [c % 2 for c in range(70)]

    n = I.unit_counts(I.threshold(8, False))
    assert n[:, u8].tolist() == [64, 64, 64] and n[:, u8 + 1].tolist() == [64, 65, 64]
    assert n[:, u7].tolist() == [65, 64, 64] and n[:, u7 + 1].tolist() == [64, 64, 65]
    assert n[:, u6].tolist() == [64, 64, 65] and light(n[:, u6 + 1])

    for case, ratio in ((I.empty_ranges, I.RATIO), (I.empty_ranges_tiny, I.RATIO_TINY)):
        p = case(8, False)
        n, ks = I.unit_counts(p), p.table.ks
        s = p.ustart.reshape(5, -1)
        assert np.all(n[0::2, u7] == ks[I.S7]) and np.all(n[0::2, u7 + 1:u7 + 4] == 0)  # first unit only
        assert np.all(s[0::2, u7 + 1:u7 + 4] == ks[I.S7])                               # ... lo == hi == k after it
        assert np.all(n[1::2, u7] == 0) and np.all(s[1::2, u7:u7 + 2] == 0)             # lo == hi == 0 before
        assert np.all(n[1::2, u8 + 2] == min(ks[I.S8], 2051))
    assert ks[I.S7] == 3 < units_of(I.SIZES[I.S7])  # (the tiny plan: k below the unit count)

    p = I.half_edges(8, False)
    K = p.table.total_k_per_client

    def positions(c, t, u):
        i = p.idx[c * K + p.table.out_offsets[t]:][:p.table.ks[t]].astype(np.int64)
        return i[(i >= u * 4096) & (i < (u + 1) * 4096)] - u * 4096
    for c in range(4):
        assert set(positions(c, I.S6, 1)) == {0, 2047, 2048}
        assert set(positions(c, I.S8, 1)) == {0, 2047, 2048, 4095}
        for t, u in ((I.S6, 0), (I.S8, 0), (I.S8, 2), (I.S7, 0), (4, 0)):
            assert positions(c, t, u).size and positions(c, t, u).min() >= 2048, (c, t, u)
        assert positions(c, I.S7, 1).size and positions(c, I.S7, 1).max() < 2048
    p = I.half_edges_tiny(8, False)
    K = p.table.total_k_per_client
    assert [int(p.idx[c * K + p.table.out_offsets[3]]) for c in range(4)] == [0, 2047, 2048, 0]

    p = I.same_positions(8, False)
    K = p.table.total_k_per_client
    assert all(np.array_equal(p.idx[:K], p.idx[c * K:(c + 1) * K]) for c in range(37))
    p = I.disjoint_positions(8, False)
    for t in (1, 2, 3, 4, I.S6, I.S7, I.S8):
        oo, k = p.table.out_offsets[t], p.table.ks[t]
        allpos = np.concatenate([p.idx[c * K + oo:c * K + oo + k] for c in range(37)])
        assert np.unique(allpos).size == allpos.size, t

    p = I.mask_passthrough(8, False)
    n = I.unit_counts(p)
    assert not p.mask[I.S6] and not p.mask[I.S8] and p.mask[I.S7]
    assert heavy(n[0, u6]) and light(n[1:, u6]) and light(n[0, u6 + 1]) and heavy(n[1:, u6 + 1])
    assert light(n[0, u8]) and heavy(n[1:, u8]) and heavy(n[0, u8 + 1]) and light(n[1:, u8 + 1])

    p = I.odd_base_half(8, True)
    n, off = I.unit_counts(p), p.table.offsets
    odd = np.isnan(p.base) | (p.base.view(np.uint32) == 0x80000000)
    halves = lambda t, u: [bool(odd[off[t] + u * 4096 + h * 2048:][:2048].any()) for h in (0, 1)]
    assert halves(I.S8, 0) == [True, False] and light(n[:, u8])
    assert halves(I.S7, 1) == [False, True] and light(n[:, u7 + 1])
    assert halves(I.S6, 0) == [True, False] and heavy(n[1, u6]) and light(np.delete(n[:, u6], 1))
    assert halves(4, 0) == [False, True] and heavy(n[:, ub[4]])


def _hand(sizes, ratio, clients, idx, vals, ustart, weights):
    t = SegmentTable(sizes, ratio, clients)
    z = np.zeros(len(t.segs), F32)
    out = np.full(t.span_per_client + I.PAD, I.SENTINEL, F32)
    counts = M.aggregate(np.asarray(idx, np.int32), np.asarray(vals, F32), z, z, np.asarray(ustart, np.int64), t.segs,
                         32, clients, weights, sum(weights), O.AGG_SUM, out)
    exp = np.full_like(out, I.SENTINEL)
    for off, n in zip(t.offsets, t.sizes):
        exp[off:off + n] = 0
    return t, out, exp, counts


def test_model_clamp_hand_computed():
    """The clamp, by hand. One client, sizes [5000, 10] at ratio 0.001: k = 5 (units of 4096 and 904 elements) and
    k = 1 (the plan's last unit); raw values 1..6, weight 2, mode sum, so an applied entry shows as twice its value."""
    idx, vals = [10, 20, 4096, 4100, 4999, 3], [1, 2, 3, 4, 5, 6]
    # a start above k: unit 0 is [5, 5), empty; unit 1 (its segment's last) is [2, min(5, 2 + 904)) = [2, 5)
    t, out, exp, n = _hand([5000, 10], 0.001, 1, idx, vals, [9, 2, 0], [2])
    assert t.ks == [5, 1] and t.offsets[1] == 5024
    exp[[4096, 4100, 4999, 5024 + 3]] = [6, 8, 10, 12]
    np.testing.assert_array_equal(out, exp)
    assert (n.applied, n.dropped) == (4, 0)
    # start[u + 1] < start[u]: unit 0 is [3, max(3, 1)) = [3, 3); unit 1 is [1, 5) and entry 1 (position 20 - 4096,
    # wrapped) is dropped by the bounds test
    t, out, exp2, n = _hand([5000, 10], 0.001, 1, idx, vals, [3, 1, 0], [2])
    np.testing.assert_array_equal(out, exp)
    assert (n.applied, n.dropped) == (4, 1) and n.units[0].tolist() == [[0, 0], [3, 1], [1, 0]]
    # 0xFFFFFFFF (-1 as int32): read as uint32, clamped to k
    t, out, exp, n = _hand([5000, 10], 0.001, 1, idx, vals, [-1, -1, -1], [2])
    np.testing.assert_array_equal(out, exp)
    assert (n.applied, n.dropped) == (0, 0)
    # a range longer than the unit: [4098] at ratio 0.002, k = 9, units of 4096 and 2 elements. Unit 0 is [0, 2);
    # unit 1 is [2, min(9, 2 + 2)) = [2, 4): entries 2 and 3 (positions 2 - 4096, 3 - 4096) are dropped, and the
    # unit's own entries 7 and 8 are never reached
    t, out, exp, n = _hand([4098], 0.002, 1, [0, 1, 2, 3, 4, 5, 6, 4096, 4097], [1, 2, 3, 4, 5, 6, 7, 8, 9], [0, 2], [2])
    assert t.ks == [9]
    exp[[0, 1]] = [2, 4]
    np.testing.assert_array_equal(out, exp)
    assert (n.applied, n.dropped) == (2, 2)
    # a duplicate position inside one range has no expected value
    with pytest.raises(M.RacyPayload):
        _hand([4098], 0.002, 1, [5, 5, 2, 3, 4, 5, 6, 4096, 4097], [1] * 9, [0, 7], [2])


def test_model_last_unit_of_a_client_ends_at_k():
    """Two clients of [5000]: client 0's last unit is followed in the starts by client 1's first unit (start 0). A
    segment's last unit ends at k, not at that next start; the plan's last unit reads its own start as the 'next'
    one and ends at k too. Both clients' entry 4 (position 4999) is applied: 2 * 5 + 3 * 50."""
    idx = [10, 20, 30, 40, 4999] * 2
    vals = [1, 2, 3, 4, 5, 10, 20, 30, 40, 50]
    t, out, exp, n = _hand([5000], 0.001, 2, idx, vals, [0, 4, 0, 4], [2, 3])
    exp[[10, 20, 30, 40, 4999]] = [32, 64, 96, 128, 160]
    np.testing.assert_array_equal(out, exp)
    assert (n.applied, n.dropped) == (10, 0)


@pytest.mark.parametrize("kind,clients,bits,base", I.CORRUPT_CASES)
def test_corrupt_uploads_are_race_free_and_not_vacuous(kind, clients, bits, base):
    """Every corrupt upload of the GPU file, at its parametrisation and seed: the model defines its result (no range
    applies a position twice: RacyPayload would propagate), the pads keep the sentinel, and some client's multi-unit
    segment has a unit that applies an entry and a unit that drops one — the GPU comparison can tell a kernel that
    applies too much from one that applies too little. Starts of all 0xFFFFFFFF clamp every range to [k, k) whatever
    the seed: that upload is pinned as applying nothing (the result is the weighted base alone)."""
    p = I.corrupt(kind, clients, bits, base)
    out, counts = run_model(p, O.AGG_RECIP)
    assert np.all(out[~inside(p.table, out.size)] == I.SENTINEL)
    if kind in I.APPLIES_NOTHING:
        assert (counts.applied, counts.dropped) == (0, 0)
        return
    ub = I.unit_begin(p.table)
    multi = [(ub[t], units_of(n)) for t, n in enumerate(p.table.sizes) if units_of(n) > 1]
    assert any(counts.units[c, u:u + nu, 0].any() and counts.units[c, u:u + nu, 1].any()
               for c in range(clients) for u, nu in multi)
    assert 0 < counts.applied < p.idx.size and counts.dropped > 0


@pytest.mark.parametrize("base", [True, False])
def test_racy_uploads_are_what_the_model_refuses(base):
    """All-zero indices put duplicate positions into one range: the model raises, the GPU file checks bounds and the
    value set only. Reversed indices are treated the same way there."""
    p = I.racy("zero_idx", base)
    with pytest.raises(M.RacyPayload):
        run_model(p, O.AGG_SUM)
    p = I.racy("reversed_idx", base)
    oo, k = p.table.out_offsets[I.S8], p.table.ks[I.S8]
    assert np.all(np.diff(p.idx[oo:oo + k]) < 0)
    assert p.weights == [1] and np.all(p.mn == 1.0) and np.all(p.scale == 0.5) and p.bits == 8
