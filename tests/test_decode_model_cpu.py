"""The hand-built decode payloads (tests/decode_inputs.py) and the start-honouring decode model
(tests/aggregate_model.decode), without a GPU: the model equals the oracle on every valid payload the GPU file runs, no
payload is racy, every corrupt payload is non-vacuous, every claim a case makes (the unit with exactly 64 / 65 / 128 /
129 / 512 / 513 entries, the twins' slots, the passes, len % 4, the plan class) holds on the finished payload, and the
GPU file's parameter list reaches all 16 variants of k_decode_lds."""
import itertools

import numpy as np
import pytest

from coala_amd.compression.spec import LATENCY_PLAN_UNITS, UNIT, units_of
from oracle import codec_oracle as O
from tests import aggregate_inputs as I
from tests import aggregate_model as M
from tests import decode_inputs as D
from tests import ef_model as EF
from tests.aggregate_inputs import S6, S7, S8
from tests.decode_inputs import S4, S5

F32 = np.float32


def same_bits(a, b):
    nan = np.isnan(b)
    np.testing.assert_array_equal(np.isnan(a), nan)
    np.testing.assert_array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def sorted_idx(p):
    """The payload's idx with every segment's entries ascending (what an encoder writes)."""
    t = p.table
    return np.concatenate([np.sort(p.idx[oo:oo + k]) for oo, k in zip(t.out_offsets, t.ks)])


def counts_of(p, t, copy=0):
    """Per-unit entry counts of segment t of one copy of the sizes."""
    s = D.copy_of(p.table, t)[copy]
    g = I.unit_begin(p.table)[s]
    return I.unit_counts(p)[0, g:g + units_of(p.table.sizes[s])].tolist()


_filler_checked = set()


@pytest.mark.parametrize("name,ratio,batch,bits,base", D.VALID_CASES)
def test_model_equals_oracle_on_valid_payloads(name, ratio, batch, bits, base):
    """Every valid payload of the GPU file: the expected buffer the GPU file compares with (decode_inputs.
    expected_decode, the model unit by unit) equals oracle.codec_oracle.decode bit for bit, NaN for NaN, inside the
    segments and holds the sentinel everywhere else; the starts are the oracle's; every entry is applied, none
    dropped; nothing is racy (RacyPayload would propagate)."""
    p = D.valid(name, ratio, batch, bits, base)
    t = p.table
    np.testing.assert_array_equal(p.ustart, O.unit_starts(sorted_idx(p), p.segs))
    out, counts = D.expected_decode(p)
    assert out.size == t.span_per_client + I.PAD
    assert (counts.applied, counts.dropped) == (t.total_k, 0)
    end = 0
    for s, (off, n, k, oo) in enumerate(p.segs):
        assert np.all(out[end:off] == I.SENTINEL)  # the pad before the segment
        end = off + n
        if n == D.FILLER and p.filler_key in _filler_checked:
            continue  # (the cached filler elements of this (ratio, bits, base): compared when first met)
        b = None if p.base is None else p.base[off:off + n]
        same_bits(out[off:end], O.decode_segment(p.idx[oo:oo + k], p.vals[oo:oo + k], p.mn[s], p.scale[s], int(n), bits, b))
        if n == D.FILLER:
            _filler_checked.add(p.filler_key)
    assert np.all(out[end:] == I.SENTINEL) and out.size - end >= I.PAD
    assert D.is_batch(t) == batch and D.is_high_ratio(t) == (ratio in (D.RATIO_EDGE, D.RATIO_HIGH))


def test_filler_shortcut_is_the_full_model():
    """expected_decode reuses the filler segment's elements across the valid batch payloads of one (ratio, bits,
    base): the same buffer and counts as the model run over every segment."""
    for name, ratio, bits, base in (("seams", D.RATIO_LOW, 8, True), ("last_element", D.RATIO_HIGH, 32, False)):
        p = D.valid(name, ratio, True, bits, base)
        assert p.filler_key is not None
        out, counts = D.expected_decode(p)
        full = np.full_like(out, I.SENTINEL)
        c2 = M.decode(p.idx, p.vals, p.mn, p.scale, p.ustart, p.segs, bits, full, base=p.base)
        same_bits(out, full)
        np.testing.assert_array_equal(counts.units, c2.units)


def test_variant_table_is_complete():
    """The 16 (raw, base, high_ratio, batch) variants of k_decode_lds, each from the finished payload's own table (k / n
    of the large segments against 0.02, n_units against LATENCY_PLAN_UNITS), never from a case's label: the GPU
    file's parameter list must reach every one — with codes of widths 1, 5 and 8 on a latency and on a batch plan."""
    seen, widths = set(), set()
    tables = {}
    for name, ratio, batch, bits, base in D.VALID_CASES:
        key = (name, ratio, batch)
        if key not in tables:
            tables[key] = D.valid(name, ratio, batch, 32, True).table
        t = tables[key]
        hr = max(k / n for n, k in zip(t.sizes, t.ks) if n > 1024) > 0.02
        seen.add((bits == 32, base, hr, t.n_units > LATENCY_PLAN_UNITS))
        widths.add((bits, t.n_units > LATENCY_PLAN_UNITS))
    assert seen == set(itertools.product((False, True), repeat=4))
    assert widths >= set(itertools.product((1, 5, 8, 32), (False, True)))
    assert len(set(D.VALID_CASES)) == len(D.VALID_CASES)
    assert {c[0] for c in D.VALID_CASES} == set(D.CASES)


def test_plan_geometry():
    """The batch plan: 16 + 8194 + 16 = 8226 units, above the latency limit, n_units % 4 == 2 (idle waves in the last block of 4) and
    ceil(n_units / 4) % 8 == 1 (the XCD remap has a remainder); structured segments at both ends of the unit order.
    Ratio 0.02 is a high_ratio plan (k rounds up), 0.019 is not."""
    t = D.valid("counts_64", D.RATIO_LOW, True, 8, False).table
    assert t.n_units == D.FILLER_UNITS + 32 == 8226 > LATENCY_PLAN_UNITS and t.n_units % 4 == 2
    assert -(-t.n_units // 4) % 8 == 1
    ub = I.unit_begin(t)
    assert ub[9] == 16 and ub[10] == 16 + D.FILLER_UNITS and t.sizes[9] == D.FILLER
    assert not D.is_high_ratio(t)
    for ratio in (D.RATIO_EDGE, D.RATIO_HIGH):
        assert D.is_high_ratio(D.valid("counts_64", ratio, False, 8, False).table)
    assert not D.is_high_ratio(D.valid("empty_tiny", D.RATIO_TINY, True, 8, False).table)
    assert D.valid("counts_64", D.RATIO_HIGH, False, 8, False).table.ks[S7:] == [1229, 1025]
    t = D.valid("last_element", D.RATIO_LOW, True, 8, False).table  # (three more units per copy: a batch plan with
    assert D.is_batch(t) and -(-t.n_units // 4) % 8 != 0             # an XCD remainder too)


@pytest.mark.parametrize("batch", [False, True])
def test_count_cases_have_the_counts_they_claim(batch):
    """Per-unit counts read back from the finished payloads' starts (both copies of the segments in a batch plan)."""
    for copy in range(2 if batch else 1):
        for ratio in (D.RATIO_LOW, D.RATIO_EDGE, D.RATIO_HIGH):
            if batch and ratio == D.RATIO_EDGE:
                continue
            p = D.valid("counts_64", ratio, batch, 8, False)
            assert counts_of(p, S6, copy)[0] == 64
            assert counts_of(p, S7, copy)[:2] == [65, 63] and counts_of(p, S7, copy)[3] == 0
            assert counts_of(p, S8, copy)[:2] == [1, 129]
            g = I.unit_begin(p.table)[D.copy_of(p.table, S7)[copy]] + 3
            assert p.ustart[g] == p.table.ks[S7]  # the empty last unit: lo == hi == k
        for ratio in D.BOTH:
            p = D.valid("counts_128", ratio, batch, 8, False)
            assert counts_of(p, S6, copy)[0] == 0
            assert counts_of(p, S7, copy)[:2] == [127, 0] and counts_of(p, S7, copy)[3] == 1
            assert counts_of(p, S8, copy)[0] == 128 and counts_of(p, S8, copy)[2] == 0
            g = I.unit_begin(p.table)[D.copy_of(p.table, S8)[copy]] + 2
            assert p.ustart[g] == p.table.ks[S8]
        p = D.valid("counts_512", D.RATIO_HIGH, batch, 8, False)
        assert counts_of(p, S6, copy) == [576, 39]
        assert counts_of(p, S7, copy) == [512, 511, 205, 1]
        assert counts_of(p, S8, copy) == [513, 512, 0]
        p = D.valid("empty_tiny", D.RATIO_TINY, batch, 8, False)
        assert p.table.ks[S7] == 3 < units_of(p.table.sizes[S7])
        assert counts_of(p, S7, copy) == [0, 0, 2, 1] and counts_of(p, S8, copy) == [3, 0, 0]
        p = D.valid("permuted_within_unit", D.RATIO_LOW, batch, 8, False)
        assert counts_of(p, S7, copy)[:2] == [65, 63]
    if not batch:
        for ratio in D.BOTH:
            p = D.valid("full_unit", ratio, False, 8, False)
            c = counts_of(p, 9)
            assert c[0] == UNIT and c[-1] == 1 and p.table.sizes[9] % UNIT == 1
            np.testing.assert_array_equal(D.unit_positions(p, 9, 0), np.arange(UNIT))
    else:
        for ratio in D.BOTH:  # every batch payload: a filler unit with every position kept, one with none, and
            p = D.valid("seams", ratio, True, 8, False)  # filler counts on both sides of the register-chunk seam
            c = np.asarray(counts_of(p, 9))
            assert c[D.FILLER_FULL] == UNIT and c[D.FILLER_EMPTY] == 0
            seam = 512 if ratio == D.RATIO_HIGH else 64
            assert (c <= seam).sum() > 500 and (c > seam).sum() > 500
            np.testing.assert_array_equal(D.unit_positions(p, 9, D.FILLER_FULL), np.arange(UNIT))
        c = np.asarray(counts_of(D.valid("empty_tiny", D.RATIO_TINY, True, 8, False), 9))
        assert c.max() == 1 and (c == 0).sum() > 1000  # k below the unit count


@pytest.mark.parametrize("batch", [False, True])
@pytest.mark.parametrize("ratio", D.BOTH)
def test_position_cases_have_the_positions_they_claim(ratio, batch):
    full = [(S4, 0), (S5, 0), (S6, 0), (S7, 0), (S7, 1), (S7, 2), (S8, 0), (S8, 1)]  # the units of 4096 elements
    for copy in range(2 if batch else 1):
        seg = lambda p, t: D.copy_of(p.table, t)[copy]  # noqa: E731
        p = D.valid("seams", ratio, batch, 8, False)
        for t, u in full:
            assert {0, 1023, 1024, 2047, 2048, 3071, 3072, 4095} <= set(D.unit_positions(p, seg(p, t), u))
        assert {0, 1023, 1024, 2047, 2048} <= set(D.unit_positions(p, seg(p, S6), 1))  # len 2049
        assert {0, 1023, 1024, 2047, 2048, 2050} <= set(D.unit_positions(p, seg(p, S8), 2))  # len 2051
        assert set(D.unit_positions(p, seg(p, 1), 0)) >= {0, 299}

        p = D.valid("slot_twins", ratio, batch, 8, False)
        for t, u in full:  # kept only below 1024: no position p + 1024 m (m >= 1) is kept
            pos = D.unit_positions(p, seg(p, t), u)
            assert pos.size and pos.max() < D.TILE
        p = D.valid("slot_twins_inverse", ratio, batch, 8, False)
        for t, u in full:  # kept only in the last 1024: no earlier twin of a kept slot is kept
            pos = D.unit_positions(p, seg(p, t), u)
            assert pos.size and pos.min() >= 3 * D.TILE
        p = D.valid("one_pass_only", ratio, batch, 8, False)
        passes = set()
        for t, u in full:
            q = set(D.unit_positions(p, seg(p, t), u) // D.TILE)
            assert q == {(t + u) % 4}
            passes |= q
        assert passes == {0, 1, 2, 3}

        p = D.valid("last_element", ratio, batch, 8, False)
        mods = set()
        for t, n in enumerate(D.LAST_SIZES):
            u = units_of(n) - 1
            L = n - u * UNIT
            if L % 4:
                assert L - 1 in set(D.unit_positions(p, seg(p, t), u)), (t, n)
                mods.add(L % 4)
        assert mods == {1, 2, 3}

        p = D.valid("permuted_within_unit", ratio, batch, 8, False)
        q = D.valid("counts_64", ratio, batch, 8, False)
        unsorted = 0
        for t, u in full + [(S6, 1), (S8, 2)]:
            a = D.unit_positions(p, seg(p, t), u)
            assert np.unique(a).size == a.size and (a.size == 0 or (a.min() >= 0 and a.max() < UNIT))
            unsorted += int(a.size > 1 and np.any(np.diff(a) < 0))
        assert unsorted >= 8
        np.testing.assert_array_equal(p.ustart, O.unit_starts(sorted_idx(p), p.segs))
        assert not np.array_equal(p.idx, sorted_idx(p))
    if batch:  # (the filler's units are shuffled too)
        a = D.unit_positions(p, 9, 100)
        assert np.any(np.diff(a) < 0) and np.unique(a).size == a.size


def test_special_value_cases_hold_their_values():
    """mn / scale: all of SPECIAL_RANGES over the two latency cases, and over one batch case; raw values and bases:
    -0.0, NaN, +-Inf and denormals, the bases both under kept entries and at positions that are not kept."""
    def classes(v):
        v = np.asarray(v, F32)
        tiny = np.finfo(F32).tiny
        return {"-0": bool(np.any(v.view(np.uint32) == 0x80000000)), "nan": bool(np.isnan(v).any()),
                "+inf": bool(np.any(v == np.inf)), "-inf": bool(np.any(v == -np.inf)),
                "denormal": bool(np.any((np.abs(v) > 0) & (np.abs(v) < tiny)))}
    want = [(F32(a), F32(b)) for a, b in I.SPECIAL_RANGES]
    key = lambda a, b: (np.asarray(a, F32).view(np.uint32).item(), np.asarray(b, F32).view(np.uint32).item())  # noqa: E731
    got = set()
    for name, ratio in (("special_values_a", D.RATIO_LOW), ("special_values_b", D.RATIO_LOW)):
        p = D.valid(name, ratio, False, 8, False)
        got |= {key(a, b) for a, b in zip(p.mn, p.scale)}
    assert got == {key(a, b) for a, b in want}
    p = D.valid("special_values_a", D.RATIO_HIGH, True, 8, True)
    assert {key(a, b) for a, b in zip(p.mn, p.scale)} >= {key(a, b) for a, b in want}
    for batch in (False, True):
        p = D.valid("special_values_a", D.RATIO_LOW, batch, 32, False)
        assert all(classes(p.vals).values())
        p = D.valid("special_base", D.RATIO_HIGH, batch, 8, True)
        kept = np.zeros(p.base.size, bool)
        for s in D.structured(p.table):
            oo, k = p.table.out_offsets[s], p.table.ks[s]
            kept[p.table.offsets[s] + p.idx[oo:oo + k].astype(np.int64)] = True
        free = D.inside(p.table, p.base.size) & ~kept
        assert all(classes(p.base[kept]).values()) and all(classes(p.base[free]).values())
        out, _ = D.expected_decode(p)  # base + 0.0f: a -0.0 base that is not kept comes out as +0.0
        neg0 = free & (p.base.view(np.uint32) == 0x80000000)
        assert neg0.any() and np.all(out[:p.base.size][neg0].view(np.uint32) == 0)


@pytest.mark.parametrize("kind,ratio,bits,base", D.CORRUPT_CASES)
def test_corrupt_payloads_are_race_free_and_not_vacuous(kind, ratio, bits, base):
    """Every corrupt batch payload of the GPU file: the model defines its result (RacyPayload would propagate), the
    pads keep the sentinel, something is applied (except where the starts clamp every range to [k, k)), something is
    dropped or left out, and the result differs from the valid original's."""
    p = D.corrupt(kind, ratio, bits, base)
    assert D.is_batch(p.table) and p.filler_key is None
    out, counts = D.expected_decode(p)
    assert np.all(out[~D.inside(p.table, out.size)] == I.SENTINEL)
    orig, _ = D.expected_decode(D.valid(D.CORRUPT_ORIGINAL, ratio, True, bits, base))
    assert not np.array_equal(out.view(np.uint32), orig.view(np.uint32))
    if kind in D.APPLIES_NOTHING:
        assert (counts.applied, counts.dropped) == (0, 0)
        return
    assert 0 < counts.applied < p.table.total_k
    if kind == "pos_ge_len":  # the moved entries, and nothing else, are dropped: all in partial last units
        t = p.table
        lastpart = [I.unit_begin(t)[s] + units_of(n) - 1 for s, n in enumerate(t.sizes) if n % UNIT]
        assert counts.dropped == counts.units[lastpart, 1].sum() == t.total_k - counts.applied
        assert (counts.units[lastpart, 1] > 0).sum() >= 12


def test_commit_model_changes_every_payload():
    """ef_model.commit of the valid payloads the GPU file commits: defined (finite) and not the identity."""
    for name, c in D.CASES.items():
        if not c.commit:
            continue
        p = D.valid(name, c.ratios[0], False, 8, c.base_only)
        a = D.residual(p.table)
        r = EF.commit(a, p.idx, p.vals, p.mn, p.scale, p.segs, p.bits)
        ins = D.inside(p.table, a.size)
        assert np.all(r[~ins] == I.SENTINEL) and (r != a).sum() > 0 and np.isfinite(r).all()
