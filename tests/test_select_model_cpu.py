"""The hand-built select cases (tests/select_inputs.py) against the route model (tests/select_model.py), without a GPU:
every case takes the route it claims with the counts it claims, its bracket is the one computed before the edits, the
boundary cases keep their entries beyond the boundary, and the cases cover every route in both plan classes."""
import re

import numpy as np
import pytest

from tests import select_inputs as I
from tests import select_model as M
from tests.sampler_model import KEY_MAX, bracket

NAMES = list(I.BUILDERS)


def modelled(name, rmax, flags=0):
    c = I.case(name)
    return c, M.route_of(c.x, c.k, c.row, I.CCAP[rmax], flags)


def rmaxes(c):
    return [r for r in I.RMAX if c.min_rmax <= r and c.only_rmax in (None, r)]


@pytest.mark.parametrize("name", NAMES)
def test_case_takes_the_route_it_claims(name):
    c = I.case(name)
    assert c.nu == I.BUILDERS[name][0] and c.x.size % 4 in (1, 2, 3) and 1 <= c.k <= c.x.size
    assert rmaxes(c)
    for rmax in rmaxes(c):
        assert c.k / c.x.size <= rmax
        _, R = modelled(name, rmax)
        assert R.route == c.route, (R.route, c.route, R.sa, R.sc, R.sz, c.k)
        assert M.agrees_with_sampler_model(c.x, c.k, R, I.CCAP[rmax])
        assert (R.tlo, R.thi, R.outcome) == c.bracket0  # the edits did not move the bracket
        assert R.shhi == min(R.thi, int((c.x.view(np.uint32)[M.sample_positions(c.x.size, c.row)] & KEY_MAX).max()))
        for key, want in c.counts.items():
            if key == "kth_key":
                keys = np.sort(c.x.view(np.uint32) & np.uint32(KEY_MAX))[::-1]
                assert int(keys[c.k - 1]) == want
                if R.wlo is not None:
                    assert R.wlo <= want <= R.whi
            elif key == "cntC_last":
                assert int(R.cntC[-1]) == want and int(R.cntC[:-1].max()) <= I.ROOM + 16
            elif key == "gcnt":
                np.testing.assert_array_equal(R.gcnt, want)
            else:
                assert getattr(R, key) == want, (key, getattr(R, key), want)
        if c.only_rmax is None:
            assert int(R.cntC.max()) <= I.CCAP[0.01]  # every unit within every plan's ccap
        if R.hist is not None:  # segment_pick's histogram holds exactly the candidates below T_hi
            assert int(R.hist.sum()) == R.sc - R.sa


@pytest.mark.parametrize("name", NAMES)
def test_bracket_does_not_depend_on_the_edits(name):
    """The bracket of the finished segment equals the skeleton's, and rewriting every unsampled position once more
    (all zeros there) leaves it where it is: it is a function of the sampled positions alone."""
    c = I.case(name)
    assert bracket(c.x, c.k, c.row) == c.bracket0
    y = np.zeros_like(c.x)
    sp = M.sample_positions(c.x.size, c.row)
    y[sp] = c.x[sp]
    assert bracket(y, c.k, c.row) == c.bracket0


BOUNDARY = [n for n in NAMES if re.fullmatch(r"(window|tie|quota|rank0)_\d+(_forced)?", n)]


@pytest.mark.parametrize("name", BOUNDARY)
def test_boundary_case_keeps_its_entries_beyond_the_boundary(name):
    """At least half of the kept entries lie in the units from the boundary on; so does every element equal to the k-th
    key that the case placed (in tie mode the sampled positions all hold K, wherever the sampler reads them: there the
    case's own ties and the end of the quota lie beyond it). generic_rank0 at 769 / 1537 units: see select_inputs."""
    c = I.case(name)
    keys = (c.x.view(np.uint32) & np.uint32(KEY_MAX)).astype(np.int64)
    order = np.argsort(-keys, kind="stable")[:c.k]
    T = int(keys[order[-1]])
    if name.startswith("tie"):  # tie mode: the records, the keys above K (the kept ties are where the sampler reads)
        order = order[keys[order] > T]
        assert order.size > 500
    b = c.boundary
    assert 2 * int((order >= b * I.UNIT).sum()) >= order.size, (b, int((order >= b * I.UNIT).sum()), order.size)
    if name.startswith("rank0") and c.nu in (33, 769, 1537, 2049):
        assert b == I.BOUNDARY_OF[c.nu - 1] and (order >= (c.nu - 1) * I.UNIT).sum() >= I.ROOM - 32
    else:
        assert b == I.BOUNDARY_OF[c.nu]
    if name.startswith("tie"):  # why no tie-mode case can do better: tie mode needs K at every position the sampler
        spos = M.sample_positions(c.x.size, c.row)  # reads, and it reads every stratum of the segment
        assert (keys[spos] == T).all()
        assert b == 0 or (spos < b * I.UNIT).sum() * c.nu >= spos.size * b // 2
    if c.ties is not None:
        sp = set(M.sample_positions(c.x.size, c.row).tolist())
        own = np.array([p for p in c.ties.tolist() if p not in sp], np.int64)
        assert own.size and (own >= b * I.UNIT).all()
        assert (keys[c.ties] == T).all() and int((keys == T).sum()) == c.ties.size
        kept_ties = c.k - int((keys > T).sum())
        assert 0 < kept_ties <= c.ties.size and c.ties[kept_ties - 1] >= b * I.UNIT  # the quota ends beyond it


def test_routes_are_covered_in_both_plan_classes():
    """Every route of select_model.ROUTES is claimed by a case (raw_forced and one generic_forced are flags on a case:
    tests/test_gpu_select_structure.py runs them), in every part's latency-bound and batch plan alike (the two hold the
    same rows)."""
    claimed = {I.case(n).route for n in NAMES}
    assert claimed == set(M.ROUTES) - {"raw_forced"}
    c, R = modelled("window_first_in_list", 0.01, flags=M.FLAG_FORCE_EXACT)
    assert R.route == "raw_forced" and M.agrees_with_sampler_model(c.x, c.k, R, I.CCAP[0.01], M.FLAG_FORCE_EXACT)
    c, R = modelled("window_first_in_list", 0.01, flags=M.FLAG_GENERIC_SELECT)
    assert R.route == "generic_forced"
    c, R = modelled("tie_K_sc+1", 0.01, flags=M.FLAG_GENERIC_SELECT)
    assert R.route == "raw_miss_low"  # the shortcut is skipped, and select_fallback finds k > sc
    for part, names in enumerate(I.PARTS):
        assert sum(I.BUILDERS[n][0] for n in names) + I.PIN_UNITS <= 8192  # a latency-bound plan
        assert sum(I.BUILDERS[n][0] for n in names) + I.PIN_UNITS + I.FILLER_UNITS > 8192  # a batch plan


def test_histogram_tail_changes_the_window():
    """segment_pick sums the first GB = 24 group histograms in one round and the others in rounds of 8, the last one
    masked. window_hist_tail_1500 (47 groups) is built so that leaving groups out moves the pick: with the first 24
    groups only, or with the last group missing, the histogram still holds k - sa keys and the rank lands in a LOWER
    bin. The window route would then resolve a smaller k-th key — more than k keys lie above it, so idx, the codes and
    the per-unit starts of the case and of the small segment after it all change (tests/test_gpu_select_structure.py
    compares them whole). The other window cases above 768 units cannot show this: their head groups hold fewer than
    k - sa band keys, hist_pick finds no bin and the (exact) generic select runs."""
    c, R = modelled("window_hist_tail_1500", 0.01)
    ng = (c.nu + M.GU - 1) // M.GU
    assert R.route == "window" and ng == 47 and (ng - 24) % 8 != 0
    np.testing.assert_array_equal(M.band_hist(c.x, R), R.hist)
    r = c.k - R.sa
    for groups in (range(24), range(ng - 1), range(32), [g for g in range(ng) if g != 24]):
        b, rank = M.hist_pick(M.band_hist(c.x, R, groups), r)
        assert b is not None and b < R.bin, (list(groups)[-1], b, R.bin)
        keys = (c.x.view(np.uint32) & np.uint32(KEY_MAX)).astype(np.int64)
        assert int((keys > R.band.whi(b)).sum()) > c.k  # every key of the wrong window lies below the true k-th key
    for name in NAMES:  # the others: silent under the same mutation, as said
        o = I.case(name)
        if name != c.name and o.route == "window" and o.nu > 24 * M.GU:
            Ro = M.route_of(o.x, o.k, o.row, I.CCAP[0.01])
            assert M.hist_pick(M.band_hist(o.x, Ro, range(24)), o.k - Ro.sa)[0] is None


def test_sizes_straddle_the_loop_boundaries():
    """The size classes against the block sizes of each plan class: 768 | 769 units straddle CB * NT of the batch plans'
    256-thread blocks and the 24 group histograms, 1536 | 1537 CB * NT of the latency-bound plans' 512-thread blocks,
    32 | 33 one group, 2048 | 2049 UCAP; every boundary of either class lies at or below a size class."""
    assert M.loop_boundaries("batch") == [32, 256, 768, 2048]
    assert M.loop_boundaries("latency") == [32, 512, 768, 1536, 2048]
    for pc in ("latency", "batch"):
        for b in M.loop_boundaries(pc):
            if b in (256, 512):  # select_finish / zero_tie_ranks chunks: crossed by every size from 768 on
                assert any(nu > b for nu in I.BOUNDARY_SIZES)
            else:
                assert b in I.BOUNDARY_SIZES and b + 1 in I.BOUNDARY_SIZES


def test_sign_cases_hinge_on_one_tie():
    """The sign cases: every kept value above the k-th key has one sign, and the first tie of the other sign sits at tie
    rank rt - 1 (kept) or rt (dropped) — the only arrangement in which mn / scale depend on `fp_rank < rt`, `fn_rank <
    rt`. The tie-mode pair's tie lies beyond unit 512, so zero_tie_ranks carries its scan across chunks."""
    for prefix, other_neg in (("tie_sign", True), ("window_sign", False)):
        for s in ("kept", "dropped"):
            c = I.case(f"{prefix}_{s}")
            bits = c.x.view(np.uint32)
            keys = (bits & np.uint32(KEY_MAX)).astype(np.int64)
            neg = (bits >> 31).astype(bool)
            T = int(np.sort(keys)[::-1][c.k - 1])
            rt = c.k - int((keys > T).sum())
            assert (neg[keys > T] != other_neg).all()
            tn = neg[c.ties]
            first = int(np.flatnonzero(tn == other_neg)[0])
            assert first == (rt - 1 if s == "kept" else rt), (first, rt)
            if prefix == "tie_sign":
                assert c.ties[first] // I.UNIT >= 512


def test_limits_of_the_sampler():
    """What decides which case exists where (select_inputs' docstring): T_hi closes only from a ratio on."""
    for nu in (32, 33, 40):
        assert not I.closed_thi(nu, int(0.01 * I.n_of(nu))) and I.closed_thi(nu, int(0.03 * I.n_of(nu)))
    for nu in (768, 769, 1536, 1537, 2048, 2049):
        assert I.closed_thi(nu, int(0.0099 * I.n_of(nu))) and not I.closed_thi(nu, 2 * I.ROOM)
    for name in NAMES:  # ... and the cases agree with that formula
        c = I.case(name)
        if not (c.bracket0[0] == 0 or c.bracket0[0] & 0x80000000):
            assert (c.bracket0[1] != KEY_MAX) == I.closed_thi(c.nu, c.k), name


def test_hist_pick_cannot_miss():
    """segment_pick returns the generic route when hist_pick finds no bin (NONE). With sa < k <= sc and no unit over ccap
    that cannot happen: the histogram holds every candidate with key <= T_hi, sc - sa of them, and the rank asked for is
    k - sa <= sc - sa. Pinned here rather than built: no consistent counts reach it."""
    for name in NAMES:
        c = I.case(name)
        for rmax in rmaxes(c):
            R = M.route_of(c.x, c.k, c.row, I.CCAP[rmax])
            if R.hist is not None:
                assert 1 <= c.k - R.sa <= int(R.hist.sum())
