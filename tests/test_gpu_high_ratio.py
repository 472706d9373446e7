"""GPU parity above ratio 0.5 and at extreme k on large segments: HIP kernels vs the CPU oracle, bit-exact (the bar of
tests/test_gpu_parity.py: idx, codes, mn, scale, the per-unit starts, and the decode both from the encoder's starts and
from host-computed ones; any difference fails).

What each test is there to reach (coalac.hip), and how it shows that it did:
  test_high_ratio_small_layout        plans with ccap = UNIT (rmax >= 0.475): thousands of records per unit, past k_scan's
                                      512 staged ones, group windows past GCAP / WLIST (select_fallback's generic select),
                                      k_emit / k_decode_lds at ~2500-4096 entries per unit. The kernel's brackets equal the
                                      sampler model's, and the raw-path count equals the model's (ccap_for = 4096).
  test_open_lower_bracket_is_reached  sample_segment with rlo >= m: T_lo = 0 (no tie flag) on data that is no frozen
                                      tensor, zero-tie mode with every nonzero element a record. Asserted: T_lo == 0.
  test_extreme_k_explicit_rows        k = 1, 2 (rhi < 1: T_hi open), n - 1, n (the k-th key is the segment's minimum, in
                                      a plan that is not dense), n // 2 + 1, ceil(n / 1000), from explicit rows.
  test_mixed_ratios_in_one_plan       per-plan switches (ccap, the high-ratio kernel variants, the decode's register
                                      chunks) taken from the largest ratio while other segments keep 0.1 %.
  test_high_ratio_batch_plan          the batch kernels (> 8192 units) at the same ratios. Asserted: n_units > 8192.
  test_decode_consumers_at_high_ratio k_aggregate and k_ef_commit at > 3000 entries per unit (asserted from the oracle's
                                      per-unit starts).

Off-by-ones these assertions catch (by reading coalac.hip, not by running a broken kernel):
  * segment_pick `k - sc <= sz` (the zero-tie shortcut, the open lower bracket's way to a k-th key of 0): with `<`,
    k = n of a segment with zeros (k - sc == sz exactly) goes to select_fallback, which finds k > sc and takes the raw
    path — test_extreme_k_explicit_rows[zeros30 / one] sees fallbacks 1 where the model says 0.
  * select_finish `quota = min(e, rt - qp)` / `so = gx + qp`: the zero quota in index order across units decides
    which zeros of zeros30 are kept at every ratio from 0.75 on, 256 units deep (idx, starts, decode).
  * k_decode_lds `hi = max(lo, min(..., lo + U.len))` (k = n in a sparse plan): a unit then holds exactly len entries;
    `lo + U.len - 1` drops each full unit's last entry (element 4095, nonzero) from both decodes.
  * k_decode_lds `for (e0 = lo + NCH * 64; ...)`: the per-pass reload of the entries past the 8 x 64 held in registers;
    starting it one chunk late loses a unit's entries 512..575 (every unit here holds > 2400).
  Not observable in any output: k_scan's CHECK form of scan_unit in zero-tie mode with K = 0. Without it the loads past
  a ragged last unit's len (key 0) would only inflate that unit's zero count, which sits after every other unit's in
  the index-order quota and can only make `k - sc <= sz` true where it already is (k <= n).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, Encoded
from coala_amd.compression._lib import COALAC_FLAG_GENERIC_SELECT
from coala_amd.compression.spec import small_limit
from oracle import codec_oracle as O
from tests import ef_model as M
from tests.ef_model import bits_of
from tests.high_ratio_inputs import (KINDS, LARGE, MIXED_RATIOS, PAD, SIZES, base_layout, explicit_rows, extreme_ks,
                                     layout, mixed_ks, segment, with_base)
from tests.sampler_model import KEY_MAX, TIE_FLAG, bracket, ccap_for, takes_raw_path
from tests.test_gpu_parity import assert_same, run_both

pytestmark = pytest.mark.gpu

F32 = np.float32


def flat_of(segs, xs):
    """The plan's flat input: segment i of xs at row i's in_off (zeros between)."""
    segs = np.asarray(segs).astype(np.int64)
    flat = np.zeros(int((segs[:, 0] + segs[:, 1]).max()), F32)
    for (off, n, _, _), x in zip(segs, xs):
        flat[off:off + n] = x
    return flat


def run_plan(plan, xs, bases=None, flags=0, brackets=False):
    """run_both of tests/test_gpu_parity.py for an already-built plan (explicit rows): the same results, keyed the same."""
    table = plan.table
    flat = flat_of(table.segs, xs)
    base = None if bases is None else flat_of(table.segs, bases)
    d_flat = torch.from_numpy(flat).cuda()
    d_base = None if base is None else torch.from_numpy(base).cuda()
    ws = plan.empty_workspace()
    enc = plan.encode(d_flat, base=d_base, workspace=ws, flags=flags, out=plan.empty_encoded(with_idx=True))
    dec = plan.decode(enc, base=d_base)
    dec_v1 = plan.decode(Encoded(enc.idx, enc.vals, enc.mn, enc.scale), base=d_base)  # no per-unit starts
    torch.cuda.synchronize()
    g = dict(idx=enc.idx.cpu().numpy(), vals=enc.vals.cpu().numpy(), mn=enc.mn.cpu().numpy(),
             scale=enc.scale.cpu().numpy(), ustart=enc.ustart.cpu().numpy(), dec=dec.cpu().numpy(),
             dec_v1=dec_v1.cpu().numpy(), fallbacks=plan.fallbacks(ws))
    if brackets:
        nl = sum((int(n) + 4095) // 4096 for n in table.segs[:, 1] if n > small_limit(table.segs[:, 1]))
        lo, hi = (ctypes.c_uint32 * max(nl, 1))(), (ctypes.c_uint32 * max(nl, 1))()
        got = plan._lib.coalac_debug_brackets(plan._h, ctypes.c_void_p(ws.data_ptr()), None, lo, hi, nl)
        assert got == nl, (got, nl)
        g["tlo"], g["thi"] = np.frombuffer(lo, np.uint32)[:nl].copy(), np.frombuffer(hi, np.uint32)[:nl].copy()
    segs = table.segs.astype(np.int64)
    idx, vals, mn, sc = O.encode(flat, segs, plan.bits, base=base)
    ref_dec = O.decode(idx, vals, mn, sc, segs, plan.bits, table.span, base=base)
    r = dict(idx=idx, vals=vals, mn=mn, scale=sc, ustart=O.unit_starts(idx, segs), dec=ref_dec)
    return plan, g, r


def check_brackets_and_raw_path(plan, g, ds, ccap, generic=False):
    """Every large segment's kernel bracket equals the sampler model's (all its units carry it), and exactly the
    segments the model sends to the raw-data path took it. ds: the fp32 values the codec sees (x, or x - base);
    generic: the encode ran with COALAC_FLAG_GENERIC_SELECT. Returns {row: (T_lo, T_hi)}."""
    segs = plan.table.segs.astype(np.int64)
    lim = small_limit(segs[:, 1])
    lu, raw, out = 0, 0, {}
    for s, (off, n, k, oo) in enumerate(segs):
        if n <= lim:
            continue
        nu = (n + 4095) // 4096
        tlo, thi, o = bracket(ds[s], int(k), s)
        got = (int(g["tlo"][lu]), int(g["thi"][lu]))
        assert got == (tlo, thi), (s, n, k, o, [hex(v) for v in got + (tlo, thi)])
        assert (g["tlo"][lu:lu + nu] == tlo).all() and (g["thi"][lu:lu + nu] == thi).all()
        raw += takes_raw_path(ds[s], int(k), tlo, thi, ccap, generic)
        out[s] = (tlo, thi)
        lu += nu
    assert g["fallbacks"] == raw, (g["fallbacks"], raw)
    return out


def inputs(kind, delta):
    """(xs, bases, the values the codec sees) of the small layout."""
    ds = layout(kind)
    if not delta:
        return ds, None, ds
    bases = base_layout()
    xs, seen = with_base(ds, bases)
    return xs, bases, seen


# -- 1. ratios 0.6 .. 0.999 on the small layout --------------------------------------------------------------------
RATIOS = (0.6, 0.75, 0.9, 0.97, 0.999)
CELLS = [(r, kind, 8, False, 0) for r in RATIOS for kind in KINDS]
CELLS += [(r, kind, b, d, 0) for r in RATIOS for kind in ("gauss", "zeros30") for b, d in ((1, False), (32, False), (8, True))]
CELLS += [(r, kind, 8, False, COALAC_FLAG_GENERIC_SELECT) for r in (0.75, 0.97) for kind in KINDS]


@pytest.mark.parametrize("ratio,kind,bits,delta,flags", CELLS)
def test_high_ratio_small_layout(cuda, ratio, kind, bits, delta, flags):
    """Ratios in (0.5, 1): bit-exact, the kernel's brackets equal the model's, and the raw-data path is taken by exactly
    the segments the model predicts with ccap_for([ratio]) = 4096 record slots per unit (so only a bracket miss can)."""
    xs, bases, seen = inputs(kind, delta)
    assert ccap_for([ratio]) == 4096
    plan, g, r = run_both(SIZES, ratio, bits, [xs], None if bases is None else [bases], flags=flags, brackets=True)
    assert not plan.dense
    assert_same(plan, g, r)
    check_brackets_and_raw_path(plan, g, seen, ccap_for([ratio]), generic=bool(flags))
    assert np.diff(r["ustart"]).max() > 2400  # a unit's kept entries: far past the 512 staged / register-held ones


# -- 2. the open lower bracket ----------------------------------------------------------------------------------------
def test_open_lower_bracket_is_reached(cuda):
    """Ratio 0.97 on Gaussian data: the sampled lower rank ceil(p m + 6 sqrt(p m) + 8) does not exist among the m sampled
    keys of the 1025-, 4097- (m = 1024) and 2^20-element (m = 8192) segments, so the kernel leaves T_lo = 0 without the
    tie flag: zero-tie mode with K = 0 on data without a single zero — every element a record, the ragged last units
    through scan_unit's CHECK form — and still bit-exact, with no raw-path fallback."""
    xs, _, seen = inputs("gauss", False)
    plan, g, r = run_both(SIZES, 0.97, 8, [xs], brackets=True)
    br = check_brackets_and_raw_path(plan, g, seen, ccap_for([0.97]))
    for s in (0, 1, 5):
        assert br[s][0] == 0 and 0 < br[s][1] < KEY_MAX, (s, br[s])
    lu = 0
    for s in LARGE:  # ... read from the kernel's own output, not through the model
        if s in (0, 1, 5):
            assert int(g["tlo"][lu]) == 0 and not int(g["tlo"][lu]) & TIE_FLAG
        lu += (SIZES[s] + 4095) // 4096
    assert all((x != 0).all() for x in xs)
    assert g["fallbacks"] == 0
    assert_same(plan, g, r)


# -- 3. extreme k from explicit rows ------------------------------------------------------------------------------
def extreme_inputs(kind, ks):
    """gauss / zeros30 / special: the layout of that kind. "one" / "equal": Gaussian, but the large segments keeping
    k = 1 and k = n - 1 are all-zero-but-one / of equal |x| (their tie quota is k - 1 of n - 1 zeros, or k of n)."""
    if kind in ("one", "equal"):
        rng = np.random.default_rng(17)
        return [segment(rng, kind, n) if i in LARGE and k in (1, n - 1) else x
                for i, (n, k, x) in enumerate(zip(SIZES, ks, layout("gauss")))]
    return layout(kind)


@functools.lru_cache(maxsize=None)
def explicit_plan(kind, order, bits):
    ks = extreme_ks(order) if kind == "extreme" else mixed_ks()
    rows = explicit_rows(SIZES, ks)
    if kind == "mixed" and order:
        rows = rows[::-1].copy()
    return CodecPlan.from_segments(rows, bits)


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("bits", [8, 32])
@pytest.mark.parametrize("kind", ["gauss", "zeros30", "special", "one", "equal"])
@pytest.mark.parametrize("order", [0, 1])
def test_extreme_k_explicit_rows(cuda, order, kind, bits, delta):
    """Any 1 <= k <= n per segment (coalac.h): the large segments keep 1, 2, n - 1, n, n // 2 + 1 and ceil(n / 1000)
    elements (order 1: that list reversed, so 2^20 elements keep one), the small ones n and 1, in one plan that is not
    dense. k = 1 / 2 leave T_hi open; k = n and n - 1 leave T_lo = 0 and the k-th key is the segment's minimum key (a zero
    in zeros30 and "one", a denormal in "special", where k = 1 / 2 keep NaNs). Encode, both decodes, the brackets and the
    raw-path count, bit-exact."""
    plan = explicit_plan("extreme", order, bits)
    assert not plan.dense
    ks = extreme_ks(order)
    ds = extreme_inputs(kind, ks)
    xs, bases, seen = ds, None, ds
    if delta:
        bases = base_layout()
        xs, seen = with_base(ds, bases)
    _, g, r = run_plan(plan, xs, bases, brackets=True)
    assert_same(plan, g, r)
    br = check_brackets_and_raw_path(plan, g, seen, ccap_for([1.0]))
    for s in LARGE if kind == "gauss" else ():  # (equal |x| at k = 1: tie mode, T_lo = T_hi = K)
        if ks[s] <= 2:
            assert br[s][1] == KEY_MAX
        if ks[s] >= SIZES[s] - 1:
            assert br[s][0] == 0
    if kind == "special" and not delta:
        s1 = ks.index(1)
        assert np.isnan(seen[s1][r["idx"][int(plan.table.segs[s1, 3])]])  # k = 1 keeps a NaN (NaN keys sort on top)


# -- 4. very different ratios in one plan -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "grid"])
@pytest.mark.parametrize("order", [0, 1])
def test_mixed_ratios_in_one_plan(cuda, order, kind):
    """Large segments at ratios 0.001, 0.9, 0.01, 0.999, 0.3, 0.6 in one plan (order 1: the same rows reversed): rmax >
    0.475, so ccap = 4096 and the high-ratio kernel variants run for the ratio-0.001 segment too."""
    plan = explicit_plan("mixed", order, 8)
    ks = mixed_ks()
    assert not plan.dense and max(k / n for k, n in zip(ks, SIZES)) > 0.475 and ccap_for(MIXED_RATIOS) == 4096
    xs = layout(kind)
    if order:
        xs = xs[::-1]
    _, g, r = run_plan(plan, xs, brackets=True)
    assert_same(plan, g, r)
    check_brackets_and_raw_path(plan, g, xs, ccap_for(MIXED_RATIOS))


# -- 5. a batch plan ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_inputs():
    rng = np.random.default_rng(5)
    xs = list(layout("gauss"))
    xs[5] = layout("zeros30")[5]
    xs.append((rng.standard_normal(PAD) * 1e-3).astype(F32))
    bases = list(base_layout()) + [(rng.standard_normal(PAD) * 1e-2).astype(F32)]
    return xs, bases


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("ratio", [0.75, 0.97])
def test_high_ratio_batch_plan(cuda, ratio, delta):
    """The small layout + one 33.6 M-element segment: > 8192 units, the batch kernels (staged k_scan, 4 units per k_emit
    wave, the tiled decode) with ~3000-4000 entries per unit. Gaussian, the 2^20-element segment 30 % zeros: bit-exact.
    (The oracle's pass over 33.6 M elements on the host dominates the run time.)"""
    ds, bases = batch_inputs()
    xs = ds
    if delta:
        xs, _ = with_base(ds, bases)
    plan, g, r = run_both(SIZES + [PAD], ratio, 8, [xs], [bases] if delta else None)
    assert plan.n_units > 8192  # a batch plan
    assert_same(plan, g, r)
    assert g["fallbacks"] == 0


# -- 6. the decode's other consumers -----------------------------------------------------------------------------------
def client_inputs(c):
    return [layout("gauss", seed=10 + c), layout("zeros30", seed=10 + c), layout("grid", seed=10 + c)][c % 3]


def aggregate_at_high_ratio(ratio, bits, delta):
    """Three clients (Gaussian, 30 % zeros, grid) of the small
    layout, the fused decode + FedAvg in modes recip and sum, with the encoder's starts and without, against
    O.aggregate, bit for bit."""
    C = 3
    plan = CodecPlan(SIZES, ratio, bits, clients=C)
    t = plan.table
    ds = [client_inputs(c) for c in range(C)]
    bases = base_layout(seed=3) if delta else None
    xs = ds if bases is None else [with_base(d, bases)[0] for d in ds]
    flat = flat_of(t.segs, [x for c in range(C) for x in xs[c]])
    base1 = None if bases is None else flat_of(t.segs[:len(SIZES)], bases)
    base1 = None if base1 is None else np.concatenate([base1, np.zeros(t.span_per_client - base1.size, F32)])
    d_base = None if base1 is None else torch.from_numpy(base1).cuda()
    enc = plan.encode(torch.from_numpy(flat).cuda(), base=None if d_base is None else d_base.repeat(C))
    weights = [17, 5, 1000]
    segs = t.segs.astype(np.int64)
    h = [x.cpu().numpy() for x in (enc.idx, enc.vals, enc.mn, enc.scale)]
    ref_enc = O.encode(flat, segs, bits, base=None if base1 is None else np.tile(base1, C))
    np.testing.assert_array_equal(h[0], ref_enc[0])
    assert np.diff(O.unit_starts(ref_enc[0], segs)).max() > 3000
    v1 = Encoded(enc.idx, enc.vals, enc.mn, enc.scale)
    for mode, om in (("recip", O.AGG_RECIP), ("sum", O.AGG_SUM)):
        ref = O.aggregate(*h, segs, bits, C, weights, sum(weights), om, base=base1, out_span=t.span_per_client)
        for e in (enc, v1):
            out = plan.aggregate(e, weights, base=d_base, mode=mode)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            for off, n in zip(t.offsets, t.sizes):
                np.testing.assert_array_equal(got[off:off + n].view(np.uint32), ref[off:off + n].view(np.uint32))


SENTINEL = F32(-12345.5)


def ef_commit_at_high_ratio(ratio, bits, kind):
    """ef_commit after encode on one client against
    tests/ef_model.commit, the whole buffer with a sentinel in the padding gaps; a unit holds > 3000 kept entries."""
    plan = CodecPlan(SIZES, ratio, bits)
    segs = plan.table.segs.astype(np.int64)
    a = np.full(plan.span, SENTINEL, F32)
    for (off, n, _, _), x in zip(segs, layout(kind, seed=4)):
        a[off:off + n] = x
    inside = np.zeros(plan.span, bool)
    for off, n, _, _ in segs:
        inside[off:off + n] = True
    assert not inside.all()  # the layout has padding gaps
    want_enc = O.encode(a, segs, bits)
    want_r = M.commit(a, *want_enc, segs, bits)
    assert np.diff(O.unit_starts(want_enc[0], segs)).max() > 3000
    rd = torch.from_numpy(a.copy()).cuda()
    enc = plan.encode(rd)
    plan.ef_commit(enc, rd)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(enc.idx.cpu().numpy(), want_enc[0])
    np.testing.assert_array_equal(bits_of(enc.vals) if bits == 32 else enc.vals.cpu().numpy(),
                                  bits_of(want_enc[1]) if bits == 32 else want_enc[1])
    np.testing.assert_array_equal(bits_of(enc.mn), bits_of(want_enc[2]))
    np.testing.assert_array_equal(bits_of(enc.scale), bits_of(want_enc[3]))
    got = rd.cpu().numpy()
    np.testing.assert_array_equal(bits_of(got), bits_of(want_r))
    assert (got[~inside] == SENTINEL).all()
    assert (bits_of(got) != bits_of(a)).sum() > 0


CONSUMERS = [("aggregate", r, b, d) for r in (0.75, 0.97) for b in (8, 32) for d in (False, True)]
CONSUMERS += [("ef_commit", r, b, kind) for r in (0.75, 0.97) for b in (8, 32) for kind in ("gauss", "zeros30")]


@pytest.mark.parametrize("consumer,ratio,bits,variant", CONSUMERS)
def test_decode_consumers_at_high_ratio(cuda, consumer, ratio, bits, variant):
    """The kept entries' other readers at ~3000-4000 entries per unit: k_aggregate (variant: with a base or without) and
    k_ef_commit (variant: the input kind), each against its CPU restatement, bit for bit."""
    if consumer == "aggregate":
        aggregate_at_high_ratio(ratio, bits, variant)
    else:
        ef_commit_at_high_ratio(ratio, bits, variant)
