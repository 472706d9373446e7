"""The encode's select chain (k_ghist -> k_gwin -> k_select, coala_amd/csrc/coalac.hip) on the hand-built segments of
tests/select_inputs.py: every route of tests/select_model.py, every loop boundary, in latency-bound and batch plans at
rmax 0.01 and 0.05.

One encode per plan, into buffers pre-filled with sentinels and fenced by canary pads. Then per case: the whole idx /
codes / mn / scale / per-unit starts of the case's segment and of the small segment after it are bit-identical to
oracle.codec_oracle (a reserved-but-unwritten slot or a shifted offset shows in the neighbour), the pads are untouched,
the kernel's bracket equals the model's, and the fallback counter equals the number of segments the model sends to a
raw-data route, exactly. tests/test_select_model_cpu.py proves without a GPU that each case takes the route it claims.

Case -> route (select_inputs; * = the case's k needs rmax 0.05, so in the rmax-0.01 plans its rows hold a Gaussian):
  window          window_first_in_list, window_last_in_list, window_rank_1, window_rank_W, window_bin_0,
                  window_bin_last_clamped, window_list_65_256, wlist_1024, rank0_sa_eq_k_minus_1*, window_sc_eq_k,
                  ccap_exact_rmax0.01, ccap_exact_rmax0.05, tie_0_sc, window_sign_kept, window_sign_dropped,
                  window_N and quota_N for N = 32, 33, 768, 769, 1536, 1537, 2048, window_hist_tail_1500
  window_gcap     gcap_257, gcap_257_last_group
  window_wlist    wlist_1025
  generic_rank0   rank0_sa_eq_k*, tie_K_sc, rank0_32*, rank0_33*, rank0_768, rank0_769, rank0_1536, rank0_1537, rank0_2048
  generic_forced  window_2049, quota_2049, rank0_2049_forced (and any case under COALAC_FLAG_GENERIC_SELECT)
  tie_shortcut    tie_K_sc+1, tie_K_sc+sz*, tie_0_sc+1, tie_0_mid, tie_sign_kept, tie_sign_dropped, tie_N for N = 32, 33*,
                  768, 769, 1536, 1537, 2048
  raw_miss_high   miss_high_sa_eq_k_plus_1*
  raw_miss_low    miss_low_sc_eq_k_minus_1, tie_K_sc+sz+1*, tie_2049
  raw_ccap        ccap_plus_1_rmax0.01, ccap_plus_1_rmax0.05 (each in the plans of its rmax only)
  raw_forced      every case under COALAC_FLAG_FORCE_EXACT
  The Gaussian pin, filler and stand-in segments take the window route; the 8200-unit filler is generic_forced.

That the cases run the routes they claim was shown once with value-only marker mutants (a constant folded into gmx in the
route's own code, on a scratch copy; the bits-8 plans without flags, so each case up to 4 times). Failing cases:
  after window_resolve          every case listed under window, plus the Gaussian stand-ins and every plan's pin / filler
  in select_generic             gcap_257, gcap_257_last_group, wlist_1025 (they run it after the fall-through), every
                                generic_rank0 and generic_forced case, the batch plans' filler; nothing else
  the raw branch                ccap_plus_1_rmax0.01, ccap_plus_1_rmax0.05, miss_high_sa_eq_k_plus_1,
                                miss_low_sc_eq_k_minus_1, tie_K_sc+sz+1, tie_2049; nothing else
  the zero_tie branch           every case listed under tie_shortcut; nothing else
  the `return false` fall-through   gcap_257, gcap_257_last_group, wlist_1025; nothing else
  `fn_rank <= rt`               tie_sign_dropped alone (window_sign_* hinge on `fp_rank < rt`, the mirrored comparison)
Not run: dropping the `g >= GB` histogram tail of segment_pick. It makes window_hist_tail_1500 pick a lower window, whose
k-th key has more than k keys above it (tests/test_select_model_cpu.py::test_histogram_tail_changes_the_window): the
kept count changes, so k_emit would write past the segment, and its detection rests on that CPU argument. The other
window cases above 768 units go silent under it (hist_pick finds no bin, the generic select is exact).

An error in segment_pick's sa / sc tail sums only moves a segment to a slower route that is still exact: the fallback
count catches the raw half of that; the generic half is not observable through the ABI."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, Encoded
from coala_amd.compression._lib import COALAC_FLAG_FORCE_EXACT, COALAC_FLAG_GENERIC_SELECT
from oracle import codec_oracle as O
from tests import select_inputs as I
from tests import select_model as M
from tests.sampler_model import bracket, ccap_for, takes_raw_path

pytestmark = pytest.mark.gpu

PAD = 64  # canary elements before and after every output buffer
SENT_I32 = -0x5A5A5A5B
SENT_F32 = np.float32(-12345.5)

# (part, rmax, batch, bits, delta, flags)
PLANS = [(p, r, b, 8, False, 0) for p in range(len(I.PARTS)) for r in I.RMAX for b in (False, True)]
PLANS += [(0, 0.05, b, 32, False, 0) for b in (False, True)]       # the raw routes and the 40-unit windows: raw values
PLANS += [(0, 0.05, b, 8, True, 0) for b in (False, True)]         # ... and delta mode
PLANS += [(0, 0.01, False, 8, False, f) for f in (COALAC_FLAG_FORCE_EXACT, COALAC_FLAG_GENERIC_SELECT)]


def plan_id(key):
    p, r, b, bits, delta, flags = key
    return f"part{p}-rmax{r}-{'batch' if b else 'latency'}-bits{bits}{'-delta' if delta else ''}{f'-flags{flags}' if flags else ''}"


@functools.lru_cache(maxsize=None)
def oracle_of(key, bits):
    """encode_segment of one segment, once: key names the array (a case, a small segment's row, a Gaussian size)."""
    kind, a, k = key
    x = I.case(a).x if kind == "case" else I.small_segment(a) if kind == "small" else I.gaussian(a)
    return O.encode_segment(x, k, bits)


@functools.lru_cache(maxsize=None)
def raw_of(kind, a, k, row, ccap, flags):
    """Whether the model sends this segment to a raw-data route."""
    if flags & COALAC_FLAG_FORCE_EXACT:
        return True
    if kind == "case":
        c = I.case(a)
        return M.route_of(c.x, k, row, ccap, flags).raw
    x = I.gaussian(a)
    tlo, thi, _ = bracket(x, k, row)
    return takes_raw_path(x, k, tlo, thi, ccap, generic=bool(flags & COALAC_FLAG_GENERIC_SELECT))


def fenced(n, dtype, fill):
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


@functools.lru_cache(maxsize=2)
def run_plan(key):
    part, rmax, batch, bits, delta, flags = key
    rows, xs, names = I.plan_rows(part, rmax, batch)
    plan = CodecPlan.from_segments(rows, bits)
    segs = rows.astype(np.int64)
    large = [i for i, x in enumerate(xs) if x.size > I.SMALL_N]
    assert not plan.dense and (sum((xs[i].size + 4095) // 4096 for i in large) > 8192) == batch
    ccap = ccap_for([max(int(segs[i, 2]) / int(segs[i, 1]) for i in large)])
    assert ccap == I.CCAP[rmax]
    span = int((segs[:, 0] + segs[:, 1]).max())
    flat = np.zeros(span, np.float32)
    for (off, n, _, _), x in zip(segs, xs):
        flat[off:off + n] = x
    d_base = None
    if delta:  # base = d, input = 2 d: the difference is d again, exactly (a zero's sign aside: no key, no code changes)
        d_base = torch.from_numpy(flat).cuda()
        flat = flat * np.float32(2)
        assert np.array_equal(flat - flat / 2, flat / 2)
    d_flat = torch.from_numpy(flat).cuda()
    del flat
    K, T, U = plan.total_k, plan.n_segments, plan.n_units
    raw32 = bits == 32
    bufs = [fenced(K, torch.int32, SENT_I32), fenced(K, torch.float32 if raw32 else torch.uint8, float(SENT_F32) if raw32 else 0xA5),
            fenced(T, torch.float32, float(SENT_F32)), fenced(T, torch.float32, float(SENT_F32)),
            fenced(U, torch.int32, SENT_I32)]
    ws = plan.empty_workspace()
    plan.encode(d_flat, base=d_base, workspace=ws, flags=flags, out=Encoded(*[v for _, v in bufs]))
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b, _ in bufs]
    pads_ok = all((h[:PAD] == h[0]).all() and (h[-PAD:] == h[0]).all() and
                  h[0] == (SENT_I32 if h.dtype == np.int32 else 0xA5 if h.dtype == np.uint8 else SENT_F32) for h in host)
    g = dict(zip(("idx", "vals", "mn", "scale", "ustart"), [h[PAD:-PAD] for h in host]))
    g["pads_ok"], g["fallbacks"] = pads_ok, plan.fallbacks(ws)
    nl = sum((xs[i].size + 4095) // 4096 for i in large)
    lo, hi = (ctypes.c_uint32 * nl)(), (ctypes.c_uint32 * nl)()
    assert plan._lib.coalac_debug_brackets(plan._h, ctypes.c_void_p(ws.data_ptr()), None, lo, hi, nl) == nl
    g["tlo"], g["thi"] = np.frombuffer(lo, np.uint32).copy(), np.frombuffer(hi, np.uint32).copy()
    # where each row's units and large units start
    nus = [(x.size + 4095) // 4096 for x in xs]
    g["ubeg"] = np.concatenate([[0], np.cumsum(nus)])
    g["lbeg"] = np.concatenate([[0], np.cumsum([nu if i in set(large) else 0 for i, nu in enumerate(nus)])])
    kinds = []
    for i, x in enumerate(xs):
        kinds.append(("case", names[i]) if names[i] else ("small", i) if x.size == I.SMALL_N else ("gauss", nus[i]))
    g["raw_expected"] = sum(raw_of(kinds[i][0], kinds[i][1], int(segs[i, 2]), i, ccap, flags) for i in large)
    plan.close()
    return segs, names, kinds, g


def check_row(segs, kinds, g, i, bits):
    off, n, k, oo = (int(v) for v in segs[i])
    idx, vals, mn, sc = oracle_of((kinds[i][0], kinds[i][1], k), bits)
    np.testing.assert_array_equal(g["idx"][oo:oo + k], idx)
    np.testing.assert_array_equal(g["vals"][oo:oo + k].view(np.uint32 if bits == 32 else np.uint8),
                                  vals.view(np.uint32 if bits == 32 else np.uint8))
    assert g["mn"][i:i + 1].view(np.uint32)[0] == np.float32(mn).view(np.uint32), (g["mn"][i], mn)
    assert g["scale"][i:i + 1].view(np.uint32)[0] == np.float32(sc).view(np.uint32), (g["scale"][i], sc)
    u0, u1 = int(g["ubeg"][i]), int(g["ubeg"][i + 1])
    want = np.searchsorted(idx, np.arange(u1 - u0, dtype=np.int64) * 4096, side="left")
    np.testing.assert_array_equal(g["ustart"][u0:u1], want)


CELLS = [(key, name) for key in PLANS for name in I.PARTS[key[0]] + ["rest_of_the_plan"]]


@pytest.mark.parametrize("key,name", CELLS, ids=[f"{plan_id(k)}-{n}" for k, n in CELLS])
def test_case(cuda, key, name):
    if name == "rest_of_the_plan":
        return check_rest_of_the_plan(key)
    segs, names, kinds, g = run_plan(key)
    bits, flags = key[3], key[5]
    i = I.ROW_OF[name][1]
    if names[i] is None:  # this plan's rmax cannot hold the case (select_inputs.plan_rows): its rows hold a Gaussian
        assert I.case(name).min_rmax > key[1] or I.case(name).only_rmax not in (None, key[1])
    check_row(segs, kinds, g, i, bits)       # the case's segment
    check_row(segs, kinds, g, i + 1, bits)   # the small segment after it
    assert g["pads_ok"]
    assert g["fallbacks"] == g["raw_expected"], (g["fallbacks"], g["raw_expected"])
    if names[i] is not None:
        c = I.case(name)
        l0, l1 = int(g["lbeg"][i]), int(g["lbeg"][i + 1])
        assert l1 - l0 == c.nu
        assert (g["tlo"][l0:l1] == c.bracket0[0]).all() and (g["thi"][l0:l1] == c.bracket0[1]).all(), \
            (hex(int(g["tlo"][l0])), hex(int(g["thi"][l0])), [hex(v) for v in c.bracket0[:2]])


def check_rest_of_the_plan(key):
    """The pin segment and the filler (shared by every case of the plan), and no sentinel left in idx or the starts."""
    segs, names, kinds, g = run_plan(key)
    for i in range(2 * len(I.PARTS[key[0]]), len(segs)):
        check_row(segs, kinds, g, i, key[3])
    assert (g["idx"] != SENT_I32).all() and (g["ustart"] != SENT_I32).all()
