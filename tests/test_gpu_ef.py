"""Error feedback on the GPU (coalac_ef_accumulate / coalac_ef_commit through CodecPlan, the codec and the hooks)
against the CPU restatement tests/ef_model.py, bit for bit.

One small layout exercises every path of the two kernels: one-element and sub-unit segments, a segment of exactly one
4096-element unit and one of a unit + 1, n % 4 in {0, 1, 3} (dword tails and padding gaps between segments),
multi-unit segments, and at ratio 0.1 more than 64 kept entries per unit (the commit's entry loop wraps).
"""
import copy
import functools

import numpy as np
import pytest
import torch

from coala_amd.compression import (CodecPlan, CompressionClientMixin, CompressionServerMixin, UpdateCodec,
                                   flatten_state)
from coala_amd.fl import LoopbackClient, LoopbackServer
from coala_amd.layouts import build_module
from oracle import codec_oracle as O
from tests import ef_model as M
from tests.ef_model import EFOracleBackend, bits_of

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [1, 5, 300, 4096, 4097, 8195, 20000, 70001]
SENTINEL = F32(-12345.5)


def eq(a, b, msg=""):
    np.testing.assert_array_equal(bits_of(a), bits_of(b), err_msg=msg)


@functools.lru_cache(maxsize=None)
def plan_for(ratio, bits, clients=1):
    return CodecPlan(SIZES, ratio, bits, clients=clients, device="cuda")


def inside_mask(plan):
    m = np.zeros(plan.span, bool)
    for off, n, _, _ in plan.table.segs.astype(np.int64):
        m[off:off + n] = True
    return m


@functools.lru_cache(maxsize=None)
def data(span, seed):
    """Three independent standard-normal fp32 arrays (x, base, r) of the plan's span."""
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(span).astype(F32) for _ in range(3))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_payload(enc, want, bits):
    idx, vals, mn, sc = want
    np.testing.assert_array_equal(enc.idx.cpu().numpy(), idx)
    if bits == 32:
        eq(enc.vals, vals)
    else:
        np.testing.assert_array_equal(enc.vals.cpu().numpy(), vals)
    eq(enc.mn, mn)
    eq(enc.scale, sc)


# -- accumulate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("source", ["flat", "segptr"])
@pytest.mark.parametrize("clients", [1, 2])
def test_accumulate(cuda, source, with_base, clients):
    plan = plan_for(0.01, 8, clients)
    segs = plan.table.segs.astype(np.int64)
    x, base, r = data(plan.span, 1)
    mask = inside_mask(plan)
    assert not mask.all()  # the layout has padding gaps
    r = np.where(mask, r, SENTINEL)
    b = base if with_base else None
    want = M.accumulate(x, r, segs, b)
    eq(want[~mask], np.full((~mask).sum(), SENTINEL))
    rd = dev(r)
    if source == "flat":
        out = plan.ef_accumulate(rd, flat=dev(x), base=None if b is None else dev(b))
    else:
        tensors = [dev(x[off:off + n]) for off, n, _, _ in segs]  # every segment in storage of its own
        out = plan.ef_accumulate(rd, tensors=tensors, base=None if b is None else dev(b))
    assert out is rd
    eq(rd, want)  # the whole buffer: every segment element, and the sentinel in every gap


def test_accumulate_argument_checks(cuda):
    plan = plan_for(0.01, 8)
    r = torch.zeros(plan.span, device="cuda")
    x = torch.zeros(plan.span, device="cuda")
    with pytest.raises(ValueError, match="exactly one"):
        plan.ef_accumulate(r)
    with pytest.raises(ValueError, match="exactly one"):
        plan.ef_accumulate(r, flat=x, tensors=[x])
    with pytest.raises(ValueError, match="residual"):
        plan.ef_accumulate(r[:-4], flat=x)
    with pytest.raises(ValueError, match="residual"):
        plan.ef_accumulate(torch.zeros(plan.span + 1, device="cuda")[1:], flat=x)
    with pytest.raises(ValueError, match="residual"):
        plan.ef_accumulate(r.cpu(), flat=x)
    enc = plan.encode(x)
    with pytest.raises(ValueError, match="residual"):
        plan.ef_commit(enc, r.double())
    enc.ustart = None
    with pytest.raises(ValueError, match="ustart"):
        plan.ef_commit(enc, r)


# -- commit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("clients", [1, 2])
@pytest.mark.parametrize("bits", [1, 8, 32])
@pytest.mark.parametrize("ratio", [0.01, 0.1])
def test_commit_after_encode(cuda, ratio, bits, clients):
    plan = plan_for(ratio, bits, clients)
    segs = plan.table.segs.astype(np.int64)
    a = np.where(inside_mask(plan), data(plan.span, 2)[0], SENTINEL)
    want_enc = O.encode(a, segs, bits)
    want_r = M.commit(a, *want_enc, segs, bits)
    if ratio == 0.1:  # a unit holds more than 64 (and more than 128) kept entries
        assert np.diff(O.unit_starts(want_enc[0], segs)).max() > 128
    rd = dev(a)
    enc = plan.encode(rd)
    eq(rd, a)  # (the encode reads only)
    plan.ef_commit(enc, rd)
    check_payload(enc, want_enc, bits)
    eq(rd, want_r)
    assert (bits_of(rd) != bits_of(a)).sum() > 0


@pytest.mark.parametrize("bits", [8, 32])
def test_dense_plan(cuda, bits):
    plan = plan_for(1.0, bits)
    assert plan.dense
    segs = plan.table.segs.astype(np.int64)
    mask = inside_mask(plan)
    a = np.where(mask, data(plan.span, 3)[0], SENTINEL)
    want_enc = O.encode(a, segs, bits)
    want_r = M.commit(a, *want_enc, segs, bits)
    rd = dev(a)
    enc = plan.encode(rd)
    assert enc.idx.numel() == 0  # implied indices: the commit is positional
    plan.ef_commit(enc, rd)
    eq(rd, want_r)
    if bits == 32:
        assert not bits_of(rd)[mask].any()  # everything was delivered: +0.0 everywhere
    eq(rd[torch.from_numpy(~mask).cuda()], np.full((~mask).sum(), SENTINEL))


def test_three_rounds_on_one_residual(cuda):
    plan = plan_for(0.01, 8)
    segs = plan.table.segs.astype(np.int64)
    r = np.zeros(plan.span, F32)
    rd = torch.zeros(plan.span, device="cuda")
    base = data(plan.span, 4)[1]
    bd = dev(base)
    for t in range(3):
        x = base + F32(0.01) * data(plan.span, 10 + t)[0]
        want_enc, r = M.ef_round(x, r, segs, 8, base)
        plan.ef_accumulate(rd, flat=dev(x), base=bd)
        enc = plan.encode(rd)
        plan.ef_commit(enc, rd)
        check_payload(enc, want_enc, 8)
        eq(rd, r, f"round {t}")


@pytest.mark.parametrize("bits", [8, 32])
def test_special_values(cuda, bits):
    plan = plan_for(0.01, bits)
    segs = plan.table.segs.astype(np.int64)
    a = data(plan.span, 5)[0].copy()
    off = {int(n): int(o) for o, n, _, _ in segs}
    # 300 elements, k = 3: five NaN (the largest keys, lower index first) and three +-Inf: three NaN are kept, the
    # other two and the infinities are not
    s = off[300]
    a[s + 10:s + 15] = np.nan
    a[s + 20:s + 23] = [np.inf, -np.inf, np.inf]
    # 20000 elements, k = 200: every non-finite value is kept
    s = off[20000]
    a[s + 7], a[s + 4096], a[s + 19999] = np.nan, np.inf, -np.inf
    # 4096 elements, k = 41: ten non-zero values, the rest +-0.0, so zeros of both signs are kept and not kept
    s = off[4096]
    z = np.zeros(4096, F32)
    z[1::2] = -0.0
    z[100:110] = np.arange(1, 11, dtype=F32)
    a[s:s + 4096] = z
    want_enc = O.encode(a, segs, bits)
    want_r = M.commit(a, *want_enc, segs, bits)
    kept = np.zeros(plan.span, bool)
    for o, n, k, oo in segs:
        kept[o + want_enc[0][oo:oo + k]] = True
    nonfin = ~np.isfinite(a)
    assert (kept & nonfin).sum() == 6 and (~kept & nonfin).sum() == 5
    zero = (bits_of(a) << 1) == 0
    assert (kept & zero).sum() == 31 and (~kept & zero).sum() > 4000
    rd = dev(a)
    enc = plan.encode(rd)
    plan.ef_commit(enc, rd)
    check_payload(enc, want_enc, bits)
    got = rd.cpu().numpy()
    eq(got, want_r)
    assert not bits_of(got)[kept & nonfin].any()  # kept non-finite entries: +0.0
    eq(got[~kept], a[~kept])  # not kept: unchanged, NaN / Inf / -0.0 included
    assert np.isfinite(got[kept]).all()


# -- codec and hooks ------------------------------------------------------------------------------
def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_((torch.randn(p.shape, generator=g) * 1e-2).to(p.device))


def test_codec_segptr_path_equals_flat_path_and_model(cuda):
    codec = UpdateCodec(0.01, 8, "delta")
    g = build_module("lenet", seed=2, device="cuda")
    m = copy.deepcopy(g)
    snap = codec.snapshot(g)
    res_mod, res_state = codec.new_residual(m), codec.new_residual(m.state_dict())
    assert res_mod.device.type == "cuda" and res_mod.dtype == torch.float32 and not res_mod.any()
    plan = codec.plan_for(tuple(int(v.numel()) for v in m.state_dict().values() if v.dtype == torch.float32),
                          res_mod.device)
    assert res_mod.numel() == plan.table.span >= plan.span  # (the flat layout's length, its last segment padded)
    segs = plan.table.segs.astype(np.int64)
    r = np.zeros(plan.table.span, F32)
    for t in range(2):
        _perturb(m, 20 + t)
        up = codec.encode_module(m, base=snap, residual=res_mod)  # the parameters read through their pointers
        # the same state as tensors at odd offsets of one buffer (misaligned: the flattened path)
        state = m.state_dict()
        odd = {}
        for k, v in state.items():
            buf = torch.empty(v.numel() + 1, dtype=v.dtype, device=v.device)
            buf[1:].copy_(v.reshape(-1))
            odd[k] = buf[1:].view(v.shape)
        up_flat = codec.encode(odd, base=snap, residual=res_state)
        x = flatten_state(state).flat.cpu().numpy()
        want_enc, r = M.ef_round(x, r, segs, 8, snap.flat.cpu().numpy())
        for u in (up, up_flat):
            check_payload(u.encoded, want_enc, 8)
            assert u.header["mode"] == "delta"
        eq(res_mod, r, f"round {t}")
        eq(res_state, r, f"round {t} (flat path)")
        assert up.to_bytes() == up_flat.to_bytes()
    with pytest.raises(ValueError, match="residual"):
        codec.encode_module(m, base=snap, residual=res_mod.cpu())


def test_hooks_one_client_two_rounds(cuda):
    def classes(backend, device):
        class Client(CompressionClientMixin, LoopbackClient):
            codec_ratio, codec_bits, codec_mode, codec_backend = 0.01, 8, "delta", backend
            codec_error_feedback = True

            def __init__(self, *a, **k):
                super().__init__(*a, device=device, **k)

        class Server(CompressionServerMixin, LoopbackServer):  # unmodified: no error-feedback setting
            codec_ratio, codec_bits, codec_mode, codec_backend = 0.01, 8, "delta", backend

        return Client, Server

    g0 = build_module("lenet", seed=4)
    Cg, Sg = classes(None, "cuda")
    Co, So = classes(EFOracleBackend(), "cpu")
    hip = Sg(copy.deepcopy(g0), [Cg("c0", 10, step_seed=1)])
    ora = So(copy.deepcopy(g0), [Co("c0", 10, step_seed=1)])
    for t in range(2):
        hip.distribution_to_train(t)
        ora.distribution_to_train(t)
        a, b = hip.uploaded["c0"].state_dict(), ora.uploaded["c0"].state_dict()
        for (k, x), (k2, y) in zip(a.items(), b.items()):
            assert k == k2 and x.dtype == y.dtype
            if x.dtype == torch.float32:
                eq(x, y, k)
            else:
                assert torch.equal(x.cpu(), y), k
        rh, ro = hip.clients[0]._codec_residual[1], ora.clients[0]._codec_residual[1]
        assert rh.device.type == "cuda" and rh.any()
        eq(rh, ro, f"round {t}")
        hip.aggregation()
        ora.model.load_state_dict(hip.model.state_dict())
    hip.clients[0].reset_error_feedback()
    assert not hip.clients[0]._codec_residual[1].any()
