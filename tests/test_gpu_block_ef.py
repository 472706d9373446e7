"""k_dense_block_quant_ef (coalac_encode_block_ef) against the model (tests/block_ef_model.py): the
block-wise encode with the client's residual read, added and rewritten in the same launch. Every comparison is
bit-exact (a NaN range compares as NaN: its payload is not part of the spec); one parametrisation is also compared with
the three-step composition of the existing entry points on the GPU. Sentinels around every output and in the residual's
padding and tail must survive."""
import copy

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, CompressionClientMixin, CompressionServerMixin, flatten_state
from coala_amd.fl import LoopbackClient, LoopbackServer
from coala_amd.fl.strategies import federated_averaging
from coala_amd.layouts import build_module
from tests import block_ef_model as M
from tests.block_ef_model import BlockEFOracleBackend
from tests.blockwise_model import BlockOracleBackend
from tests.test_gpu_blockwise import ROWS, _gauss, _same_ranges, _special

pytestmark = pytest.mark.gpu

UNIT = 4096
SIZES = [1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 5]
PAD = 64
SENTINEL = 123.25
KINDS = ["plain", "empty", "batched", "rows"]
_PLANS = {}


def _plan(kind, bits):
    key = (kind, bits)
    if key not in _PLANS:
        if kind == "plain":
            p = CodecPlan(SIZES, 1.0, bits)
        elif kind == "empty":
            p = CodecPlan(SIZES[:5] + [0] + SIZES[5:], 1.0, bits)
        elif kind == "batched":
            p = CodecPlan([33, 4097, 70], 1.0, bits, clients=3)
        elif kind == "special":
            p = CodecPlan([3 * UNIT + 100, 33], 1.0, bits)
        elif kind == "many":
            p = CodecPlan([4] * 8200, 1.0, bits)
        else:
            p = CodecPlan.from_segments(np.array(ROWS, dtype=np.uint64), bits)
        _PLANS[key] = p
    return _PLANS[key]


def _inside(plan, length):
    m = np.zeros(length, bool)
    for off, n, _, _ in plan.table.segs.astype(np.int64).tolist():
        m[off:off + n] = True
    return m


def _residual(plan, seed, scale=0.3):
    """A residual buffer of span + PAD elements: non-zero values inside the segments, sentinels in the padding between
    them and in the tail."""
    r = np.full(plan.span + PAD, SENTINEL, np.float32)
    inside = _inside(plan, r.size)
    r[inside] = (np.random.default_rng(seed).standard_normal(int(inside.sum())) * scale).astype(np.float32)
    return r


def _same_floats(got, want, msg=""):
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=msg)
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32), err_msg=msg)


def _round_and_check(plan, flat, base, r0, segptr):
    """One fused call on the GPU against the model -> (the device residual buffer, the model's outputs)."""
    segs = plan.table.segs.astype(np.int64)
    U, P = plan.n_units, plan.dense_packed_words
    bmn, bsc, _, stream, r1 = M.block_ef_round(flat, r0, segs, plan.bits, base)
    rbuf = torch.full((2, PAD + U + PAD), SENTINEL, dtype=torch.float32, device="cuda")
    obuf = torch.full((16 + P + 64,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    out = (rbuf[0, PAD:PAD + U], rbuf[1, PAD:PAD + U], obuf[16:])
    dres = torch.from_numpy(r0).cuda()
    dbase = None if base is None else torch.from_numpy(base).cuda()
    if segptr:
        tensors = [torch.from_numpy(flat[off:off + n].copy()).cuda() for off, n, _, _ in segs.tolist()]
        plan.encode_block_ef(dres, tensors=tensors, base=dbase, out=out)
    else:
        plan.encode_block_ef(dres, flat=torch.from_numpy(flat).cuda(), base=dbase, out=out)
    torch.cuda.synchronize()
    r, o, res = rbuf.cpu().numpy(), obuf.cpu().numpy(), dres.cpu().numpy()
    _same_ranges(r[0, PAD:PAD + U], bmn)
    _same_ranges(r[1, PAD:PAD + U], bsc)
    np.testing.assert_array_equal(o[16:16 + P], stream)
    assert (r[:, :PAD] == SENTINEL).all() and (r[:, PAD + U:] == SENTINEL).all()
    assert (o[:16] == 0xFFFFFFFF).all() and (o[16 + P:] == 0xFFFFFFFF).all()
    inside = _inside(plan, res.size)
    np.testing.assert_array_equal(res.view(np.uint32), r1.view(np.uint32))
    assert (res[~inside] == SENTINEL).all() and np.isfinite(res[inside]).all()
    return dres, (bmn, bsc, stream, r1)


@pytest.mark.parametrize("segptr", [False, True], ids=["flat", "segptr"])
@pytest.mark.parametrize("delta", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("bits", range(1, 9))
@pytest.mark.parametrize("kind", KINDS)
def test_encode_block_ef(cuda, kind, bits, delta, segptr):
    plan = _plan(kind, bits)
    assert plan.dense and plan.has_block_ef
    flat = _gauss(plan, bits)
    base = _gauss(plan, 100 + bits) if delta else None
    _round_and_check(plan, flat, base, _residual(plan, 200 + bits), segptr)


@pytest.mark.parametrize("bits", [2, 3])
def test_equals_the_three_existing_entry_points(cuda, bits):
    """ef_accumulate; encode_block of the residual without a base; residual -= decode_block of that payload without a
    base (+0.0 where not finite) — on the GPU, from the same inputs."""
    plan = _plan("plain", bits)
    flat, base, r0 = _gauss(plan, 31), _gauss(plan, 32), _residual(plan, 33)
    dres, (bmn, bsc, stream, _) = _round_and_check(plan, flat, base, r0, False)
    three = torch.from_numpy(r0).cuda()
    plan.ef_accumulate(three, flat=torch.from_numpy(flat).cuda(), base=torch.from_numpy(base).cuda())
    tmn, tsc, tpacked = plan.encode_block(flat=three)
    d = plan.decode_block(tpacked, tmn, tsc, out=torch.zeros(three.numel(), device="cuda"))
    inside = torch.from_numpy(_inside(plan, three.numel())).cuda()
    v = three - d
    v = torch.where(torch.isfinite(v), v, torch.zeros_like(v))
    three = torch.where(inside, v, three)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tmn.cpu().numpy().view(np.uint32), bmn.view(np.uint32))
    np.testing.assert_array_equal(tsc.cpu().numpy().view(np.uint32), bsc.view(np.uint32))
    np.testing.assert_array_equal(tpacked.cpu().numpy(), stream)
    np.testing.assert_array_equal(three.cpu().numpy().view(np.uint32), dres.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("bits", [1, 3, 4, 8])
def test_special_values(cuda, bits, start):
    """NaN and +-Inf elements (residual +0.0), an all-NaN unit, a constant unit (scale 0, residual exactly 0),
    denormals and +-0."""
    plan = _plan("special", bits)
    flat = _special(plan)
    r0 = _residual(plan, 5, scale=0.0 if start == "zero" else 1e-3)
    dres, (bmn, bsc, _, r1) = _round_and_check(plan, flat, None, r0, False)
    res = dres.cpu().numpy()
    zero = np.zeros(1, np.float32).view(np.uint32)[0]
    bad = ~np.isfinite(flat[:3 * UNIT + 100])
    assert bad[5] and bad[7] and bad[11] and bad[2 * UNIT:3 * UNIT].all()
    assert (res[:3 * UNIT + 100][bad].view(np.uint32) == zero).all()  # +0.0, not -0.0
    assert np.isnan(bmn[2]) and np.isnan(bsc[2])
    if start == "zero":
        assert bsc[1] == 0 and bmn[1] == 7.5
        assert (res[UNIT:2 * UNIT].view(np.uint32) == zero).all()
        assert bsc[3] == 0 and (res[3 * UNIT:3 * UNIT + 100] == 0).all()


@pytest.mark.parametrize("bits", [2, 3])
def test_three_rounds_with_the_residual_carried(cuda, bits):
    plan = _plan("plain", bits)
    segs = plan.table.segs.astype(np.int64)
    r = _residual(plan, 9, scale=0.0)
    dres = torch.from_numpy(r).cuda()
    for rnd in range(3):
        flat, base = _gauss(plan, 40 + rnd), _gauss(plan, 50 + rnd)
        bmn, bsc, _, stream, r = M.block_ef_round(flat, r, segs, bits, base)
        gmn, gsc, packed = plan.encode_block_ef(dres, flat=torch.from_numpy(flat).cuda(), base=torch.from_numpy(base).cuda())
        torch.cuda.synchronize()
        _same_ranges(gmn.cpu().numpy(), bmn)
        _same_ranges(gsc.cpu().numpy(), bsc)
        np.testing.assert_array_equal(packed.cpu().numpy(), stream)
        np.testing.assert_array_equal(dres.cpu().numpy().view(np.uint32), r.view(np.uint32), err_msg=f"round {rnd}")
    assert np.count_nonzero(r[_inside(plan, r.size)])


@pytest.mark.parametrize("delta", [False, True], ids=["nobase", "base"])
def test_many_small_segments_reach_the_xcd_unit_order(cuda, delta):
    """More than 8192 units, each a 4-element segment: the kernel takes the XCD-aware unit order."""
    plan = _plan("many", 3)
    assert plan.n_units == 8200 > 8192
    flat = _gauss(plan, 3)
    _round_and_check(plan, flat, _gauss(plan, 4) if delta else None, _residual(plan, 6), False)


def test_wrapper_checks_the_residual(cuda):
    plan = _plan("plain", 4)
    x = torch.from_numpy(_gauss(plan, 1)).cuda()
    r = torch.zeros(plan.span, device="cuda")
    for bad in (None, r[:-4], r.double(), r.cpu(), torch.zeros(2 * plan.span, device="cuda")[::2]):
        with pytest.raises(ValueError):
            plan.encode_block_ef(bad, flat=x)
    with pytest.raises(ValueError):
        plan.encode_block_ef(r)
    with pytest.raises(ValueError):
        CodecPlan([5000, 300], 0.1, 4).encode_block_ef(torch.zeros(5312, device="cuda"), flat=torch.zeros(5312, device="cuda"))
    torch.cuda.synchronize()
    assert not r.any()


# -- end to end -----------------------------------------------------------------------------------
def _run(client_backend, server_kw, device, rounds=2):
    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 2, "delta", client_backend
        codec_blockwise, codec_error_feedback = True, True

    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode = 1.0, 2, "delta"

        def aggregate(self, models, weights):
            if self.codec_fused_aggregate:
                return super().aggregate(models, weights)
            # decode-each + FedAvg, the average taken on the GPU (torch's division there) whatever decoded the uploads
            return federated_averaging([copy.deepcopy(m).cuda() for m in models], weights)

    for k, v in server_kw.items():
        setattr(Server, k, v)
    clients = [Client(f"c{i}", 5 + 3 * i, device=device, step_seed=i, step_scale=1e-2) for i in range(3)]
    server = Server(build_module("lenet", seed=7).to(device), clients)
    states = []
    for rnd in range(rounds):
        server.round(rnd)
        states.append(flatten_state(server.model.state_dict()).flat.cpu().numpy().copy())
    return states, [c._codec_residual[1].cpu().numpy().copy() for c in clients]


def test_rounds_end_to_end(cuda):
    """Two rounds of three clients with codec_blockwise + codec_error_feedback on the HIP backend: the server's fused
    dense aggregate (kind BLOCK, delta base), the same server decoding every upload, and the whole run on the model
    backend agree bit for bit, global model and residuals alike. The server side has no switch for this."""
    fused, res_f = _run(None, dict(codec_fused_aggregate=True, codec_fused_dense_aggregate=True), "cuda")
    each, res_e = _run(None, dict(codec_fused_aggregate=False), "cuda")
    model, res_m = _run(BlockEFOracleBackend(), dict(codec_fused_aggregate=False, codec_backend=BlockOracleBackend()), "cpu")
    for rnd in range(2):
        _same_floats(fused[rnd], each[rnd], f"round {rnd}: fused against decode-each")
        _same_floats(each[rnd], model[rnd], f"round {rnd}: HIP against the model backend")
    for a, b, c in zip(res_f, res_e, res_m):
        assert np.count_nonzero(a)
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        np.testing.assert_array_equal(a.view(np.uint32), c.view(np.uint32))
    assert not np.array_equal(fused[0], fused[1])
