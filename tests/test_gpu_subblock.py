"""The block-wise dense kernels with 256- and 1024-element blocks (k_dense_block_quant_g / k_dense_deq_stream_g /
k_aggregate_dense_g) against the CPU model (tests/subblock_model.py): the existing oracle over a segment
table cut into G-element blocks, the stream in wire v4's layout. Every comparison is bit-exact; a NaN compares as NaN
(its payload is not part of the spec). One plan whose segments sit on every side of a row (256), a block and a unit."""
import copy
import pickle

import numpy as np
import pytest
import torch

from coala_amd.compression import (CodecPlan, CompressedModel, CompressionClientMixin, CompressionServerMixin, wire)
from coala_amd.fl import LoopbackClient, LoopbackServer
from coala_amd.layouts import build_module
from tests import subblock_model as SM
from tests.dense_aggregate_model import same_bits

pytestmark = pytest.mark.gpu

UNIT = 4096
SIZES = [0, 1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4096 + 256 + 3, 8192 + 1023]
BLOCKS = [256, 1024]
BITS = [1, 3, 4, 5, 8]  # (3 and 5: a lane's field straddles two words)
LATENCY_PLAN_UNITS = 8192  # coalac.hip: a plan with more units takes the XCD-aware unit order
PAD = 64
SENTINEL = 123.25
_PLANS, _INPUTS, _MODEL = {}, {}, {}


def _plan(bits):
    if bits not in _PLANS:
        _PLANS[bits] = CodecPlan(SIZES, 1.0, bits)
    return _PLANS[bits]


def _segs(plan):
    return plan.table.segs.astype(np.int64)


def _gauss(plan, seed):
    key = (plan.span, seed)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        flat = np.zeros(plan.span, np.float32)
        for off, n, _, _ in _segs(plan).tolist():
            flat[off:off + n] = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
        _INPUTS[key] = flat
    return _INPUTS[key]


def _inside(plan):
    m = np.zeros(plan.span, dtype=bool)
    for off, n, _, _ in _segs(plan).tolist():
        m[off:off + n] = True
    return m


def _model(plan, block, delta, seed=1):
    """(flat, base, bmn, bscale, stream, decoded) of the Gaussian input, computed once per (bits, block, delta, seed)."""
    key = (plan.bits, block, delta, seed)
    if key not in _MODEL:
        flat = _gauss(plan, seed)
        base = _gauss(plan, 100) if delta else None
        bmn, bsc, _, stream = SM.encode(flat, _segs(plan), plan.bits, block, base=base)
        dec = SM.decode(stream, bmn, bsc, _segs(plan), plan.bits, plan.span, block, base=base)
        _MODEL[key] = (flat, base, bmn, bsc, stream, dec)
    return _MODEL[key]


def _encode(plan, block, flat, base, segptr=False):
    """encode_block_g into canaried buffers -> (bmn, bscale, stream) on the host; nothing outside them is written."""
    NB, P = plan.block_count(block), plan.dense_packed_words
    rbuf = torch.full((2, PAD + NB + PAD), SENTINEL, dtype=torch.float32, device="cuda")
    obuf = torch.full((16 + P + 64,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    out = (rbuf[0, PAD:PAD + NB], rbuf[1, PAD:PAD + NB], obuf[16:])
    dbase = None if base is None else torch.from_numpy(base).cuda()
    if segptr:
        tensors = [torch.from_numpy(flat[off:off + n].copy()).cuda() for off, n, _, _ in _segs(plan).tolist()]
        plan.encode_block_g(block, tensors=tensors, base=dbase, out=out)
    else:
        plan.encode_block_g(block, flat=torch.from_numpy(flat).cuda(), base=dbase, out=out)
    torch.cuda.synchronize()
    r, o = rbuf.cpu().numpy(), obuf.cpu().numpy()
    assert (r[:, :PAD] == SENTINEL).all() and (r[:, PAD + NB:] == SENTINEL).all()
    assert (o[:16] == 0xFFFFFFFF).all() and (o[16 + P:] == 0xFFFFFFFF).all()
    return r[0, PAD:PAD + NB], r[1, PAD:PAD + NB], o[16:16 + P]


def _decode(plan, block, stream, bmn, bsc, base):
    out = torch.full((plan.span + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    dbase = None if base is None else torch.from_numpy(base).cuda()
    plan.decode_block_g(block, torch.from_numpy(stream.copy()).cuda(), torch.from_numpy(bmn.copy()).cuda(),
                        torch.from_numpy(bsc.copy()).cuda(), base=dbase, out=out)
    got, inside = out.cpu().numpy(), _inside(plan)
    assert (got[:plan.span][~inside] == SENTINEL).all() and (got[plan.span:] == SENTINEL).all()
    return got[:plan.span], inside


def test_block_counts(cuda):
    plan = _plan(4)
    for block in (256, 1024, UNIT):
        assert plan.block_count(block) == wire.block_count(SIZES, block) == len(SM.split_table(_segs(plan), block))
    assert plan.block_count() == plan.n_units
    for bad in (64, 2048, 8192, 0, True):
        with pytest.raises(ValueError):
            plan.block_count(bad)


@pytest.mark.parametrize("segptr", [False, True], ids=["flat", "segptr"])
@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("block", BLOCKS)
def test_encode_and_decode(cuda, block, bits, delta, segptr):
    plan = _plan(bits)
    flat, base, bmn, bsc, stream, dec = _model(plan, block, delta)
    gmn, gsc, gstream = _encode(plan, block, flat, base, segptr)
    same_bits(gmn, bmn)
    same_bits(gsc, bsc)
    np.testing.assert_array_equal(gstream, stream)  # (the model's padding bits are zero: so are the kernel's)
    if not segptr:
        got, inside = _decode(plan, block, stream, bmn, bsc, base)
        same_bits(got[inside], dec[inside])


def _special(plan):
    """In the last segment (8192 + 1023 elements): NaN, +-Inf, denormals and -0.0 inside Gaussian blocks, a constant
    1024 elements (scale 0), an all-NaN 1024, 256 zeros of both signs; the 257-element segment all -0.0."""
    rng = np.random.default_rng(99)
    flat = _gauss(plan, 7).copy()
    off = int(_segs(plan)[-1, 0])
    x = rng.standard_normal(8192 + 1023).astype(np.float32)
    x[5::97] = np.nan
    x[7], x[11], x[300], x[1500] = np.inf, -np.inf, np.inf, -np.inf
    x[13:20] = np.array([1e-40, -1e-40, 1e-45, 0.0, -0.0, 3e-39, -2e-44], np.float32)
    x[2048:3072] = 7.5
    x[4096:5120] = np.nan
    x[5120:5376] = np.where(np.arange(256) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    x[8192:8192 + 256] = -3.25  # a constant row in the ragged unit
    flat[off:off + x.size] = x
    o257 = int(_segs(plan)[SIZES.index(257), 0])
    flat[o257:o257 + 257] = np.float32(-0.0)
    return flat


@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("block", BLOCKS)
def test_range_edge_cases(cuda, block, delta):
    plan = _plan(4)
    flat = _special(plan)
    base = None
    if delta:
        base = _gauss(plan, 100).copy()
        base[3::211] = np.float32(-0.0)
    bmn, bsc, _, stream = SM.encode(flat, _segs(plan), 4, block, base=base)
    assert (bsc == 0).any() and np.isnan(bmn).any()
    gmn, gsc, gstream = _encode(plan, block, flat, base)
    same_bits(gmn, bmn)
    same_bits(gsc, bsc)
    np.testing.assert_array_equal(gstream, stream)
    got, inside = _decode(plan, block, stream, bmn, bsc, base)
    same_bits(got[inside], SM.decode(stream, bmn, bsc, _segs(plan), 4, plan.span, block, base=base)[inside])


@pytest.mark.parametrize("block", BLOCKS)
def test_an_outlier_stays_in_its_block(cuda, block):
    plan = _plan(4)
    flat = _gauss(plan, 3)
    segs = _segs(plan)
    off, n = int(segs[-1, 0]), int(segs[-1, 1])
    hot = flat.copy()
    hot[off:off + n] = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    calm = hot.copy()
    e = 4096 + 2 * 256 + 17
    hot[off + e] = 1000.0
    (mn0, sc0, st0), (mn1, sc1, st1) = _encode(plan, block, calm, None), _encode(plan, block, hot, None)
    table = wire.block_table(segs[:, 1], block)  # (offsets in back-to-back element order = code order)
    first = int(segs[:-1, 1].sum())
    b = int(np.nonzero((table[:, 0] <= first + e) & (first + e < table[:, 0] + table[:, 1]))[0][0])
    keep = np.ones(len(table), dtype=bool)
    keep[b] = False
    same_bits(mn1[keep], mn0[keep])
    same_bits(sc1[keep], sc0[keep])
    assert sc1[b] > 50 * sc0[b]
    c0 = wire.unpack_dense_codes(st0, segs[:, 1], 4)
    c1 = wire.unpack_dense_codes(st1, segs[:, 1], 4)
    lo, ln = table[b].tolist()
    np.testing.assert_array_equal(np.delete(c1, np.s_[lo:lo + ln]), np.delete(c0, np.s_[lo:lo + ln]))
    assert (c1[lo:lo + ln] != c0[lo:lo + ln]).any()


@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("bits", [3, 4])
def test_block_4096_is_the_existing_path(cuda, bits, delta):
    plan = _plan(bits)
    flat = torch.from_numpy(_gauss(plan, 1)).cuda()
    base = torch.from_numpy(_gauss(plan, 100)).cuda() if delta else None
    old = plan.encode_block(flat=flat, base=base)
    new = plan.encode_block_g(UNIT, flat=flat, base=base)
    for a, b in zip(old, new):
        assert a.dtype == b.dtype and a.shape == b.shape
    same_bits(new[0].cpu().numpy(), old[0].cpu().numpy())
    same_bits(new[1].cpu().numpy(), old[1].cpu().numpy())
    np.testing.assert_array_equal(new[2].cpu().numpy(), old[2].cpu().numpy())
    same_bits(plan.decode_block_g(UNIT, *[old[i] for i in (2, 0, 1)], base=base).cpu().numpy(),
              plan.decode_block(*[old[i] for i in (2, 0, 1)], base=base).cpu().numpy())
    w = [2, 1]
    same_bits(plan.aggregate_dense_g(UNIT, [old[2]] * 2, [old[0]] * 2, [old[1]] * 2, w, base=base).cpu().numpy(),
              plan.aggregate_dense([old[2]] * 2, [old[0]] * 2, [old[1]] * 2, w, base=base, kind="block").cpu().numpy())


AGG_CASES = [(1, "sum", False, False, 4), (3, "div", True, True, 3), (5, "recip", False, True, 4),
             (5, "div", True, False, 5), (3, "recip", False, False, 8), (5, "sum", True, True, 1)]


@pytest.mark.parametrize("clients,mode,mask,delta,bits", AGG_CASES)
@pytest.mark.parametrize("block", BLOCKS)
def test_aggregate(cuda, block, clients, mode, mask, delta, bits):
    """1, 3 and 5 uploads (AGD_DEPTH is 4: one chunk, a partial chunk, two chunks) against the model and against
    decode_block_g of every upload followed by torch's weighted sum and division."""
    plan = _plan(bits)
    ups = [_model(plan, block, False, seed=10 + c) for c in range(clients)]
    weights = [3, 1, 4, 1, 5][:clients]
    total = float(sum(weights))
    base = _gauss(plan, 100) if delta else None
    avg_mask = [i % 3 != 1 for i in range(len(SIZES))] if mask else None
    dev = [[torch.from_numpy(u[i].copy()).cuda() for u in ups] for i in (4, 2, 3)]  # streams, bmn, bscale
    dbase = None if base is None else torch.from_numpy(base).cuda()
    out = torch.full((plan.span + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    got = plan.aggregate_dense_g(block, *dev, weights, base=dbase, out=out, mode=mode, avg_mask=avg_mask)
    assert got.data_ptr() == out.data_ptr()
    got, inside = out.cpu().numpy(), _inside(plan)
    assert (got[:plan.span][~inside] == SENTINEL).all() and (got[plan.span:] == SENTINEL).all()
    want = SM.aggregate([u[4] for u in ups], [u[2] for u in ups], [u[3] for u in ups], _segs(plan), bits, block, weights,
                        total, mode, plan.span, base=base, avg_mask=avg_mask)
    same_bits(got[:plan.span][inside], want[inside])
    # ... and the composition it replaces (torch's division by a scalar: a reciprocal multiply on the GPU, a division
    # on the CPU); a segment the mask leaves out keeps upload 0's decoded value
    dec = [plan.decode_block_g(block, s, m, c, base=dbase) for s, m, c in zip(*dev)]
    if mode == "div":
        dec = [d.cpu() for d in dec]
    acc = dec[0] * weights[0]
    for d, w in zip(dec[1:], weights[1:]):
        acc += d * w
    comp = (acc if mode == "sum" else torch.div(acc, total)).cpu().numpy()
    first = dec[0].cpu().numpy()
    for (off, n, _, _), m in zip(_segs(plan).tolist(), avg_mask or [True] * len(SIZES)):
        same_bits(got[off:off + n], comp[off:off + n] if m else first[off:off + n])


@pytest.mark.parametrize("block", BLOCKS)
def test_more_units_than_one_pass_of_the_device(cuda, block):
    """A segment of 1100 units and a ragged tail: more blocks of 256 threads (one per four units) than the device has
    CUs, unit and block indices past 1024 / 4096. A decode kernel with a per-lane unit index went wrong exactly from
    the 1025th unit on at G = 1024; the sizes of the other tests do not reach it."""
    plan = CodecPlan([1100 * UNIT + 300 + 3], 1.0, 4)
    segs = _segs(plan)
    flat = np.random.default_rng(8).uniform(-0.02, 0.02, plan.span).astype(np.float32)
    bmn, bsc, _, stream = SM.encode(flat, segs, 4, block)
    gmn, gsc, gstream = _encode(plan, block, flat, None)
    same_bits(gmn, bmn)
    same_bits(gsc, bsc)
    np.testing.assert_array_equal(gstream, stream)
    want = SM.decode(stream, bmn, bsc, segs, 4, plan.span, block)
    got, inside = _decode(plan, block, stream, bmn, bsc, None)
    same_bits(got[inside], want[inside])
    dev = [[torch.from_numpy(a.copy()).cuda()] for a in (stream, bmn, bsc)]
    agg = plan.aggregate_dense_g(block, *dev, [1], mode="sum").cpu().numpy()  # (-0.0 + x * 1.0 is x itself)
    same_bits(agg[:plan.span][inside], want[inside])


def test_xcd_unit_order(cuda):
    """A plan of LATENCY_PLAN_UNITS + 1 units, just past the launch code's threshold (coalac.hip: decode_latency is
    n_units <= LATENCY_PLAN_UNITS): the three kernels walk the units in the XCD-aware order."""
    sizes = [300] * (LATENCY_PLAN_UNITS - 3) + [4097, 1025, 1]
    plan = CodecPlan(sizes, 1.0, 4)
    assert plan.n_units == LATENCY_PLAN_UNITS + 1
    flat = _gauss(plan, 21)
    segs = _segs(plan)
    bmn, bsc, _, stream = SM.encode(flat, segs, 4, 256)
    gmn, gsc, gstream = _encode(plan, 256, flat, None)
    same_bits(gmn, bmn)
    same_bits(gsc, bsc)
    np.testing.assert_array_equal(gstream, stream)
    want = SM.decode(stream, bmn, bsc, segs, 4, plan.span, 256)
    got, inside = _decode(plan, 256, stream, bmn, bsc, None)
    same_bits(got[inside], want[inside])
    # one upload of weight 1, mode sum: -0.0 + x * 1.0 is x itself
    dev = [[torch.from_numpy(a.copy()).cuda()] for a in (stream, bmn, bsc)]
    agg = plan.aggregate_dense_g(256, *dev, [1], mode="sum").cpu().numpy()
    same_bits(agg[:plan.span][inside], want[inside])


def test_round_end_to_end(cuda):
    """A client / server round through the mixins: a block-wise download with 1024-element blocks, delta uploads with
    256-element blocks, and the fused dense aggregate — against the same server with the dense kernel switched off
    (decode_module of every upload + FedAvg) and, for the download, against the model."""
    seen = {}

    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode = 1.0, 4, "delta"
        codec_blockwise, codec_block_size = True, 256

    def server(dense, clients):
        class Server(CompressionServerMixin, LoopbackServer):
            codec_ratio, codec_bits, codec_mode = 1.0, 4, "delta"
            codec_fused_aggregate = True
            codec_fused_dense_aggregate = dense
            codec_download, codec_download_bits = True, 4
            codec_download_blockwise, codec_download_block_size = True, 1024

            def compression(self):
                super().compression()
                seen.setdefault("sent", []).append(self.model)
                seen.setdefault("global", []).append(copy.deepcopy(self._real_global().state_dict()))

            def aggregate(self, models, weights):
                seen.setdefault("uploads", []).append(list(models))
                return super().aggregate(models, weights)
        return Server(build_module("lenet", seed=7).cuda(), clients, remote=True)

    def clients():
        return [Client(f"c{i}", 5 + i, device="cuda", step_seed=i) for i in range(3)]
    on, off = server(True, clients()), server(False, clients())
    plan_calls = []
    inner = CodecPlan.aggregate_dense_g
    CodecPlan.aggregate_dense_g = lambda self, block, *a, **k: (plan_calls.append(block), inner(self, block, *a, **k))[1]
    try:
        on.round(0)
    finally:
        CodecPlan.aggregate_dense_g = inner
    assert plan_calls == [256]  # the fused aggregate took the 256-element kernel, once
    carrier, ups = seen["sent"][0], seen["uploads"][0]
    assert isinstance(carrier, CompressedModel) and carrier.update.header["blockwise"] == 1024
    h = carrier.update.header
    sizes = [e["n"] for e in h["entries"] if e["kind"] == "seg"]
    assert h["n_blocks"] == wire.block_count(sizes, 1024)
    assert carrier.nbytes == 8 * h["n_blocks"] + 4 * wire.dense_packed_words(sizes, 4) + carrier.update.raw.nbytes
    # the download: what every client decoded is the model's decode of the global the server compressed
    plan = on._codec().dense_aggregate_plan(ups[0].header)
    segs = plan.table.segs.astype(np.int64)
    flat = np.zeros(plan.span, np.float32)
    for e in h["entries"]:
        if e["kind"] == "seg":
            flat[e["off"]:e["off"] + e["n"]] = seen["global"][0][e["name"]].cpu().numpy().reshape(-1)
    mn, sc, _, stream = SM.encode(flat, segs, 4, 1024)
    want = SM.decode(stream, mn, sc, segs, 4, plan.span, 1024)
    _, gmn, gsc, _, _, _, _ = wire.unpack(carrier.update.to_bytes())
    same_bits(gmn, mn)
    same_bits(gsc, sc)
    np.testing.assert_array_equal(carrier.update.packed.cpu().numpy(), stream)
    got = pickle.loads(pickle.dumps(carrier)).bind(on._codec().backend).state_dict()
    for e in h["entries"]:
        if e["kind"] == "seg":
            same_bits(got[e["name"]].cpu().numpy().reshape(-1), want[e["off"]:e["off"] + e["n"]])
    # the uploads name their size and count their longer range sections
    for u in ups:
        assert u.header["blockwise"] == 256 and u.header["n_blocks"] == wire.block_count(sizes, 256)
        assert u.nbytes == 8 * u.header["n_blocks"] + 4 * wire.dense_packed_words(sizes, 4) + u.raw.nbytes
    # the fused round gives what decoding upload by upload gives (the same round on the server without the dense kernel)
    off.round(0)
    for (k, a), b in zip(on.model.state_dict().items(), off.model.state_dict().values()):
        assert a.dtype == b.dtype
        if a.dtype == torch.float32:
            same_bits(a.cpu().numpy().reshape(-1), b.cpu().numpy().reshape(-1))
        else:
            assert torch.equal(a, b), k
