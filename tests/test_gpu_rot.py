"""The rotated block-wise kernels (k_dense_block_quant_rot / k_dense_deq_stream_rot) against the CPU
model (tests/rot_model.py) through CodecPlan. Every comparison is bit-exact; a NaN compares as NaN (its sign and payload
are not part of the contract). One plan interleaves rotated (full) and unrotated (ragged) units."""
import copy
import struct

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, CompressedModel, CompressionClientMixin, CompressionServerMixin
from coala_amd.fl import LoopbackClient, LoopbackServer
from coala_amd.layouts import build_module
from tests import rot_model as RM

pytestmark = pytest.mark.gpu

UNIT = 4096
SIZES = [0, 1, 255, 4095, 4096, 4097, 8192, 8192 + 1023, 3 * 4096]
BITS = [1, 3, 4, 5, 8]  # (3 and 5: a lane's field straddles two words)
LATENCY_PLAN_UNITS = 8192  # coalac.hip: a plan with more units takes the XCD-aware unit order
PAD = 64
SENTINEL = 123.25
ROT, SR = 0x0123456789ABCDEF, 0xFEDCBA9876543210
_PLANS, _INPUTS, _MODEL = {}, {}, {}


def _plan(bits):
    if bits not in _PLANS:
        _PLANS[bits] = CodecPlan(SIZES, 1.0, bits)
    return _PLANS[bits]


def _segs(plan):
    return plan.table.segs.astype(np.int64)


def _heavy(plan, seed):
    """Student-t(3) values, each segment at a scale of its own."""
    key = (plan.span, seed)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        flat = np.zeros(plan.span, np.float32)
        for off, n, _, _ in _segs(plan).tolist():
            flat[off:off + n] = (rng.standard_t(3, n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
        _INPUTS[key] = flat
    return _INPUTS[key]


def _inside(plan):
    m = np.zeros(plan.span, dtype=bool)
    for off, n, _, _ in _segs(plan).tolist():
        m[off:off + n] = True
    return m


def _model(plan, delta, sr, seed=1):
    """(flat, base, bmn, bscale, stream, decoded) of the heavy-tailed input, once per (bits, delta, sr, seed)."""
    key = (plan.bits, delta, sr, seed)
    if key not in _MODEL:
        flat = _heavy(plan, seed)
        base = _heavy(plan, 100) if delta else None
        bmn, bsc, _, stream = RM.encode(flat, _segs(plan), plan.bits, ROT, seed=SR if sr else None, base=base)
        dec = RM.decode(stream, bmn, bsc, _segs(plan), plan.bits, plan.span, ROT, base=base)
        _MODEL[key] = (flat, base, bmn, bsc, stream, dec)
    return _MODEL[key]


def _encode(plan, flat, base, segptr=False, rot_seed=ROT, seed=None):
    """encode_block_rot into canaried buffers -> (bmn, bscale, stream) on the host; nothing outside them is written."""
    U, P = plan.n_units, plan.dense_packed_words
    rbuf = torch.full((2, PAD + U + PAD), SENTINEL, dtype=torch.float32, device="cuda")
    obuf = torch.full((16 + P + 64,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    out = (rbuf[0, PAD:PAD + U], rbuf[1, PAD:PAD + U], obuf[16:])
    dbase = None if base is None else torch.from_numpy(base).cuda()
    if segptr:
        tensors = [torch.from_numpy(flat[off:off + n].copy()).cuda() for off, n, _, _ in _segs(plan).tolist()]
        plan.encode_block_rot(tensors=tensors, base=dbase, rot_seed=rot_seed, seed=seed, out=out)
    else:
        plan.encode_block_rot(flat=torch.from_numpy(flat).cuda(), base=dbase, rot_seed=rot_seed, seed=seed, out=out)
    torch.cuda.synchronize()
    r, o = rbuf.cpu().numpy(), obuf.cpu().numpy()
    assert (r[:, :PAD] == SENTINEL).all() and (r[:, PAD + U:] == SENTINEL).all()
    assert (o[:16] == 0xFFFFFFFF).all() and (o[16 + P:] == 0xFFFFFFFF).all()
    return r[0, PAD:PAD + U], r[1, PAD:PAD + U], o[16:16 + P]


def _decode(plan, stream, bmn, bsc, base, rot_seed=ROT):
    out = torch.full((plan.span + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    dbase = None if base is None else torch.from_numpy(base).cuda()
    plan.decode_block_rot(torch.from_numpy(stream.copy()).cuda(), torch.from_numpy(bmn.copy()).cuda(),
                          torch.from_numpy(bsc.copy()).cuda(), rot_seed, base=dbase, out=out)
    got, inside = out.cpu().numpy(), _inside(plan)
    assert (got[:plan.span][~inside] == SENTINEL).all() and (got[plan.span:] == SENTINEL).all()
    return got[:plan.span], inside


def _check(plan, flat, base, want, sr=False, segptr=False):
    bmn, bsc, stream, dec = want
    gmn, gsc, gstream = _encode(plan, flat, base, segptr, seed=SR if sr else None)
    assert RM.same_bits(gmn, bmn) and RM.same_bits(gsc, bsc)
    np.testing.assert_array_equal(gstream, stream)  # (the model's padding bits are zero: so are the kernel's)
    got, inside = _decode(plan, stream, bmn, bsc, base)
    assert RM.same_bits(got[inside], dec[inside])
    return got, inside


@pytest.mark.parametrize("segptr", [False, True], ids=["flat", "segptr"])
@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("sr", [False, True], ids=["rn", "sr"])
@pytest.mark.parametrize("bits", BITS)
def test_encode_and_decode(cuda, bits, sr, delta, segptr):
    plan = _plan(bits)
    assert plan.has_block_rot
    flat, base, *want = _model(plan, delta, sr)
    _check(plan, flat, base, want, sr, segptr)


@pytest.mark.parametrize("bits", [3, 4])
def test_stochastic_seeds(cuda, bits):
    plan = _plan(bits)
    flat = _heavy(plan, 1)
    a, b = _encode(plan, flat, None, seed=SR), _encode(plan, flat, None, seed=SR)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))  # the same seed pair: the same payload
    c = _encode(plan, flat, None, seed=SR + 1)
    assert RM.same_bits(c[0], a[0]) and RM.same_bits(c[1], a[1]) and (c[2] != a[2]).any()  # the ranges stay
    rn = _encode(plan, flat, None)
    assert RM.same_bits(rn[0], a[0]) and RM.same_bits(rn[1], a[1])
    d = _encode(plan, flat, None, rot_seed=ROT + 1)  # another rotation: other coefficients
    assert (d[2] != rn[2]).any() and not RM.same_bits(d[0], rn[0])


def test_a_plan_of_ragged_units_is_encode_block(cuda):
    plan = CodecPlan([1, 255, 4095, 300, 2000], 1.0, 4)
    flat = torch.from_numpy(_heavy(plan, 3)).cuda()
    base = torch.from_numpy(_heavy(plan, 100)).cuda()
    for b in (None, base):
        for seed, old in ((None, plan.encode_block(flat=flat, base=b)), (SR, plan.encode_block_sr(flat=flat, base=b, seed=SR))):
            new = plan.encode_block_rot(flat=flat, base=b, rot_seed=ROT, seed=seed)
            for x, y in zip(old, new):
                assert x.dtype == y.dtype and x.shape == y.shape
                np.testing.assert_array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
        old = plan.encode_block(flat=flat, base=b)
        got = plan.decode_block_rot(old[2], old[0], old[1], ROT, base=b).cpu().numpy()
        want = plan.decode_block(old[2], old[0], old[1], base=b).cpu().numpy()
        inside = _inside(plan)
        assert RM.same_bits(got[inside], want[inside])


def _special(plan):
    """Full units of the 3 x 4096 and 8192 segments made special — constant, all zero, all -0.0, one NaN, +Inf and -Inf,
    all NaN — beside ordinary units; the ragged tail of 8192 + 1023 holds a NaN too."""
    flat = _heavy(plan, 7).copy()
    segs = _segs(plan)
    o3, o2, or_ = (int(segs[SIZES.index(n), 0]) for n in (3 * 4096, 8192, 8192 + 1023))
    flat[o3:o3 + UNIT] = 7.5
    flat[o3 + UNIT:o3 + 2 * UNIT] = 0.0
    flat[o3 + 2 * UNIT:o3 + 3 * UNIT] = np.float32(-0.0)
    flat[o2 + 17] = np.nan
    flat[o2 + UNIT + 5], flat[o2 + UNIT + 900] = np.inf, -np.inf
    flat[or_:or_ + UNIT] = np.nan
    flat[or_ + 2 * UNIT + 3] = np.nan
    return flat


@pytest.mark.parametrize("sr", [False, True], ids=["rn", "sr"])
@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
def test_special_units(cuda, delta, sr):
    plan = _plan(4)
    flat = _special(plan)
    base = None
    if delta:
        base = _heavy(plan, 100).copy()
        base[3::211] = np.float32(-0.0)
    segs = _segs(plan)
    bmn, bsc, _, stream = RM.encode(flat, segs, 4, ROT, seed=SR if sr else None, base=base)
    dec = RM.decode(stream, bmn, bsc, segs, 4, plan.span, ROT, base=base)
    assert np.isnan(bmn).any() and (delta or (bsc == 0).any())
    _check(plan, flat, base, (bmn, bsc, stream, dec), sr)
    # the ordinary units are untouched: their ranges and codes are those of the input without the special values
    calm = _heavy(plan, 7)
    cmn, csc, _, cstream = RM.encode(calm, segs, 4, ROT, seed=SR if sr else None, base=base)
    rows = RM.unit_rows(segs)
    same = np.array([np.array_equal(flat[o:o + n].view(np.uint32), calm[o:o + n].view(np.uint32)) for o, n in rows.tolist()])
    assert same.sum() == len(rows) - 7
    assert RM.same_bits(bmn[same], cmn[same]) and RM.same_bits(bsc[same], csc[same])


@pytest.mark.parametrize("bits", [1, 4, 8])
def test_round_trip_error_is_within_a_step_of_the_coefficients(cuda, bits):
    """decode(encode(x)) - x is the rotated quantisation error of the coefficients: per unit its RMS is at most half a
    step of the unit's own range (round to nearest), plus the transform's fp32 rounding — 12 stages of relative 2^-24
    each way on values up to the unit's largest |coefficient| — bounded here by one whole step, from the model's bscale."""
    plan = _plan(bits)
    flat, _, bmn, bsc, stream, _ = _model(plan, False, False)
    gmn, gsc, gstream = _encode(plan, flat, None)
    got, inside = _decode(plan, gstream, gmn, gsc, None)
    for (off, n), step in zip(RM.unit_rows(_segs(plan)).tolist(), bsc.tolist()):
        err = got[off:off + n].astype(np.float64) - flat[off:off + n]
        assert np.sqrt(np.mean(err ** 2)) <= step, (off, n)


def test_more_units_than_one_pass_of_the_device(cuda):
    """A segment of 1100 full units and a ragged tail: more blocks of 256 threads (one per four units) than the device
    has CUs, unit indices past 1024 (DESIGN.md §20 records a decode that went wrong from there on)."""
    plan = CodecPlan([1100 * UNIT + 300 + 3], 1.0, 4)
    segs = _segs(plan)
    flat = np.random.default_rng(8).standard_t(3, plan.span).astype(np.float32)
    bmn, bsc, _, stream = RM.encode(flat, segs, 4, ROT)
    dec = RM.decode(stream, bmn, bsc, segs, 4, plan.span, ROT)
    _check(plan, flat, None, (bmn, bsc, stream, dec))


def test_xcd_unit_order(cuda):
    """A plan of LATENCY_PLAN_UNITS + 1 units, just past the launch code's threshold: the kernels walk the units in the
    XCD-aware order (the other instantiation)."""
    sizes = [300] * (LATENCY_PLAN_UNITS - 4) + [2 * UNIT + 1, UNIT, 1]
    plan = CodecPlan(sizes, 1.0, 4)
    assert plan.n_units == LATENCY_PLAN_UNITS + 1
    flat, segs = _heavy(plan, 21), _segs(plan)
    for sr in (False, True):
        bmn, bsc, _, stream = RM.encode(flat, segs, 4, ROT, seed=SR if sr else None)
        dec = RM.decode(stream, bmn, bsc, segs, 4, plan.span, ROT)
        _check(plan, flat, None, (bmn, bsc, stream, dec), sr)


def test_round_end_to_end(cuda):
    """A client / server round through the mixins on the HIP backend: a rotated download and rotated delta uploads,
    decoded upload by upload — the download against the model, the uploads' headers and version word."""
    seen = {}

    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode = 1.0, 4, "delta"
        codec_blockwise = codec_rotate = True

    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode = 1.0, 4, "delta"
        codec_fused_aggregate = codec_fused_dense_aggregate = True
        codec_download, codec_download_bits = True, 4
        codec_download_blockwise = codec_download_rotate = True
        codec_download_rotate_seed = 17

        def compression(self):
            super().compression()
            seen.setdefault("sent", []).append(self.model)
            seen.setdefault("global", []).append(copy.deepcopy(self._real_global().state_dict()))

        def aggregate(self, models, weights):
            seen.setdefault("uploads", []).append(list(models))
            return super().aggregate(models, weights)

    clients = [Client(f"c{i}", 5 + i, device="cuda", step_seed=i) for i in range(2)]
    server = Server(build_module("lenet", seed=7).cuda(), clients, remote=True)
    server.round(0)
    carrier, ups = seen["sent"][0], seen["uploads"][0]
    assert isinstance(carrier, CompressedModel)
    h = carrier.update.header
    assert h["blockwise"] == UNIT and struct.unpack_from("<I", carrier.update.to_bytes(), 8)[0] == 6
    sizes = [e["n"] for e in h["entries"] if e["kind"] == "seg"]
    plan = CodecPlan(sizes, 1.0, 4)
    segs = _segs(plan)
    flat = np.zeros(plan.span, np.float32)
    for e in h["entries"]:
        if e["kind"] == "seg":
            flat[e["off"]:e["off"] + e["n"]] = seen["global"][0][e["name"]].cpu().numpy().reshape(-1)
    mn, sc, _, stream = RM.encode(flat, segs, 4, h["rotate"])
    want = RM.decode(stream, mn, sc, segs, 4, plan.span, h["rotate"])
    np.testing.assert_array_equal(carrier.update.packed.cpu().numpy(), stream)
    for c in clients:  # what each client decoded
        got = c._codec_base.flat.cpu().numpy()[:plan.span]
        assert RM.same_bits(got[_inside(plan)], want[_inside(plan)])
    assert len({u.header["rotate"] for u in ups}) == len(ups)
    for u in ups:
        assert u.header["blockwise"] == UNIT and struct.unpack_from("<I", u.to_bytes(), 8)[0] == 6
    for v in server.model.state_dict().values():
        assert bool(torch.isfinite(v.float()).all())
