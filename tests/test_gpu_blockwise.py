"""The block-wise dense kernels (k_dense_block_quant / k_dense_deq_stream) against the split-table model
(tests/blockwise_model.py): the existing oracle run over a segment table in which every segment has been cut into its
4096-element blocks, the stream in wire v4's layout. Every comparison is bit-exact (a NaN range compares as NaN: its
payload is not part of the spec). Shapes as tests/test_gpu_dense_pack.py: one instantiation per code width, full and
partial units, segments shorter than a word's worth of codes, an empty segment, batched and explicit-row plans."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, CompressionServerMixin, UpdateCodec, _lib, wire
from coala_amd.fl import LoopbackServer
from coala_amd.fl.strategies import federated_averaging
from coala_amd.layouts import build_module
from tests import blockwise_model as BM
from tests.blockwise_model import BlockOracleBackend

pytestmark = pytest.mark.gpu

UNIT = 4096
SIZES = [1, 31, 32, 33, 4095, 4096, 4097, 2 * 4096 + 5]
ROWS = [(0, 33, 33, 5), (64, 4097, 4097, 101), (8192, 70, 70, 4300)]  # explicit k == n rows, odd out_off
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
            p = CodecPlan(SIZES[:4] + [0] + SIZES[4:], 1.0, bits)
        elif kind == "batched":
            p = CodecPlan([33, 4097, 70], 1.0, bits, clients=3)
        elif kind == "special":
            p = CodecPlan([3 * UNIT + 100, 33], 1.0, bits)
        else:
            p = CodecPlan.from_segments(np.array(ROWS, dtype=np.uint64), bits)
        _PLANS[key] = p
    return _PLANS[key]


def _gauss(plan, seed):
    rng = np.random.default_rng(seed)
    flat = np.zeros(plan.span, np.float32)
    for off, n, _, _ in plan.table.segs.astype(np.int64).tolist():
        flat[off:off + n] = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
    return flat


def _special(plan):
    """NaN, +-inf, denormals, +-0 inside a Gaussian block; a constant block (scale 0); an all-NaN block; a block of
    zeros of both signs; a segment of denormals."""
    rng = np.random.default_rng(99)
    flat = np.zeros(plan.span, np.float32)
    x = rng.standard_normal(3 * UNIT + 100).astype(np.float32)
    x[5::97] = np.nan
    x[7] = np.inf
    x[11] = -np.inf
    x[13:20] = np.array([1e-40, -1e-40, 1e-45, 0.0, -0.0, 3e-39, -2e-44], np.float32)
    x[UNIT:2 * UNIT] = 7.5
    x[2 * UNIT:3 * UNIT] = np.nan
    x[3 * UNIT:] = np.where(np.arange(100) % 2 == 0, np.float32(-0.0), np.float32(0.0))
    flat[:x.size] = x
    off = int(plan.table.segs[1, 0])
    flat[off:off + 33] = (rng.standard_normal(33) * 1e-40).astype(np.float32)
    return flat


def _same_ranges(got, want):
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def _encode_and_check(plan, flat, base, segptr):
    segs = plan.table.segs.astype(np.int64)
    U, P = plan.n_units, plan.dense_packed_words
    assert U == len(BM.split_table(segs)) and P == wire.dense_packed_words(segs[:, 1], plan.bits)
    bmn, bsc, _, stream = BM.encode(flat, segs, plan.bits, base=base)
    rbuf = torch.full((2, PAD + U + PAD), SENTINEL, dtype=torch.float32, device="cuda")
    obuf = torch.full((16 + P + 64,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    out = (rbuf[0, PAD:PAD + U], rbuf[1, PAD:PAD + U], obuf[16:])
    dbase = None if base is None else torch.from_numpy(base).cuda()
    if segptr:
        tensors = [torch.from_numpy(flat[off:off + n].copy()).cuda() for off, n, _, _ in segs.tolist()]
        plan.encode_block(tensors=tensors, base=dbase, out=out)
    else:
        plan.encode_block(flat=torch.from_numpy(flat).cuda(), base=dbase, out=out)
    torch.cuda.synchronize()
    r, o = rbuf.cpu().numpy(), obuf.cpu().numpy()
    _same_ranges(r[0, PAD:PAD + U], bmn)
    _same_ranges(r[1, PAD:PAD + U], bsc)
    np.testing.assert_array_equal(o[16:16 + P], stream)  # (the model's padding bits are zero: so are the kernel's)
    assert (r[:, :PAD] == SENTINEL).all() and (r[:, PAD + U:] == SENTINEL).all()
    assert (o[:16] == 0xFFFFFFFF).all() and (o[16 + P:] == 0xFFFFFFFF).all()
    return bmn, bsc, stream


@pytest.mark.parametrize("segptr", [False, True], ids=["flat", "segptr"])
@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("bits", range(1, 9))
@pytest.mark.parametrize("kind", KINDS)
def test_encode_block(cuda, kind, bits, delta, segptr):
    plan = _plan(kind, bits)
    assert plan.dense
    flat = _gauss(plan, bits)
    base = _gauss(plan, 100 + bits) if delta else None
    _encode_and_check(plan, flat, base, segptr)


@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("bits", [1, 3, 4, 8])
def test_encode_block_special_values(cuda, bits, delta):
    plan = _plan("special", bits)
    flat = _special(plan)
    base = None
    if delta:
        base = _gauss(plan, 7)
        base[::9] = -0.0
    bmn, bsc, _ = _encode_and_check(plan, flat, base, False)
    if not delta:
        assert bsc[1] == 0 and bmn[1] == 7.5 and np.isnan(bmn[2]) and np.isnan(bsc[2])
        assert bmn[3].view(np.uint32) == 0 and bsc[3] == 0  # min(-0, +0) + 0.0f = +0


@pytest.mark.parametrize("bits", [4, 8])
def test_block_quantise_near_code_boundaries(cuda, bits):
    """tests/test_gpu_parity.py test_dense_quantise_near_code_boundaries' inputs, each as one 4096-element block: the
    reciprocal quantise k_dense_block_quant shares with k_dense_quant, against the oracle's IEEE division."""
    rng = np.random.default_rng(40 + bits)
    levels = (1 << bits) - 1
    blocks = []
    for mant in (0x7FFFFF, 0x0, 0x7FFF00, 0x3A5A5A, int(rng.integers(0, 1 << 23))):
        for e in (-100, -80, -20, -3, 0, 7, 60, 95):  # (-100, 95: outside [2^-90, 2^90], the division)
            sc = np.array([((127 + e) << 23) | mant], np.uint32).view(np.float32)[0]
            mn = np.float32(rng.standard_normal()) * np.float32(2.0 ** e)
            mx = np.float32(mn + np.float32(levels) * sc)
            sc = np.float32((mx - mn) / np.float32(levels))
            m = UNIT - 2
            ks = rng.integers(0, levels, m).astype(np.float32)
            near = np.where(rng.random(m) < 0.5, (ks + np.float32(0.5)) * sc, ks * sc).astype(np.float32)
            x = (mn + near).astype(np.float32)
            x = (x.view(np.int32) + rng.integers(-3, 4, m).astype(np.int32)).view(np.float32)
            x = np.clip(x, mn, mx).astype(np.float32)
            blocks.append(np.concatenate([[mn, mx], x]).astype(np.float32))
    plan = CodecPlan([UNIT * len(blocks)], 1.0, bits)
    assert plan.n_units == len(blocks)
    flat = np.zeros(plan.span, np.float32)
    flat[:UNIT * len(blocks)] = np.concatenate(blocks)
    _encode_and_check(plan, flat, None, False)


@pytest.mark.parametrize("base_kind", [None, "random", "special"])
@pytest.mark.parametrize("bits", range(1, 9))
@pytest.mark.parametrize("kind", KINDS)
def test_decode_block(cuda, kind, bits, base_kind):
    plan = _plan(kind, bits)
    segs = plan.table.segs.astype(np.int64)
    flat = _gauss(plan, 20 + bits)
    mn, sc, _, stream = BM.encode(flat, segs, bits)
    rng = np.random.default_rng(bits)
    base = None
    if base_kind is not None:
        base = rng.standard_normal(plan.span).astype(np.float32)
        if base_kind == "special":
            base[::5] = -0.0
            base[1::7] = np.float32(np.nan)
    ref = np.full(plan.span, SENTINEL, dtype=np.float32)
    inside = np.zeros(plan.span, dtype=bool)
    for off, n, _, _ in segs.tolist():
        inside[off:off + n] = True
    dec = BM.decode(stream, mn, sc, segs, bits, plan.span, base=base)
    ref[inside] = dec[inside]
    dirty = stream.copy()  # padding bits of a received stream are ignored
    W = (segs[:, 1] * bits + 31) // 32
    for n, w, p in zip(segs[:, 1], W, np.cumsum(W) - W):
        if w and (n * bits) % 32:
            dirty[p + w - 1] |= np.uint32((0xFFFFFFFF << int((n * bits) % 32)) & 0xFFFFFFFF)
    d = lambda a: None if a is None else torch.from_numpy(a).cuda()
    for words in (stream, dirty):
        out = torch.full((plan.span + 64,), SENTINEL, dtype=torch.float32, device="cuda")
        plan.decode_block(d(words), d(mn), d(sc), base=d(base), out=out)
        got = out.cpu().numpy()
        nan = np.isnan(ref)
        np.testing.assert_array_equal(np.isnan(got[:plan.span]), nan)
        np.testing.assert_array_equal(got[:plan.span][~nan].view(np.uint32), ref[~nan].view(np.uint32))
        assert (got[plan.span:] == SENTINEL).all() and (got[:plan.span][~inside] == SENTINEL).all()


def test_batch_plan_reaches_the_xcd_unit_order(cuda):
    """More than 8192 units: both kernels take the XCD-aware unit order. Encode, then decode, block by block against
    the model."""
    n, clients, bits = 40960 + 3, 900, 4
    plan = CodecPlan([n], 1.0, bits, clients=clients)
    assert plan.n_units == 11 * clients > 8192
    segs = plan.table.segs.astype(np.int64)
    rng = np.random.default_rng(5)
    flat = rng.standard_normal(plan.span, dtype=np.float32)
    flat *= np.repeat(10.0 ** rng.uniform(-3, 1, (plan.span + 511) // 512), 512)[:plan.span].astype(np.float32)
    mn, sc, _, stream = BM.encode(flat, segs, bits)
    dflat = torch.from_numpy(flat).cuda()
    bmn, bsc, packed = plan.encode_block(flat=dflat)
    out = plan.decode_block(packed, bmn, bsc, out=torch.full((plan.span,), SENTINEL, device="cuda"))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(bmn.cpu().numpy().view(np.uint32), mn.view(np.uint32))
    np.testing.assert_array_equal(bsc.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    np.testing.assert_array_equal(packed.cpu().numpy(), stream)
    ref = BM.decode(stream, mn, sc, segs, bits, plan.span, out=np.full(plan.span, SENTINEL, np.float32))
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_abi_errors(cuda):
    lib = _lib.load()
    plan = _plan("plain", 4)
    sparse = CodecPlan([5000, 300], 0.1, 4)
    raw = CodecPlan([64, 8], 1.0, 32)
    empty = CodecPlan([0, 0], 1.0, 4)
    U, P = plan.n_units, plan.dense_packed_words
    x = torch.from_numpy(_gauss(plan, 1)).cuda()
    ptrs = plan.segment_pointers([x[o:o + n] for o, n, _, _ in plan.table.segs.astype(np.int64).tolist()])
    bmn = torch.full((U + 4,), SENTINEL, device="cuda")
    bsc = torch.full((U + 4,), SENTINEL, device="cuda")
    packed = torch.full((P + 4,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    out = torch.full((plan.span,), SENTINEL, device="cuda")
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    N = ctypes.c_void_p(0)
    nbytes, short = ctypes.c_uint64(4 * P), ctypes.c_uint64(4 * P - 4)
    enc, dec = lib.coalac_encode_block, lib.coalac_decode_block
    good_enc = (plan._h, p(x), N, N, p(bmn), p(bsc), p(packed), nbytes, N)
    good_dec = (plan._h, p(packed), nbytes, p(bmn), p(bsc), N, p(out), N)

    def bad(fn, args, word, **change):
        a = list(args)
        for i, v in change.items():
            a[int(i[1:])] = v
        assert fn(*a) == -1, (fn.__name__, change)
        msg = lib.coalac_last_error()
        assert fn.__name__.encode() in msg and word in msg, msg

    bad(enc, good_enc, b"exactly one", a2=p(ptrs))            # both inputs
    bad(enc, good_enc, b"exactly one", a1=N)                   # neither
    bad(enc, good_enc, b"dense", a0=sparse._h)
    bad(enc, good_enc, b"32", a0=raw._h)
    for i in (4, 5, 6):
        bad(enc, good_enc, b"NULL", **{f"a{i}": N})
    bad(enc, good_enc, b"packed_bytes", a7=short)
    bad(enc, good_enc, b"aligned", a1=p(x, 4))
    bad(enc, good_enc, b"aligned", a3=p(x, 8))
    bad(enc, good_enc, b"aligned", a6=p(packed, 2))
    assert enc(None, *good_enc[1:]) == -1
    bad(dec, good_dec, b"dense", a0=sparse._h)
    bad(dec, good_dec, b"32", a0=raw._h)
    for i in (1, 3, 4, 6):
        bad(dec, good_dec, b"NULL", **{f"a{i}": N})
    bad(dec, good_dec, b"packed_bytes", a2=short)
    bad(dec, good_dec, b"aligned", a6=p(out, 4))
    bad(dec, good_dec, b"aligned", a5=p(x, 8))
    bad(dec, good_dec, b"aligned", a1=p(packed, 2))
    assert dec(None, *good_dec[1:]) == -1
    # an empty plan: OK, nothing launched
    assert enc(empty._h, p(x), N, N, p(bmn), p(bsc), p(packed), ctypes.c_uint64(0), N) == 0
    assert dec(empty._h, p(packed), ctypes.c_uint64(0), p(bmn), p(bsc), N, p(out), N) == 0
    torch.cuda.synchronize()  # nothing was launched: the buffers are what they were
    assert (bmn == SENTINEL).all() and (bsc == SENTINEL).all() and (out == SENTINEL).all()
    assert (packed.cpu().numpy() == 0xFFFFFFFF).all()
    # the typed wrappers check before any launch
    for wrong in (sparse, raw):
        with pytest.raises(ValueError):
            wrong.encode_block(flat=x)
        with pytest.raises(ValueError):
            wrong.decode_block(packed, bmn, bsc)
    for call in (lambda: plan.encode_block(), lambda: plan.encode_block(flat=x, tensors=[x]),
                 lambda: plan.encode_block(flat=x[:-8]), lambda: plan.encode_block(flat=x.cpu()),
                 lambda: plan.encode_block(flat=x, out=(bmn[:U - 1], bsc, packed)),
                 lambda: plan.encode_block(flat=x, out=(bmn, bsc, packed[:P - 1])),
                 lambda: plan.decode_block(packed[:P - 1], bmn, bsc), lambda: plan.decode_block(packed, bmn[:U - 1], bsc),
                 lambda: plan.decode_block(packed.view(torch.int32), bmn, bsc),
                 lambda: plan.decode_block(packed, bmn, bsc, out=out[:-40])):
        with pytest.raises(ValueError):
            call()
    assert enc(*good_enc) == 0 and dec(*good_dec) == 0
    torch.cuda.synchronize()
    assert (bmn[U:] == SENTINEL).all() and (packed[P:].cpu().numpy() == 0xFFFFFFFF).all()


def _i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("layout", ["lenet", "resnet18"])
def test_end_to_end_codec(cuda, layout):
    """encode -> to_bytes -> from_bytes -> encoded_to -> decode_state on the device: the blob is the model backend's,
    byte for byte, the receiver moves one mn ... packed region and decodes the stream to what the model decodes."""
    model = build_module(layout, seed=1)
    hip = UpdateCodec(1.0, 4, "weights", blockwise=True, recycle=False)
    ref = UpdateCodec(1.0, 4, "weights", backend=BlockOracleBackend(), blockwise=True)
    up = hip.encode_module(copy.deepcopy(model).cuda())
    assert up.header["blockwise"] == UNIT and up.packed.is_cuda and up.encoded.vals is None
    blob = up.to_bytes()
    want = ref.encode(model.state_dict())
    assert blob == want.to_bytes() and up.nbytes == want.nbytes
    own = hip.decode_state(up)  # the sender's own decode: the server's reconstruction of its download
    back = pickle.loads(pickle.dumps(up))
    staged = []
    inner = hip._staging
    hip._staging = lambda n: (staged.append(n), inner(n))[1]
    got = hip.decode_state(back)
    _, sec = wire.sections(blob)
    assert staged == [sec["packed"][0] + sec["packed"][1] - sec["mn"][0]]  # one pinned copy, the stream still packed
    enc = back.encoded_to(torch.device("cuda", 0), staging=inner)
    hip._staged(torch.cuda.current_stream())
    assert enc.vals is None and enc.packed.is_cuda and enc.packed.numel() == sec["packed"][1] // 4
    assert enc.mn.numel() == enc.scale.numel() == up.header["n_blocks"]
    oracle = ref.decode_state(pickle.loads(pickle.dumps(want)))
    assert list(got) == list(oracle) == list(own)
    for k in oracle:
        for mine in (got[k], own[k]):
            assert mine.dtype == oracle[k].dtype
            if mine.dtype == torch.float32:
                assert torch.equal(_i32(mine.cpu()), _i32(oracle[k])), k
            else:
                assert torch.equal(mine.cpu(), oracle[k]), k


def test_server_round_of_blockwise_uploads_is_decoded_per_upload(cuda):
    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode = 1.0, 4, "weights"
        codec_fused_aggregate = True

    g = build_module("lenet", seed=5)
    mods = [build_module("lenet", seed=s) for s in (1, 2, 3)]
    hip = UpdateCodec(1.0, 4, "weights", blockwise=True)
    ups = [pickle.loads(pickle.dumps(hip.encode_module(copy.deepcopy(m).cuda()))) for m in mods]
    server = Server(copy.deepcopy(g).cuda(), [])
    assert all(server.decompression(u) is u for u in ups)  # fused mode keeps the carriers for aggregate()
    with pytest.raises(ValueError):
        server._codec().aggregate(ups, [1, 3, 2], g)
    agg = server.aggregate(list(ups), [1, 3, 2])
    ref = UpdateCodec(1.0, 4, "weights", backend=BlockOracleBackend(), blockwise=True)
    decoded = [ref.decode_module(ref.encode(m.state_dict()), g) for m in mods]
    want = federated_averaging([copy.deepcopy(d).cuda() for d in decoded], [1, 3, 2])  # torch's GPU division
    for (k, a), b in zip(agg.state_dict().items(), want.state_dict().values()):
        assert torch.equal(a.cpu(), b.cpu()), k
