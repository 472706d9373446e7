"""The bit-packed dense codes' kernels (k_pack_dense / k_unpack_dense / k_dense_deq_stream) against the
host model of the format, wire.pack_dense_codes / wire.unpack_dense_codes, and against the plain dense decode. Every
comparison is bit-exact. Small plans: the kernels have one instantiation per code width, a dword and a byte path
(segments that start at an odd out_off, or whose length is no multiple of 4), full and partial units, and segments
shorter than one 32-entry group."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, Encoded, UpdateCodec, _lib, wire
from coala_amd.layouts import build_module
from oracle import codec_oracle as O
from tests.oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 4095, 4096, 4097, 2 * 4096 + 5]
# explicit k == n rows (in_off, n, k, out_off): odd out_off, gaps between the rows' codes
ROWS = [(0, 33, 33, 5), (64, 4097, 4097, 101), (8192, 70, 70, 4300)]
PAD = 256
SENTINEL = 123.25


def _plan(kind, bits):
    if kind == "plain":
        return CodecPlan(SIZES, 1.0, bits)
    if kind == "empty":
        return CodecPlan(SIZES[:4] + [0] + SIZES[4:], 1.0, bits)
    if kind == "batched":
        return CodecPlan([33, 4097, 70], 1.0, bits, clients=3)
    return CodecPlan.from_segments(np.array(ROWS, dtype=np.uint64), bits)


def _case(plan, seed):
    """(codes uint8[total_k] with 0xFF wherever no segment owns the position, the numpy model's stream, segs)."""
    rng = np.random.default_rng(seed)
    segs = plan.table.segs.astype(np.int64)
    codes = np.full(plan.total_k, 0xFF, dtype=np.uint8)
    for _, n, _, oo in segs:
        codes[oo:oo + n] = rng.integers(0, 1 << plan.bits, n)
    want = wire.pack_dense_codes(codes, segs[:, 1], plan.bits, out_off=segs[:, 3])
    return codes, want, segs


def _owned(plan, segs):
    own = np.zeros(plan.total_k, dtype=bool)
    for _, n, _, oo in segs:
        own[oo:oo + n] = True
    return own


KINDS = ["plain", "empty", "batched", "rows"]


@pytest.mark.parametrize("bits", range(1, 8))
@pytest.mark.parametrize("kind", KINDS)
def test_pack_and_unpack(cuda, kind, bits):
    plan = _plan(kind, bits)
    assert plan.dense
    codes, want, segs = _case(plan, bits)
    P, K = plan.dense_packed_words, plan.total_k
    assert P == want.size == wire.dense_packed_words(segs[:, 1], bits)
    # pack: the codes' surroundings and the output pre-filled with 0xFF
    vbuf = torch.full((PAD + K + PAD,), 0xFF, dtype=torch.uint8, device="cuda")
    vbuf[PAD:PAD + K] = torch.from_numpy(codes).cuda()
    obuf = torch.full((P + 64,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    out = plan.pack_dense(vbuf[PAD:PAD + K], out=obuf)
    assert out.data_ptr() == obuf.data_ptr()
    got = obuf.cpu().numpy()
    np.testing.assert_array_equal(got[:P], want)  # (the model's padding bits are zero: so are the kernel's)
    assert (got[P:] == 0xFFFFFFFF).all()
    assert torch.equal(plan.pack_dense(Encoded(None, vbuf[PAD:PAD + K], None, None))[:P], obuf[:P])
    # unpack: canaries before and after vals, in a buffer longer than total_k; positions no segment owns stay
    ubuf = torch.full((PAD + K + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.unpack_dense(obuf[:P], out=ubuf[PAD:])
    u = ubuf.cpu().numpy()
    own = _owned(plan, segs)
    assert (u[:PAD] == 0xA5).all() and (u[PAD + K:] == 0xA5).all()
    np.testing.assert_array_equal(u[PAD:PAD + K][own], codes[own])
    assert (u[PAD:PAD + K][~own] == 0xA5).all()
    # padding bits of a received stream are ignored
    dirty = want.copy()
    W = (segs[:, 1] * bits + 31) // 32
    for n, w, p in zip(segs[:, 1], W, np.cumsum(W) - W):
        if w and (n * bits) % 32:
            dirty[p + w - 1] |= np.uint32((0xFFFFFFFF << int((n * bits) % 32)) & 0xFFFFFFFF)
    u2 = plan.unpack_dense(torch.from_numpy(dirty).cuda()).cpu().numpy()
    np.testing.assert_array_equal(u2[own], codes[own])


def _i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("base_kind", [None, "random", "special"])
@pytest.mark.parametrize("bits", range(1, 8))
@pytest.mark.parametrize("kind", KINDS)
def test_decode_packed(cuda, kind, bits, base_kind):
    plan = _plan(kind, bits)
    codes, want, segs = _case(plan, 10 + bits)
    rng = np.random.default_rng(bits)
    T = plan.n_segments
    mn = rng.standard_normal(T).astype(np.float32)
    scale = np.abs(rng.standard_normal(T)).astype(np.float32) * 0.01
    scale[::3] = 0.0
    base = None
    if base_kind is not None:
        base = rng.standard_normal(plan.span).astype(np.float32)
        if base_kind == "special":
            base[::5] = -0.0
            base[1::7] = np.float32(np.nan)
    d = lambda a: None if a is None else torch.from_numpy(a).cuda()
    packed, vals, dmn, dsc, dbase = d(want), d(codes), d(mn), d(scale), d(base)
    fresh = lambda: torch.full((plan.span + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    a = plan.decode_packed(packed, dmn, dsc, base=dbase, out=fresh())
    unpacked = plan.unpack_dense(packed, out=torch.full((plan.total_k,), 0xFF, dtype=torch.uint8, device="cuda"))
    enc = Encoded(torch.empty(0, dtype=torch.int32, device="cuda"), unpacked, dmn, dsc)
    b = plan.decode(enc, base=dbase, out=fresh())
    assert torch.equal(_i32(a), _i32(b))
    # ... and the oracle's dense decode; the alignment pads between segments and behind the span keep the sentinel
    idx = np.concatenate([np.arange(n, dtype=np.int32) for n in segs[:, 1]] + [np.zeros(0, np.int32)])
    if kind == "rows":  # (the oracle takes idx / vals at the rows' own out_off)
        full = np.zeros(plan.total_k, dtype=np.int32)
        for _, n, _, oo in segs:
            full[oo:oo + n] = np.arange(n)
        idx = full
    ref = np.full(plan.span, SENTINEL, dtype=np.float32)
    dec = O.decode(idx, codes, mn, scale, segs, bits, plan.span, base=base)
    inside = np.zeros(plan.span, dtype=bool)
    for off, n, _, _ in segs:
        inside[off:off + n] = True
    ref[inside] = dec[inside]
    got = a.cpu().numpy()
    np.testing.assert_array_equal(got[:plan.span].view(np.uint32), ref.view(np.uint32))
    assert (got[plan.span:] == SENTINEL).all() and (got[:plan.span][~inside] == SENTINEL).all()


def test_eight_bits_at_the_abi_level(cuda):
    """b = 8 (the host never packs it: the stream is as long as the codes) through the entry points themselves."""
    lib = _lib.load()
    plan = _plan("plain", 8)
    codes, want, segs = _case(plan, 8)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N = ctypes.c_void_p(0)
    b = ctypes.c_uint64()
    assert lib.coalac_plan_dense_packed_bytes(plan._h, ctypes.byref(b)) == 0 and b.value == 4 * want.size
    vals = torch.from_numpy(codes).cuda()
    packed = torch.full((want.size + 8,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    assert lib.coalac_pack_dense(plan._h, p(vals), p(packed), b, N) == 0
    np.testing.assert_array_equal(packed.cpu().numpy()[:want.size], want)
    assert (packed[want.size:].cpu().numpy() == 0xFFFFFFFF).all()
    back = torch.full((plan.total_k + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.coalac_unpack_dense(plan._h, p(packed), b, p(back), N) == 0
    assert torch.equal(back[:plan.total_k], vals) and (back[plan.total_k:] == 0xA5).all()
    mn = torch.linspace(-1, 1, plan.n_segments, device="cuda")
    scale = torch.full((plan.n_segments,), 0.004, device="cuda")
    out = torch.full((plan.span,), SENTINEL, device="cuda")
    assert lib.coalac_decode_packed(plan._h, p(packed), b, p(mn), p(scale), N, p(out), N) == 0
    ref = plan.decode(Encoded(torch.empty(0, dtype=torch.int32, device="cuda"), vals, mn, scale),
                      out=torch.full((plan.span,), SENTINEL, device="cuda"))
    assert torch.equal(_i32(out), _i32(ref))


def test_abi_errors(cuda):
    lib = _lib.load()
    plan = _plan("plain", 4)
    sparse = CodecPlan([5000, 300], 0.1, 4)
    raw = CodecPlan([64, 8], 1.0, 32)
    codes, want, _ = _case(plan, 1)
    vals, packed = torch.from_numpy(codes).cuda(), torch.from_numpy(want).cuda()
    keep = (vals.clone(), packed.clone())
    mn = torch.zeros(plan.n_segments, device="cuda")
    out = torch.zeros(plan.span, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N = ctypes.c_void_p(0)
    nbytes, short = ctypes.c_uint64(4 * want.size), ctypes.c_uint64(4 * want.size - 4)
    b = ctypes.c_uint64()
    assert lib.coalac_plan_dense_packed_bytes(None, ctypes.byref(b)) == -1
    assert lib.coalac_plan_dense_packed_bytes(plan._h, None) == -1
    good = {"coalac_pack_dense": (plan._h, p(vals), p(packed), nbytes, N),
            "coalac_unpack_dense": (plan._h, p(packed), nbytes, p(vals), N),
            "coalac_decode_packed": (plan._h, p(packed), nbytes, p(mn), p(mn), N, p(out), N)}
    pointers = {"coalac_pack_dense": (0, 1, 2), "coalac_unpack_dense": (0, 1, 3), "coalac_decode_packed": (0, 1, 3, 4, 6)}
    for name, args in good.items():
        fn = getattr(lib, name)
        for i in pointers[name]:  # every pointer NULL in turn (the decode's base may be NULL)
            assert fn(*[N if j == i else a for j, a in enumerate(args)]) == -1, (name, i)
        size_at = 3 if name == "coalac_pack_dense" else 2
        assert fn(*[short if j == size_at else a for j, a in enumerate(args)]) == -1
        assert b"packed_bytes" in lib.coalac_last_error()
        assert fn(sparse._h, *args[1:]) == -1
        assert b"dense" in lib.coalac_last_error()
        assert fn(raw._h, *args[1:]) == -1
        assert b"32" in lib.coalac_last_error()
    assert lib.coalac_plan_dense_packed_bytes(sparse._h, ctypes.byref(b)) == -1 and b"dense" in lib.coalac_last_error()
    assert lib.coalac_plan_dense_packed_bytes(raw._h, ctypes.byref(b)) == -1
    torch.cuda.synchronize()  # nothing was launched: the buffers are what they were
    assert torch.equal(vals, keep[0]) and torch.equal(packed, keep[1]) and not out.any()
    # the typed wrappers check before any launch
    for bad in (sparse, raw):
        with pytest.raises(ValueError):
            bad.dense_packed_words
        with pytest.raises(ValueError):
            bad.pack_dense(vals)
        with pytest.raises(ValueError):
            bad.unpack_dense(packed)
        with pytest.raises(ValueError):
            bad.decode_packed(packed, mn, mn)
    for call in (lambda: plan.pack_dense(vals[:-1]), lambda: plan.pack_dense(vals.cpu()),
                 lambda: plan.pack_dense(vals.view(torch.int8)), lambda: plan.pack_dense(vals, out=packed[:-1]),
                 lambda: plan.unpack_dense(packed[:-1]), lambda: plan.unpack_dense(packed.view(torch.int32)),
                 lambda: plan.unpack_dense(packed, out=vals[:-1]), lambda: plan.unpack_dense(packed.cpu()),
                 lambda: plan.decode_packed(packed[:-1], mn, mn), lambda: plan.decode_packed(packed, mn[:-1], mn),
                 lambda: plan.decode_packed(packed, mn, mn, out=out[:-40])):
        with pytest.raises(ValueError):
            call()
    assert all(getattr(lib, name)(*args) == 0 for name, args in good.items())
    torch.cuda.synchronize()


@pytest.mark.parametrize("layout", ["lenet", "resnet18"])
def test_end_to_end_codec(cuda, layout):
    """The HIP backend's v4 blob is the oracle backend's, byte for byte; the receiver moves the mn ... packed region
    (not the uint8 codes) to the device and decodes the stream there to what the oracle decodes."""
    model = build_module(layout, seed=1)
    hip = UpdateCodec(1.0, 4, "weights", pack_dense=True, recycle=False)
    ref = UpdateCodec(1.0, 4, "weights", backend=OracleBackend(), pack_dense=True)
    up = hip.encode_module(copy.deepcopy(model).cuda())
    assert up.header.get("dense_packed") is True and up.packed.is_cuda
    blob = up.to_bytes()
    want = ref.encode(model.state_dict())
    assert blob == want.to_bytes() and up.nbytes == want.nbytes
    # the sender's own decode (the server's reconstruction of its download) reads the stream too
    own = hip.decode_state(up)
    back = pickle.loads(pickle.dumps(up))
    staged = []
    inner = hip._staging
    hip._staging = lambda n: (staged.append(n), inner(n))[1]
    got = hip.decode_state(back)
    _, sec = wire.sections(blob)
    assert staged == [sec["packed"][0] + sec["packed"][1] - sec["mn"][0]]
    enc = back.encoded_to(torch.device("cuda", 0), staging=inner, plan=hip.plan_for(tuple(back._seg_sizes()), torch.device("cuda", 0), ratio=1.0, bits=4))
    hip._staged(torch.cuda.current_stream())
    assert enc.vals is None and enc.packed.is_cuda and enc.packed.numel() == sec["packed"][1] // 4
    oracle = ref.decode_state(pickle.loads(pickle.dumps(want)))
    assert list(got) == list(oracle) == list(own)
    for k in oracle:
        for mine in (got[k], own[k]):
            assert mine.dtype == oracle[k].dtype
            if mine.dtype == torch.float32:
                assert torch.equal(_i32(mine.cpu()), _i32(oracle[k])), k
            else:
                assert torch.equal(mine.cpu(), oracle[k]), k
