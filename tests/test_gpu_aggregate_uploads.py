"""coalac_aggregate_uploads (k_aggregate_uploads): the fused sparse FedAvg read from every upload's own
buffers — its idx / vals arrays (kind entries) or its wire v3 stream (kind compact).

The uploads are tests/aggregate_inputs.py's hand-built payloads cut into their clients (aggregate_uploads_model.split),
every client's arrays in separate allocations of differing sizes made in a shuffled order, so nothing lies at a constant
stride. Every result is compared bit for bit (NaN for NaN) over the WHOLE sentinel-filled output, pads and tail
included, against the numpy model (tests/aggregate_uploads_model.py, whose equality with tests/aggregate_model.py
tests/test_aggregate_uploads_cpu.py proves) and against coalac_aggregate on the concatenation of the same uploads."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, CompressedUpdate, CompressionServerMixin, UpdateCodec, _lib, wire
from coala_amd.compression import plugin as plugin_mod
from coala_amd.compression.plan import Encoded
from coala_amd.fl import LoopbackServer
from coala_amd.layouts import build_module
from oracle import codec_oracle as O
from tests import aggregate_inputs as I
from tests import aggregate_uploads_model as UM
from tests.test_aggregate_uploads_cpu import COMPACT_CORRUPT, compact_corrupt, model_with_racy, random_words, same_bits

pytestmark = pytest.mark.gpu

MODES = {"recip": O.AGG_RECIP, "div": O.AGG_DIV, "sum": O.AGG_SUM}
KINDS = ("entries", "compact")
_plans = {}


def plan_of(p, clients=1):
    key = (tuple(p.table.sizes), p.table.ratio, p.bits, clients)
    if key not in _plans:
        _plans[key] = CodecPlan(p.table.sizes, p.table.ratio, p.bits, clients=clients)
    return _plans[key]


def on_device(ups, seed=0):
    """Every upload's arrays as separate device allocations, made client by client in a shuffled order with a
    throw-away allocation of a varying size between them; the arrays themselves carry a varying slack behind them."""
    rng = np.random.default_rng(seed)
    dev, keep = [None] * len(ups), []
    for c in rng.permutation(len(ups)):
        u, d = ups[c], {}
        for name in ("idx", "vals", "mn", "scale", "ustart", "packed"):
            a = getattr(u, name)
            if a is None:
                d[name] = None
                continue
            slack = int(rng.integers(0, 40)) * 4
            raw = torch.zeros((a.size + slack) * a.itemsize, dtype=torch.uint8, device="cuda")
            raw[:a.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)))
            d[name] = raw[:a.nbytes].view(torch.from_numpy(a[:0]).dtype)
            keep.append(torch.empty(int(rng.integers(1, 5000)), dtype=torch.uint8, device="cuda"))
        dev[c] = d
    return dev


def run(plan, dev, p, kind, mode, out=None, base="payload"):
    base = (None if p.base is None else torch.from_numpy(p.base).cuda()) if isinstance(base, str) else base
    out = sentinel_out(p) if out is None else out
    col = lambda f: [d[f] for d in dev]  # noqa: E731
    got = plan.aggregate_uploads(col("idx"), col("packed"), col("vals"), col("mn"), col("scale"), col("ustart"),
                                 p.weights, base=base, out=out, mode=mode, avg_mask=p.mask, kind=kind)
    torch.cuda.synchronize()
    assert got is out
    return out.cpu().numpy()


def sentinel_out(p):
    return torch.full((p.table.span_per_client + I.PAD,), float(I.SENTINEL), dtype=torch.float32, device="cuda")


def model(ups, p, kind, mode):
    out = np.full(p.table.span_per_client + I.PAD, I.SENTINEL, np.float32)
    UM.aggregate(ups, UM.one_layout_segs(p), p.bits, p.weights, sum(p.weights), MODES[mode], out, base=p.base,
                 avg_mask=p.mask, kind=kind)
    return out


def batched(p, mode):
    """coalac_aggregate on the concatenation of the same uploads (the batched plan's own buffers)."""
    plan = plan_of(p, p.clients)
    enc = plan.empty_encoded()
    for name in ("idx", "vals", "mn", "scale", "ustart"):
        getattr(enc, name).copy_(torch.from_numpy(np.ascontiguousarray(getattr(p, name))))
    out = sentinel_out(p)
    plan.aggregate(enc, p.weights, base=None if p.base is None else torch.from_numpy(p.base).cuda(), out=out, mode=mode,
                   avg_mask=p.mask)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check(p, mode, seed=0):
    """Both kinds of one payload against the model and against coalac_aggregate."""
    ups = [UM.pack(u, p.bits) for u in UM.split(p)]
    dev = on_device(ups, seed)
    ref = batched(p, mode)
    for kind in KINDS:
        got = run(plan_of(p), dev, p, kind, mode)
        same_bits(got, model(ups, p, kind, mode))
        same_bits(got, ref)


@pytest.mark.parametrize("name", [n for n in I.STRUCTURE if n != I.ALL_BITS_CASE])
def test_structure_case_both_kinds(cuda, name):
    """The 64 | 65 entries threshold, heavy clients at j = 0 / 15 / 16 / 63 / 64 of 70 (second 64-client chunk,
    AGG_DEPTH seams), empty ranges, half edges 0 / 2047 / 2048 / len - 1, odd-base halves, special ranges, the mask
    passthrough: each generator's docstring says which path it reaches."""
    check(I.STRUCTURE[name](8, True), "sum" if name == "mask_passthrough" else "recip")
    if name != "odd_base_half":
        check(I.STRUCTURE[name](8, False), "recip", seed=1)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("base", [True, False])
@pytest.mark.parametrize("bits", [1, 5, 8, 32])
def test_mixed_across_bit_widths_and_modes(cuda, bits, base, mode):
    """Field widths 13, 17, 20 and 12 (bits 32: the fp32 values beside the stream), every division mode."""
    assert wire.field_bits(bits) == {1: 13, 5: 17, 8: 20, 32: 12}[bits]
    check(I.mixed(bits, base), mode, seed=bits)


# total_k = 8: 8 x 20 bits end exactly with word 4; total_k = 7: the last field occupies bits [120, 140), from word 3
# into the stream's final word 4
EDGE_SIZES = {"whole_words": [5000, 300, 100, 7], "last_field_straddles": [5000, 300, 100]}


@pytest.mark.parametrize("base", [True, False])
@pytest.mark.parametrize("edge", list(EDGE_SIZES))
def test_stream_ends_with_its_allocation(cuda, edge, base):
    """ks 5, 1, 1 (, 1) at ratio 0.001 and bits 8 (w = 20). packed_bytes is exactly coalac_plan_packed_bytes and every
    stream the last bytes of its allocation, all-ones words before it and an all-ones canary allocation behind it."""
    p = I.build(8, 5, 40, ratio=0.001, sizes=EDGE_SIZES[edge], base=base)
    plan = plan_of(p)
    K, w = plan.total_k, 20
    assert list(p.table.ks) == [5, 1, 1, 1][:len(p.table.sizes)]
    if edge == "whole_words":
        assert K == 8 and K * w % 32 == 0
    else:
        assert K == 7 and ((K - 1) * w) % 32 + w > 32 and ((K - 1) * w) // 32 + 1 == plan.packed_words - 1
    ups = [UM.pack(u, 8) for u in UM.split(p)]
    dev = on_device(ups)
    canaries = []
    for u, d in zip(ups, dev):
        assert u.packed.size == plan.packed_words
        buf = torch.full((128,), -1, dtype=torch.int32, device="cuda").view(torch.uint32)  # one 512-byte block
        canaries.append(torch.full((128,), -1, dtype=torch.int32, device="cuda"))
        buf.view(torch.int32)[-u.packed.size:].copy_(torch.from_numpy(u.packed.view(np.int32)))
        d["packed"] = buf[-u.packed.size:]
    got = run(plan, dev, p, "compact", "recip")
    same_bits(got, model(ups, p, "compact", "recip"))
    same_bits(got, batched(p, "recip"))
    assert all(bool((c == -1).all()) for c in canaries)


@pytest.mark.parametrize("kind,clients,bits,base", I.CORRUPT_CASES)
def test_corrupt_entries_match_model_and_decode_each(cuda, kind, clients, bits, base):
    """aggregate_inputs.CORRUPT_CASES in kind entries: the whole buffer equals the model, and the segments equal
    coalac_decode of every corrupt upload followed by torch's weighted sum and division on the GPU."""
    p = I.corrupt(kind, clients, bits, base)
    ups = UM.split(p)
    dev = on_device(ups)
    plan = plan_of(p)
    got = run(plan, dev, p, "entries", "recip")
    same_bits(got, model(ups, p, "entries", "recip"))
    b = None if p.base is None else torch.from_numpy(p.base).cuda()
    acc = None
    for d, wgt in zip(dev, p.weights):
        x = plan.decode(Encoded(d["idx"], d["vals"], d["mn"], d["scale"], d["ustart"]), base=b)
        acc = x * wgt if acc is None else acc.add_(x * wgt)
    ref = torch.div(acc, sum(p.weights)).cpu().numpy()
    for off, n in zip(p.table.offsets, p.table.sizes):
        same_bits(got[off:off + n], ref[off:off + n])


def _defined(got, want, racy, p):
    ins = np.zeros(got.size, bool)
    for off, n in zip(p.table.offsets, p.table.sizes):
        ins[off:off + n] = True
    assert np.all(got[~ins] == I.SENTINEL)  # pads and the tail behind the span
    same_bits(got[~racy], want[~racy])
    return ins


@pytest.mark.parametrize("kind,clients,bits,base", COMPACT_CORRUPT)
def test_corrupt_starts_compact(cuda, kind, clients, bits, base):
    """Wrong starts over valid streams: a shifted range can apply a neighbouring unit's entry, whose 12-bit position may
    repeat one of this unit's — the result equals the stream model in every unit where no client applies a position
    twice (that some such unit exists and differs from the valid upload's: tests/test_aggregate_uploads_cpu.py);
    everywhere the sentinels outside the segments survive."""
    ups, p = compact_corrupt(kind, clients, bits, base)
    want, racy, _ = model_with_racy(ups, p, O.AGG_RECIP)
    got = run(plan_of(p), on_device(ups), p, "compact", "recip")
    _defined(got, want, racy, p)


@pytest.mark.parametrize("base", [True, False])
def test_random_field_words_stay_in_bounds(cuda, base):
    """A stream of random words (one client, weight 1, mode sum, mn 1, scale 0.5): the model where it is defined; in
    the racy units every element is base + 0 or base + (1 + 0.5 q) for a code q; the sentinels are intact."""
    ups, p = random_words(base)
    want, racy, _ = model_with_racy(ups, p, O.AGG_SUM)
    got = run(plan_of(p), on_device(ups), p, "compact", "sum")
    ins = _defined(got, want, racy, p)
    d = np.concatenate([[np.float32(0)], np.float32(1) + np.arange(256, dtype=np.float32) * np.float32(0.5)])
    sel = np.flatnonzero(ins & racy)
    allowed = d[None, :] if p.base is None else p.base[sel, None] + d[None, :]
    assert sel.size and np.all((got[sel, None] == allowed).any(axis=1))


def test_abi_errors(cuda):
    lib = _lib.load()
    p = I.threshold(8, True)
    plan = plan_of(p)
    ups = [UM.pack(u, 8) for u in UM.split(p)]
    dev = on_device(ups)
    C = len(ups)
    names = ("idx", "packed", "vals", "mn", "scale", "ustart")
    tab = torch.tensor([[d[n].data_ptr() for d in dev] for n in names], dtype=torch.int64).cuda()
    w = torch.tensor([1.0, 3.0, 2.0], device="cuda")
    out, base = sentinel_out(p), torch.from_numpy(p.base).cuda()
    ptr = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)  # noqa: E731
    N = ctypes.c_void_p(0)
    fn = lib.coalac_aggregate_uploads
    dense = CodecPlan([64, 8], 1.0, 8)
    raw = CodecPlan(p.table.sizes, p.table.ratio, 32)
    empty = CodecPlan([0, 0], 0.5, 8)

    def args(kind, plan_=plan):
        return [plan_._h, C, plan.AGG_UPLOAD_KINDS[kind], ptr(tab[0]), ptr(tab[1]), ctypes.c_uint64(4 * plan.packed_words),
                ptr(tab[2]), ptr(tab[3]), ptr(tab[4]), ptr(tab[5]), ptr(w), ctypes.c_float(6.0), _lib.COALAC_AGG_RECIP,
                N, ptr(base), ptr(out), N]

    def bad(word, kind="compact", plan_=plan, **change):
        a = args(kind, plan_)
        for i, v in change.items():
            a[int(i[1:])] = v
        assert fn(*a) == -1, change
        msg = lib.coalac_last_error()
        assert b"coalac_aggregate_uploads" in msg and word in msg, msg

    bad(b"coalac_aggregate_dense", plan_=dense)
    bad(b"clients", a1=0)
    bad(b"clients", a1=-2)
    bad(b"kind", a2=2)
    bad(b"kind", a2=-1)
    bad(b"mode", a12=3)
    bad(b"NULL", a9=N)                   # ustart
    bad(b"NULL", a10=N)                  # weights
    bad(b"NULL", a15=N)                  # output
    bad(b"NULL", a4=N)                   # compact: the streams
    bad(b"NULL", kind="entries", a3=N)   # entries: idx
    bad(b"NULL", kind="entries", a6=N)   # entries: vals
    bad(b"NULL", plan_=raw, a6=N)        # compact at bits 32: the fp32 values
    bad(b"NULL", a7=N)                   # mn
    bad(b"NULL", a8=N)                   # scale
    bad(b"packed_bytes", a5=ctypes.c_uint64(4 * plan.packed_words - 4))
    bad(b"aligned", a15=ptr(out, 4))
    bad(b"aligned", a14=ptr(base, 8))
    assert fn(None, *args("compact")[1:]) == -1
    torch.cuda.synchronize()  # nothing was launched
    assert (out == float(I.SENTINEL)).all()
    assert fn(*args("compact", empty)) == 0  # a plan without units: OK, nothing launched
    torch.cuda.synchronize()
    assert (out == float(I.SENTINEL)).all()
    # what a kind does not read may be NULL
    a = args("compact")
    a[3], a[6] = N, N
    assert fn(*a) == 0
    a = args("entries")
    a[4], a[5] = N, ctypes.c_uint64(0)
    assert fn(*a) == 0
    torch.cuda.synchronize()
    # the typed wrapper checks every tensor before any launch
    col = lambda f: [d[f] for d in dev]  # noqa: E731
    A = [col(n) for n in names]
    call = lambda *a, **k: plan.aggregate_uploads(*a, p.weights, **k)  # noqa: E731
    short = lambda ts: [ts[0], ts[1][:-1], ts[2]]  # noqa: E731
    with pytest.raises(ValueError):
        dense.aggregate_uploads(*A, p.weights)
    for wrong in (lambda: call(*A, kind="stream"), lambda: call(*A, mode="mean"),
                  lambda: call(A[0][:2], *A[1:]),
                  lambda: call(short(A[0]), *A[1:]),
                  lambda: call(A[0], short(A[1]), *A[2:], kind="compact"),
                  lambda: call(*A[:5], short(A[5])),
                  lambda: call(*A[:3], short(A[3]), *A[4:]),
                  lambda: call([A[0][0].cpu()] + A[0][1:], *A[1:]),
                  lambda: call([A[0][0].view(torch.float32)] + A[0][1:], *A[1:]),
                  lambda: call(*A, avg_mask=[True]),
                  lambda: call(*A, out=out[1:]),
                  lambda: call(*A, base=base[:-40])):
        with pytest.raises(ValueError):
            wrong()
    # an odd-byte offset of a code array is not 4-byte aligned
    odd = torch.zeros(plan.total_k + 8, dtype=torch.uint8, device="cuda")[1:plan.total_k + 1]
    with pytest.raises(ValueError, match="aligned"):
        call(A[0], A[1], [odd] + A[2][1:], *A[3:])


# -- hooks ----------------------------------------------------------------------------------------------
def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].is_cuda and sb[k].is_cuda, k
        if sa[k].dtype == torch.float32:
            same_bits(sa[k].cpu().numpy().reshape(-1), sb[k].cpu().numpy().reshape(-1))
        else:
            assert torch.equal(sa[k], sb[k]), k


def _blobs(compact, bits=8, mode="delta", n=16):
    g = build_module("lenet", seed=5).cuda()
    client = UpdateCodec(0.05, bits, mode, compact=compact)
    base = client.snapshot(g) if mode == "delta" else None
    ups = [CompressedUpdate.from_bytes(client.encode_module(build_module("lenet", seed=s).cuda(), base=base).to_bytes())
           for s in range(1, n + 1)]
    return g, base, ups


def _spy(plan, calls):
    inner = plan.aggregate_uploads
    plan.aggregate_uploads = lambda *a, **k: (calls.append(k.get("kind")), inner(*a, **k))[1]


@pytest.mark.parametrize("bits", [8, 32])
@pytest.mark.parametrize("compact", [False, True], ids=["v2", "v3"])
def test_sixteen_received_blobs(cuda, compact, bits):
    """16 lenet blobs of a client codec through from_bytes: sparse_uploads=True equals False bit for bit, in one
    aggregate_uploads call of the format's kind — and a compact blob is neither unpacked nor given room for idx."""
    g, base, ups = _blobs(compact, bits)
    assert wire.format_of(ups[0].header).version == (3 if compact else 2)
    server = UpdateCodec(0.05, bits, "delta", recycle=False)
    weights = list(range(1, 17))
    want = server.aggregate(ups, weights, g, base=base)
    plan = server.sparse_uploads_plan(ups)
    calls = []
    _spy(plan, calls)
    plan.unpack = lambda *a, **k: pytest.fail("a compact upload must stay compact")
    try:
        got = server.aggregate(ups, weights, g, base=base, sparse_uploads=True)
        params = server.aggregate(ups, weights, g, base=base, sparse_uploads=True, params_only=True)
    finally:
        del plan.aggregate_uploads
        del plan.unpack
    assert calls == ["compact" if compact else "entries"] * 2
    _same_state(got, want)
    _same_state(params, server.aggregate(ups, weights, g, base=base, params_only=True))


def test_local_compact_carriers_are_read_where_they_are(cuda):
    g = build_module("lenet", seed=5).cuda()
    codec = UpdateCodec(0.05, 8, "weights", compact=True, recycle=False)
    ups = [codec.encode_module(build_module("lenet", seed=s).cuda()) for s in (1, 2, 3)]
    assert all(u.stream_for(torch.device("cuda", 0)) for u in ups)
    e = ups[0].encoded_to(torch.device("cuda", 0), keep_packed=True)
    assert e.packed.data_ptr() == ups[0].packed.data_ptr() and e.mn.data_ptr() == ups[0].encoded.mn.data_ptr()
    calls = []
    _spy(codec.sparse_uploads_plan(ups), calls)
    try:
        got = codec.aggregate(ups, [1, 3, 2], g, sparse_uploads=True)
    finally:
        del codec.sparse_uploads_plan(ups).aggregate_uploads
    assert calls == ["compact"]
    _same_state(got, codec.aggregate(ups, [1, 3, 2], g))


@pytest.mark.parametrize("distributed", [False, True], ids=["single", "distributed"])
@pytest.mark.parametrize("compact", [False, True], ids=["v2", "v3"])
def test_server_switch(cuda, compact, distributed, monkeypatch):
    """CompressionServerMixin.codec_fused_sparse_uploads in the single-process branch and, with is_distributed and a
    recording reduce_models, in the per-rank weighted-sum branch: one aggregate_uploads call, the same model as off."""
    g, base, ups = _blobs(compact, mode="weights", n=3)
    reduced = []
    monkeypatch.setattr(plugin_mod, "reduce_models", lambda params_only=False: lambda m, s: reduced.append(float(s)))
    monkeypatch.setattr(torch.distributed, "barrier", lambda *a, **k: None)

    class Conf:
        class server:
            aggregation_strategy = "FedAvg"
            aggregation_content = "all"
        is_distributed = distributed

    def server(on):
        class Server(CompressionServerMixin, LoopbackServer):
            codec_ratio, codec_bits, codec_mode = 0.05, 8, "weights"
            codec_fused_aggregate = True
            codec_fused_sparse_uploads = on
        s = Server(copy.deepcopy(g), [])
        s.conf = Conf
        return s

    on, off = server(True), server(False)
    want = off.aggregate(list(ups), [1, 3, 2])
    calls = []
    plan = on._codec().sparse_uploads_plan(ups)
    _spy(plan, calls)
    try:
        got = on.aggregate(list(ups), [1, 3, 2])
    finally:
        del plan.aggregate_uploads
    assert calls == ["compact" if compact else "entries"]
    assert reduced == ([6.0, 6.0] if distributed else [])
    _same_state(got, want)
    assert pickle.loads(pickle.dumps(ups[0])).header == ups[0].header  # (the uploads are untouched)
