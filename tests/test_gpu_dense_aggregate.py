"""k_aggregate_dense (coalac_aggregate_dense) against the model (tests/dense_aggregate_model.py: the
oracle's aggregate over implied indices, over the split table for block-wise data) AND against the GPU composition it
replaces (decode / decode_packed / decode_block of every upload, torch's weighted sum, torch.div). Every comparison is
bit-exact (a NaN compares as NaN: its payload is not part of the spec). The layout has ragged tails, lengths that are
no multiple of 4, an empty segment, exact and multi-unit segments; every client's buffers are separate allocations."""
import copy
import ctypes
import pickle

import numpy as np
import pytest
import torch

from coala_amd import workload
from coala_amd.compression import CodecPlan, CompressionServerMixin, UpdateCodec, _lib
from coala_amd.compression.spec import SegmentTable
from coala_amd.fl import LoopbackServer
from coala_amd.layouts import build_module, fp32_sizes
from tests import dense_aggregate_model as DM

pytestmark = pytest.mark.gpu

UNIT = 4096
SIZES = [1, 5, 0, 4095, 4096, 4097, 3 * 4096 + 5, 2 * 4096]
DEPTH = _lib.AGGD_DEPTH  # AGD_DEPTH of coalac.hip: the clients whose code words a wave loads together
CLIENTS = [1, 2, 5, DEPTH + 3]
WEIGHTS = [3, 0, 1.0e6, 7, 2, 5, 11, 1, 4, 9, 6, 8][:max(CLIENTS)]  # a 0 and a large value among them
SENTINEL = 123.25
_PLANS, _INPUTS = {}, {}
assert len(WEIGHTS) == max(CLIENTS)


def _plan(bits, layout="sizes"):
    key = (bits, layout)
    if key not in _PLANS:
        _PLANS[key] = CodecPlan(SIZES if layout == "sizes" else fp32_sizes(layout), 1.0, bits)
    return _PLANS[key]


class _Upload:
    """One client's payload in the three forms, every buffer its own allocation, with host copies for the model."""

    def __init__(self, plan, flat, base):
        enc = plan.encode(flat, base=base)
        self.codes, self.mn, self.scale = enc.vals.clone(), enc.mn.clone(), enc.scale.clone()
        self.stream = plan.pack_dense(self.codes).clone()
        bmn, bsc, bstream = plan.encode_block(flat=flat, base=base)
        self.bmn, self.bscale, self.bstream = bmn.clone(), bsc.clone(), bstream.clone()
        torch.cuda.synchronize()
        self.host = {k: getattr(self, k).cpu().numpy() for k in
                     ("codes", "mn", "scale", "stream", "bmn", "bscale", "bstream")}

    def of(self, kind, host=False):
        names = {"codes": ("codes", "mn", "scale"), "packed": ("stream", "mn", "scale"),
                 "block": ("bstream", "bmn", "bscale")}[kind]
        return tuple(self.host[n] if host else getattr(self, n) for n in names)


def _inputs(bits, delta, layout="sizes", clients=max(CLIENTS)):
    """(plan, uploads, base on the device, base on the host): workload.synth_batch's updates, encoded on the device."""
    key = (bits, delta, layout)
    if key not in _INPUTS:
        plan = _plan(bits, layout)
        table = SegmentTable(plan.table.sizes, 1.0, clients)
        flat = workload.synth_batch(table, torch.device("cuda", 0))
        base = None
        if delta:
            base = workload.synth_batch(SegmentTable(plan.table.sizes, 1.0, 1), torch.device("cuda", 0), client_ids=[99])
        so = table.client_span_off
        ups = [_Upload(plan, flat[so[c]:so[c] + plan.span].clone(), base) for c in range(clients)]
        _INPUTS[key] = (plan, ups, base, None if base is None else base.cpu().numpy())
    return _INPUTS[key]


def _inside(plan):
    m = np.zeros(plan.span, dtype=bool)
    for off, n, _, _ in plan.table.segs.astype(np.int64).tolist():
        m[off:off + n] = True
    return m


def _run(plan, kind, ups, weights, mode, base, avg_mask=None, tail=64):
    out = torch.full((plan.span + tail,), SENTINEL, dtype=torch.float32, device="cuda")
    c, m, s = zip(*(u.of(kind) for u in ups))
    got = plan.aggregate_dense(list(c), list(m), list(s), weights, base=base, out=out, mode=mode, avg_mask=avg_mask,
                               kind=kind)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy()


def _model(plan, kind, ups, weights, mode, hbase, avg_mask=None):
    c, m, s = zip(*(u.of(kind, host=True) for u in ups))
    return DM.expected(kind, c, m, s, plan.table.segs.astype(np.int64), plan.bits, weights, float(sum(weights)), mode,
                       plan.span, base=hbase, avg_mask=avg_mask)


def _composition(plan, kind, ups, weights, base):
    """What the kernel replaces, on the device: one dense decode per upload, torch's weighted sum, torch.div."""
    dec = []
    for u in ups:
        c, m, s = u.of(kind)
        if kind == "codes":
            from coala_amd.compression.plan import Encoded
            dec.append(plan.decode(Encoded(torch.empty(0, dtype=torch.int32, device="cuda"), c, m, s), base=base))
        elif kind == "packed":
            dec.append(plan.decode_packed(c, m, s, base=base))
        else:
            dec.append(plan.decode_block(c, m, s, base=base))
    acc = dec[0] * weights[0]
    for d, w in zip(dec[1:], weights[1:]):
        acc += d * w
    return torch.div(acc, float(sum(weights))).cpu().numpy()


def _check(got, want, plan, inside):
    DM.same_bits(got[:plan.span][inside], want[:plan.span][inside])
    # canaries: the padding between segments and everything after the span are never written
    assert (got[:plan.span][~inside] == SENTINEL).all() and (got[plan.span:] == SENTINEL).all()


@pytest.mark.parametrize("delta", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("bits", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("kind", DM.KINDS)
def test_parity(cuda, kind, bits, delta):
    plan, ups, base, hbase = _inputs(bits, delta)
    inside = _inside(plan)
    for C in CLIENTS:
        w = WEIGHTS[:C]
        for mode in ("recip", "div", "sum"):
            got = _run(plan, kind, ups[:C], w, mode, base)
            _check(got, _model(plan, kind, ups[:C], w, mode, hbase), plan, inside)
            if mode == "recip":
                comp = _composition(plan, kind, ups[:C], w, base)
                DM.same_bits(got[:plan.span][inside], comp[:plan.span][inside])


@pytest.mark.parametrize("kind", DM.KINDS)
def test_parity_lenet(cuda, kind):
    plan, ups, base, hbase = _inputs(4, True, layout="lenet", clients=3)
    assert plan.n_units > 1000
    inside = _inside(plan)
    w = [13, 0, 7]
    got = _run(plan, kind, ups, w, "recip", base)
    _check(got, _model(plan, kind, ups, w, "recip", hbase), plan, inside)
    DM.same_bits(got[:plan.span][inside], _composition(plan, kind, ups, w, base)[:plan.span][inside])


@pytest.mark.parametrize("mode", ["recip", "sum"])
@pytest.mark.parametrize("kind", DM.KINDS)
def test_mask_and_odd_bases(cuda, kind, mode):
    """An avg mask with both values (first segment averaged, second not, then alternating); a base holding -0.0, NaN
    and +-Inf; data holding NaN (a NaN element, and for the block-wise form a block that is all NaN)."""
    bits = 4
    plan = _plan(bits)
    rng = np.random.default_rng(11)
    segs = plan.table.segs.astype(np.int64)
    hbase = rng.standard_normal(plan.span).astype(np.float32)
    hbase[::5] = -0.0
    hbase[1::7] = np.nan
    hbase[2::11] = np.inf
    hbase[3::13] = -np.inf
    base = torch.from_numpy(hbase).cuda()
    ups = []
    for c in range(3):
        x = (rng.standard_normal(plan.span) * 10.0 ** rng.uniform(-3, 0)).astype(np.float32)
        x[c::17] = np.nan
        off = int(segs[6, 0])
        if c == 1:
            x[off + UNIT:off + 2 * UNIT] = np.nan  # one whole block of the multi-unit segment
        ups.append(_Upload(plan, torch.from_numpy(x).cuda(), None))
    mask = [i % 2 == 0 for i in range(len(SIZES))]
    assert mask[0] and not mask[1]
    inside = _inside(plan)
    w = [2, 0, 5]
    for b, hb in ((base, hbase), (None, None)):
        got = _run(plan, kind, ups, w, mode, b, avg_mask=mask)
        _check(got, _model(plan, kind, ups, w, mode, hb, avg_mask=mask), plan, inside)
        # a segment left out of the average is client 0's decode
        alone = _run(plan, kind, ups[:1], [1], "sum", b)
        for (off, n, _, _), m in zip(segs.tolist(), mask):
            if not m:
                DM.same_bits(got[off:off + n], alone[off:off + n])


@pytest.mark.parametrize("bits", [3, 4, 7])
@pytest.mark.parametrize("kind", ["packed", "block"])
def test_untrusted_stream_padding_is_ignored(cuda, kind, bits):
    plan, ups, base, _ = _inputs(bits, False)
    segs = plan.table.segs.astype(np.int64)
    W = (segs[:, 1] * bits + 31) // 32
    dirty_ups = []
    for u in ups[:3]:
        d = copy.copy(u)
        for name in ("stream", "bstream"):
            words = u.host[name].copy()
            for n, w, p in zip(segs[:, 1], W, np.cumsum(W) - W):
                if w and (n * bits) % 32:
                    words[p + w - 1] |= np.uint32((0xFFFFFFFF << int((n * bits) % 32)) & 0xFFFFFFFF)
            assert not np.array_equal(words, u.host[name])
            setattr(d, name, torch.from_numpy(words).cuda())
        dirty_ups.append(d)
    w = WEIGHTS[:3]
    np.testing.assert_array_equal(_run(plan, kind, dirty_ups, w, "recip", None).view(np.uint32),
                                  _run(plan, kind, ups[:3], w, "recip", None).view(np.uint32))


def test_abi_errors(cuda):
    lib = _lib.load()
    plan, ups, base, _ = _inputs(4, True)
    sparse = CodecPlan([5000, 300], 0.1, 4)
    raw = CodecPlan([64, 8], 1.0, 32)
    empty = CodecPlan([0, 0], 1.0, 4)
    C = 2
    out = torch.full((plan.span,), SENTINEL, device="cuda")
    tabs = {k: torch.tensor([t.data_ptr() for u in ups[:C] for t in (u.of(k)[i] for i in range(3))],
                            dtype=torch.int64).view(C, 3).t().contiguous().cuda() for k in DM.KINDS}
    w = torch.tensor([1.0, 3.0], device="cuda")
    mask = torch.ones(len(SIZES), dtype=torch.uint8, device="cuda")
    p = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)
    N = ctypes.c_void_p(0)
    fn = lib.coalac_aggregate_dense

    def args(kind, plan_=plan):
        t = tabs[kind]
        nbytes = plan.total_k if kind == "codes" else 4 * plan.dense_packed_words
        return [plan_._h, C, plan.AGG_DENSE_KINDS[kind], p(t[0]), ctypes.c_uint64(nbytes), p(t[1]), p(t[2]), p(w),
                ctypes.c_float(4.0), _lib.COALAC_AGG_RECIP, p(mask), p(base), p(out), N]

    def bad(word, kind="packed", **change):
        a = args(kind)
        for i, v in change.items():
            a[int(i[1:])] = v
        assert fn(*a) == -1, change
        msg = lib.coalac_last_error()
        assert b"coalac_aggregate_dense" in msg and word in msg, msg

    bad(b"dense", a0=sparse._h)
    bad(b"32", a0=raw._h)
    bad(b"clients", a1=0)
    bad(b"clients", a1=-3)
    bad(b"kind", a2=3)
    bad(b"kind", a2=-1)
    bad(b"mode", a9=3)
    for i in (3, 5, 6, 7, 12):
        bad(b"NULL", **{f"a{i}": N})
    bad(b"code_bytes", a4=ctypes.c_uint64(4 * plan.dense_packed_words - 4))
    bad(b"code_bytes", kind="codes", a4=ctypes.c_uint64(plan.total_k - 1))
    bad(b"aligned", a12=p(out, 4))
    bad(b"aligned", a11=p(base, 8))
    assert fn(None, *args("packed")[1:]) == -1
    torch.cuda.synchronize()  # nothing was launched: the output is what it was
    assert (out == SENTINEL).all()
    # a plan without units: OK, nothing launched; NULL base and mask: fine
    a = args("packed", empty)
    a[4] = ctypes.c_uint64(0)
    assert fn(*a) == 0
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    for kind in DM.KINDS:
        a = args(kind)
        a[10], a[11] = N, N
        assert fn(*a) == 0
    torch.cuda.synchronize()
    # the typed wrapper checks before any launch
    c, m, s = (list(x) for x in zip(*(u.of("packed") for u in ups[:C])))
    bm, bs = [u.bmn for u in ups[:C]], [u.bscale for u in ups[:C]]
    codes = [u.codes for u in ups[:C]]
    for wrong in (sparse, raw):
        with pytest.raises(ValueError):
            wrong.aggregate_dense(c, m, s, [1, 3], kind="packed")
    for call in (lambda: plan.aggregate_dense(c, m, s, [1], kind="packed"),
                 lambda: plan.aggregate_dense(c, m[:1], s, [1, 3], kind="packed"),
                 lambda: plan.aggregate_dense([], [], [], [], kind="packed"),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="stream"),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="packed", mode="mean"),
                 lambda: plan.aggregate_dense([c[0], c[1][:-1]], m, s, [1, 3], kind="packed"),
                 lambda: plan.aggregate_dense([c[0], c[1].view(torch.int32)], m, s, [1, 3], kind="packed"),
                 lambda: plan.aggregate_dense([c[0], c[1].cpu()], m, s, [1, 3], kind="packed"),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="block"),  # per-segment ranges: too few for blocks
                 lambda: plan.aggregate_dense(c, bm, [bs[0], bs[1][:-1]], [1, 3], kind="block"),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="codes"),  # streams are not uint8 codes
                 lambda: plan.aggregate_dense([codes[0], codes[1][1:]], m, s, [1, 3], kind="codes"),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="packed", avg_mask=[True]),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="packed", out=out[:-40]),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="packed", out=out[1:]),
                 lambda: plan.aggregate_dense(c, m, s, [1, 3], kind="packed", base=base[:-40])):
        with pytest.raises(ValueError):
            call()


# -- end to end -----------------------------------------------------------------------------------------
def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].is_cuda and sb[k].is_cuda, k
        if sa[k].dtype == torch.float32:
            DM.same_bits(sa[k].cpu().numpy().reshape(-1), sb[k].cpu().numpy().reshape(-1))
        else:
            assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("fmt", ["block4", "packed4", "plain8", "block4_delta", "packed4_params"])
def test_server_round_end_to_end(cuda, fmt):
    """Three pickled lenet uploads through a CompressionServerMixin server with both switches on, against the same
    server with the new switch off (block-wise: decode_module of every upload + FedAvg; per-tensor: the sparse fused
    kernel over implied indices)."""
    bits = 8 if fmt.startswith("plain") else 4
    mode = "delta" if fmt.endswith("delta") else "weights"
    kw = dict(blockwise=True) if fmt.startswith("block") else dict(pack_dense=True) if fmt.startswith("packed") else {}

    class Conf:
        class server:
            aggregation_strategy = "FedAvg"
            aggregation_content = "parameters" if fmt.endswith("params") else "all"
        is_distributed = False

    def server(dense):
        class Server(CompressionServerMixin, LoopbackServer):
            codec_ratio, codec_bits, codec_mode = 1.0, bits, mode
            codec_fused_aggregate = True
            codec_fused_dense_aggregate = dense
        s = Server(copy.deepcopy(g).cuda(), [])
        s.conf = Conf
        return s

    g = build_module("lenet", seed=5)
    on, off = server(True), server(False)
    hip = UpdateCodec(1.0, bits, mode, **kw)
    base = hip.snapshot(copy.deepcopy(g).cuda()) if mode == "delta" else None
    ups = [pickle.loads(pickle.dumps(hip.encode_module(build_module("lenet", seed=s).cuda(), base=base)))
           for s in (1, 2, 3)]
    assert all(on.decompression(u) is u for u in ups)
    calls = []
    plan = on._codec().dense_aggregate_plan(ups[0].header)
    inner = plan.aggregate_dense
    plan.aggregate_dense = lambda *a, **k: (calls.append(k.get("kind")), inner(*a, **k))[1]
    try:
        got = on.aggregate(list(ups), [1, 3, 2])
    finally:
        del plan.aggregate_dense
    assert calls == [{"block4": "block", "packed4": "packed", "plain8": "codes"}[fmt.split("_")[0]]]
    _same_state(got, off.aggregate(list(ups), [1, 3, 2]))
