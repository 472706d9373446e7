"""The sparse fused aggregate from each upload's own buffers, without a GPU: the per-upload model
(tests/aggregate_uploads_model.py) against tests/aggregate_model.py on the concatenated uploads, the dropped-position
rule by hand, CompressedUpdate.encoded_to(keep_packed=True), the host routing of UpdateCodec.aggregate(...,
sparse_uploads=True) and the server switch with the model behind the plan interface, and the C ABI's new symbol."""
import ctypes
import pickle
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

from coala_amd.compression import CompressedUpdate, CompressionServerMixin, UpdateCodec, _lib, wire
from coala_amd.compression.plan import Encoded
from coala_amd.fl import LoopbackServer
from oracle import codec_oracle as O
from tests import aggregate_inputs as I
from tests import aggregate_model as M
from tests import aggregate_uploads_model as UM
from tests.oracle_backend import OracleBackend

KINDS = ("entries", "compact")
CPU = torch.device("cpu")


def same_bits(g, ref):
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(g), nan)
    np.testing.assert_array_equal(g[~nan].view(np.uint32), ref[~nan].view(np.uint32))


def both_models(p, kind, mode=O.AGG_RECIP):
    """(the per-upload model's buffer and counts, the batched model's) on a sentinel-filled output."""
    ups = [UM.pack(u, p.bits) for u in UM.split(p)]
    n = p.table.span_per_client + I.PAD
    got, want = np.full(n, I.SENTINEL, np.float32), np.full(n, I.SENTINEL, np.float32)
    c1 = UM.aggregate(ups, UM.one_layout_segs(p), p.bits, p.weights, sum(p.weights), mode, got, base=p.base,
                      avg_mask=p.mask, kind=kind)
    c2 = M.aggregate(p.idx, p.vals, p.mn, p.scale, p.ustart, p.segs, p.bits, p.clients, p.weights, sum(p.weights),
                     mode, want, base=p.base, avg_mask=p.mask)
    return got, c1, want, c2


# -- the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(I.STRUCTURE))
def test_model_equals_batched_model_on_every_structure_case(name, kind):
    """Every structure case, cut into its clients' uploads (and packed into wire v3 streams): the per-upload model
    gives the batched model's whole buffer and applies / drops the same entries per client and unit."""
    p = I.STRUCTURE[name](8, True)
    got, c1, want, c2 = both_models(p, kind)
    same_bits(got, want)
    assert (c1.applied, c1.dropped) == (c2.applied, c2.dropped) and c1.dropped == 0
    np.testing.assert_array_equal(c1.units, c2.units)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bits", [1, 5, 32])
def test_model_equals_batched_model_across_bit_widths(bits, kind):
    p = I.STRUCTURE[I.ALL_BITS_CASE](bits, False)
    got, c1, want, c2 = both_models(p, kind, O.AGG_DIV)
    same_bits(got, want)
    assert c1.applied == c2.applied > 0


def test_dropped_position_rule_by_hand():
    """One segment of 300 elements keeping 3, one upload, weight 1, mode sum, mn 1, scale 0.5. Stream fields: position
    7 code 2, position 300 (== the unit's length: dropped) code 9, position 299 code 4. The same entries as idx
    7 / 300 / 299 give the same result in kind entries."""
    segs = np.array([[0, 300, 3, 0]], np.int64)
    w = wire.field_bits(8)
    f = [7 | 2 << 12, 300 | 9 << 12, 299 | 4 << 12]
    bits_ = sum(v << (i * w) for i, v in enumerate(f))
    packed = np.array([(bits_ >> (32 * i)) & 0xFFFFFFFF for i in range(2)], np.uint32)
    assert packed.size == wire.packed_words(3, 8)
    np.testing.assert_array_equal(UM.fields(packed, np.arange(3), w), f)
    u = UM.Upload(np.array([7, 300, 299], np.int32), np.array([2, 9, 4], np.uint8), np.array([1.0], np.float32),
                  np.array([0.5], np.float32), np.array([0], np.int32), packed)
    want = np.zeros(300, np.float32)
    want[7], want[299] = 2.0, 3.0
    for kind in KINDS:
        out = np.full(300 + 8, I.SENTINEL, np.float32)
        c = UM.aggregate([u], segs, 8, [1], 1.0, O.AGG_SUM, out, kind=kind)
        assert (c.applied, c.dropped) == (2, 1)
        np.testing.assert_array_equal(out[:300], want)
        assert np.all(out[300:] == I.SENTINEL)


# -- corrupt uploads, compact kind: what the GPU file runs is defined and not vacuous -----------------------------
COMPACT_CORRUPT = [(kind, C, bits, base) for kind in ("starts_plus1", "starts_random", "starts_garbage", "starts_ones")
                   for C in (3, 70) for bits in (8, 32) for base in (True, False)]


def compact_corrupt(kind, C, bits, base):
    """(the corrupt payload's uploads with the streams of the VALID entries, the payload)."""
    p = I.corrupt(kind, C, bits, base)
    return [UM.pack(u, bits) for u in UM.split(p)], p


def random_words(base, seed=300):
    """One client (weight 1, mn 1, scale 0.5, bits 8: aggregate_inputs.racy's setting) whose stream is random words."""
    p = I.racy("zero_idx", base, seed)
    u = UM.pack(UM.split(p)[0], 8)
    u.packed = np.random.default_rng(seed).integers(0, 1 << 32, u.packed.size, dtype=np.uint64).astype(np.uint32)
    return [u], p


def model_with_racy(ups, p, mode):
    n = p.table.span_per_client + I.PAD
    out, racy = np.full(n, I.SENTINEL, np.float32), np.zeros(n, bool)
    c = UM.aggregate(ups, UM.one_layout_segs(p), p.bits, p.weights, sum(p.weights), mode, out, base=p.base,
                     avg_mask=p.mask, kind="compact", racy=racy)
    return out, racy, c


@pytest.mark.parametrize("kind,C,bits,base", COMPACT_CORRUPT)
def test_compact_corrupt_starts_are_defined_and_change_the_result(kind, C, bits, base):
    ups, p = compact_corrupt(kind, C, bits, base)
    out, racy, c = model_with_racy(ups, p, O.AGG_RECIP)
    valid = I._valid(bits, C, base, 100 + list(I.CORRUPTIONS).index(kind))
    ref, _, _, _ = both_models(valid, "compact")
    ins = np.zeros(out.size, bool)
    for off, n in zip(p.table.offsets, p.table.sizes):
        ins[off:off + n] = True
    assert np.all(out[~ins] == I.SENTINEL)
    assert (~racy[ins]).any()  # part of the result is defined (no client applies a position twice there) ...
    if kind in I.APPLIES_NOTHING:
        assert c.applied == 0
    else:
        assert c.applied > 0
    differs = ~((out == ref) | (np.isnan(out) & np.isnan(ref)))
    assert differs[ins & ~racy].any()  # ... and differs from the valid upload's where it is


@pytest.mark.parametrize("base", [True, False])
def test_compact_random_words_apply_and_drop(base):
    ups, p = random_words(base)
    out, racy, c = model_with_racy(ups, p, O.AGG_SUM)
    assert c.applied > 0 and c.dropped > 0 and racy.any() and not racy.all()


# -- encoded_to(keep_packed=True) -------------------------------------------------------------------------
def _tiny(seed):
    g = torch.Generator().manual_seed(seed)
    m = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Linear(1024, 6), nn.Linear(1100, 9))
    with torch.no_grad():
        for t in list(m.parameters()) + [m[1].running_mean, m[1].running_var]:
            t.copy_(torch.randn(t.shape, generator=g) * 0.05)
        m[1].running_var.abs_()
        m[1].num_batches_tracked.fill_(3 + seed)
    return m


def _uploads(backend, compact, bits=8, ratio=0.05, mode="weights", base=None, seeds=(1, 2, 3)):
    c = UpdateCodec(ratio, bits, mode, backend=backend, compact=compact)
    return [pickle.loads(pickle.dumps(c.encode(_tiny(s).state_dict(), base=base))) for s in seeds]


@pytest.mark.parametrize("bits", [8, 32])
def test_encoded_to_keeps_a_compact_stream_on_request(bits):
    u = _uploads(OracleBackend(), True, bits, seeds=(1,))[0]
    assert wire.format_of(u.header).version == 3 and u.stream_for(CPU)
    plain = u.encoded_to(CPU)
    assert plain.packed is None and plain.idx.numel() == u.header["total_k"]
    e = u.encoded_to(CPU, keep_packed=True)
    assert e.idx.numel() == 0 and e.packed.dtype == torch.uint32
    o, n = wire.sections(u.to_bytes(), u.header)[1]["packed"]
    np.testing.assert_array_equal(e.packed.numpy(), np.frombuffer(u.to_bytes(), "<u4", n // 4, o))
    np.testing.assert_array_equal(e.packed.numpy(), wire.pack_entries(plain.idx.numpy(), plain.vals.numpy(), bits))
    assert torch.equal(e.ustart, plain.ustart) and torch.equal(e.mn, plain.mn) and torch.equal(e.scale, plain.scale)
    if bits == 32:
        assert torch.equal(e.vals, plain.vals) and e.vals.dtype == torch.float32
    else:
        assert e.vals is None


def test_encoded_to_keyword_leaves_other_formats_alone():
    v2 = _uploads(OracleBackend(), False, seeds=(1,))[0]
    assert not v2.stream_for(CPU)
    e = v2.encoded_to(CPU, keep_packed=True)
    assert e.packed is None and e.idx.numel() == v2.header["total_k"]
    local = UpdateCodec(0.05, 8, "weights", backend=OracleBackend(), compact=True).encode(_tiny(1).state_dict())
    assert not local.stream_for(CPU)  # (never pickled, and its backend packs nothing: read from its entries)
    assert local.encoded_to(CPU, keep_packed=True).idx.numel() == local.header["total_k"]


# -- routing --------------------------------------------------------------------------------------------
WEIGHTS = [13, 0, 7]


def _same_modules(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype, k
        if sa[k].dtype == torch.float32:
            same_bits(sa[k].numpy().reshape(-1), sb[k].numpy().reshape(-1))
        else:
            assert torch.equal(sa[k], sb[k]), k


def _calls():
    n = len(UM.UploadsOraclePlan.calls)
    return lambda: UM.UploadsOraclePlan.calls[n:]


@pytest.mark.parametrize("params_only", [False, True], ids=["all", "params"])
@pytest.mark.parametrize("mode", ["weights", "delta"])
@pytest.mark.parametrize("bits", [8, 32])
@pytest.mark.parametrize("compact", [False, True], ids=["v2", "v3"])
def test_sparse_uploads_reaches_aggregate_uploads_once(compact, bits, mode, params_only, monkeypatch):
    g = _tiny(5)
    codec = UpdateCodec(0.05, bits, mode, backend=UM.UploadsOracleBackend(), compact=compact)
    base = codec.snapshot(g) if mode == "delta" else None
    ups = _uploads(UM.UploadsOracleBackend(), compact, bits, mode=mode, base=base)
    want = codec.aggregate(ups, WEIGHTS, g, base=base, mode="div", params_only=params_only)
    calls = _calls()

    def boom(*a, **k):
        raise AssertionError("the uploads route must not concatenate and call aggregate")
    monkeypatch.setattr(UM.UploadsOraclePlan, "aggregate", boom)
    got = codec.aggregate(ups, WEIGHTS, g, base=base, mode="div", params_only=params_only, sparse_uploads=True)
    assert calls() == ["compact" if compact else "entries"]
    _same_modules(got, want)


def _as_v1(u):
    h = {k: v for k, v in u.header.items() if k != "n_units"}
    e = u.encoded
    return CompressedUpdate(h, Encoded(e.idx, e.vals, e.mn, e.scale, None), u.raw)


def test_fallbacks_take_the_existing_route():
    g = _tiny(5)
    be = UM.UploadsOracleBackend()
    codec = UpdateCodec(0.05, 8, "weights", backend=be)
    v2 = _uploads(be, False)
    want = codec.aggregate(v2, WEIGHTS, g, mode="div")
    calls = _calls()
    # v1 uploads (no starts)
    v1 = [_as_v1(u) for u in v2]
    assert wire.format_of(v1[0].header).version == 1 and codec.sparse_uploads_plan(v1) is None
    _same_modules(codec.aggregate(v1, WEIGHTS, g, mode="div", sparse_uploads=True), want)
    # a dense round (ratio 1)
    dense_codec = UpdateCodec(1.0, 8, "weights", backend=be)
    dense = _uploads(be, False, ratio=1.0)
    assert dense_codec.sparse_uploads_plan(dense) is None
    _same_modules(dense_codec.aggregate(dense, WEIGHTS, g, mode="div", sparse_uploads=True),
                  dense_codec.aggregate(dense, WEIGHTS, g, mode="div"))
    # mixed formats: not one round, with or without the keyword
    mixed = [v2[0], _uploads(be, True, seeds=(2,))[0], v2[2]]
    for kw in ({}, {"sparse_uploads": True}):
        with pytest.raises(ValueError):
            codec.aggregate(mixed, WEIGHTS, g, mode="div", **kw)
    # a backend without the method
    plain = UpdateCodec(0.05, 8, "weights", backend=OracleBackend())
    assert plain.sparse_uploads_plan(v2) is None
    _same_modules(plain.aggregate(v2, WEIGHTS, g, mode="div", sparse_uploads=True), want)
    assert calls() == []


def _server(on, backend, compact, distributed=False):
    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.05, 8, "weights", backend
        codec_compact = compact
        codec_fused_aggregate = True
        codec_fused_sparse_uploads = on
    return Server(_tiny(5), [])


@pytest.mark.parametrize("compact", [False, True], ids=["v2", "v3"])
def test_server_switch(compact):
    be = UM.UploadsOracleBackend()
    ups = _uploads(be, compact)
    calls = _calls()
    want = _server(False, be, compact).aggregate(list(ups), WEIGHTS)
    assert calls() == []
    got = _server(True, be, compact).aggregate(list(ups), WEIGHTS)
    assert calls() == ["compact" if compact else "entries"]
    _same_modules(got, want)
    _same_modules(_server(True, OracleBackend(), compact).aggregate(list(ups), WEIGHTS), want)


def test_defaults_are_off():
    assert CompressionServerMixin.codec_fused_sparse_uploads is False


# -- the C ABI ------------------------------------------------------------------------------------------
def test_abi_11_exports_and_binds_aggregate_uploads():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 11 and lib.coalac_version() == 11
    fn = getattr(lib, "coalac_aggregate_uploads")
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17
    hdr = (Path(__file__).resolve().parents[1] / "include" / "coalac.h").read_text()
    decl = re.search(r"int coalac_aggregate_uploads\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == 17
    assert re.search(r"COALAC_AGGS_ENTRIES = 0, COALAC_AGGS_COMPACT = 1", hdr)
    assert (_lib.COALAC_AGGS_ENTRIES, _lib.COALAC_AGGS_COMPACT) == (0, 1)
    # no GPU needed for the argument checks that come before the device's
    assert fn(None, 1, 0, None, None, 0, None, None, None, None, None, ctypes.c_float(1), 0, None, None, None,
              None) == -1
    assert b"coalac_aggregate_uploads: plan is NULL" in lib.coalac_last_error()
