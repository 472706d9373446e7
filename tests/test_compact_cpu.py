"""The compact upload payload (wire v3) without a GPU: the host model of the format
(wire.pack_entries / wire.unpack_entries), the carrier, the blob and the hook mixins, with the CPU oracle as the
codec backend. Every comparison is bit-exact: the repacking is lossless."""
import copy
import pickle
import struct
from collections import OrderedDict

import numpy as np
import pytest
import torch

from coala_amd.compression import (CompressedUpdate, CompressionClientMixin, CompressionServerMixin, Encoded,
                                   UpdateCodec, wire)
from coala_amd.compression.spec import RAW_BITS, UNIT, SegmentTable, k_for
from coala_amd.fl import LoopbackClient, LoopbackServer
from coala_amd.layouts import build_module
from tests.ef_model import EFOracleBackend
from tests.oracle_backend import OracleBackend

HAND = [1, 5, 4095, 4096, 4097, 8193, 20000]


def _state(layout, seed):
    if layout == "hand":
        g = torch.Generator().manual_seed(seed)
        return OrderedDict((f"t{i}", torch.randn(n, generator=g)) for i, n in enumerate(HAND))
    return build_module(layout, seed=seed).state_dict()


_STATES = {}


def _pair(layout):
    """(trained state, global state) of a layout, made once."""
    if layout not in _STATES:
        _STATES[layout] = (_state(layout, 1), _state(layout, 2))
    return _STATES[layout]


def _encode(layout, ratio, bits, compact):
    codec = UpdateCodec(ratio, bits, "delta", backend=OracleBackend(), compact=compact)
    state, base = _pair(layout)
    snap = codec.snapshot(base)
    return codec, snap, codec.encode(state, base=snap)


def _expected_nbytes(u):
    h = u.header
    P = (h["total_k"] * (12 + (0 if h["bits"] == RAW_BITS else h["bits"])) + 31) // 32
    return (8 * h["n_segments"] + 4 * P + (4 * h["total_k"] if h["bits"] == RAW_BITS else 0) + 4 * h["n_units"]
            + u.raw.nbytes)


# -- round trip through the wire ----------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 4, 5, 8, 32])
@pytest.mark.parametrize("ratio", [0.01, 0.3, 0.9])
@pytest.mark.parametrize("layout", ["lenet", "resnet18_split_cut4", "hand"])
def test_round_trip_through_the_wire(layout, ratio, bits):
    codec, snap, plain = _encode(layout, ratio, bits, False)
    _, _, comp = _encode(layout, ratio, bits, True)
    assert comp.header.get("compact") is True and "compact" not in plain.header
    blob = comp.to_bytes()
    assert struct.unpack_from("<I", blob, 8)[0] == 3
    back = pickle.loads(pickle.dumps(comp))
    for f in Encoded.FIELDS:
        a, b = getattr(back.encoded, f), getattr(plain.encoded, f)
        assert a.dtype == b.dtype and torch.equal(a, b), f
    # the blob's shape
    assert comp.nbytes == back.nbytes == _expected_nbytes(comp)
    if comp.header["total_k"] >= 32:
        assert comp.nbytes < plain.nbytes
    assert comp.compression_ratio > plain.compression_ratio or comp.header["total_k"] < 32
    h, sec = wire.sections(blob)
    assert "idx" not in sec and ("vals" in sec) == (bits == 32)
    o, n = sec["packed"]
    K, w = h["total_k"], 12 + (0 if bits == 32 else bits)
    assert o % 16 == 0 and n == 4 * ((K * w + 31) // 32)
    packed = np.frombuffer(blob, dtype="<u4", count=n // 4, offset=o)
    np.testing.assert_array_equal(packed, wire.pack_entries(plain.encoded.idx.numpy(), plain.encoded.vals.numpy(), bits))
    np.testing.assert_array_equal(packed, comp.packed.numpy())
    stream = np.unpackbits(packed.view(np.uint8), bitorder="little")
    assert not stream[K * w:].any()  # padding bits are zero
    if ratio == 0.01:  # equal payloads give equal bytes (a second encode of the same state)
        assert _encode(layout, ratio, bits, True)[2].to_bytes() == blob
    # both decode to the same tensors
    want = codec.decode_state(pickle.loads(pickle.dumps(plain)), base=snap)
    got = codec.decode_state(back, base=snap)
    assert list(want) == list(got)
    for k in want:
        assert want[k].dtype == got[k].dtype and torch.equal(want[k], got[k]), k


def test_deepcopy_shares_the_packed_buffer():
    _, _, comp = _encode("lenet", 0.3, 4, True)
    p = comp.packed
    twin = copy.deepcopy(comp)
    assert twin.packed is p and twin.to_bytes() is comp.to_bytes()


# -- the format functions directly --------------------------------------------------------------------
def _starts(idx, ns, ks):
    out, o = [], 0
    for n, k in zip(ns, ks):
        seg = idx[o:o + k]
        o += k
        out += [int(np.searchsorted(seg, u * UNIT)) for u in range((n + UNIT - 1) // UNIT)]
    return np.array(out, dtype=np.int32)


def _bitwise_pack(idx, vals, w):
    """The format, literally: bit t of the stream is bit t % 32 of word t // 32."""
    words = [0] * ((len(idx) * w + 31) // 32)
    for j, (i, v) in enumerate(zip(idx.tolist(), vals.tolist())):
        field = (i & 0xFFF) | ((v << 12) if w > 12 else 0)
        for b in range(w):
            t = j * w + b
            words[t // 32] |= ((field >> b) & 1) << (t % 32)
    return np.array(words, dtype=np.uint32)


@pytest.mark.parametrize("bits", [1, 2, 3, 4, 5, 6, 7, 8, 32])  # every field width from 12 to 20 (32 -> 12)
@pytest.mark.parametrize("K", [0, 1, 31, 32, 33])
def test_pack_entries_is_the_documented_bit_stream(K, bits):
    rng = np.random.default_rng(K * 100 + bits)
    n = 3 * UNIT + 77  # one segment, its last unit partial
    idx = np.sort(rng.choice(n, K, replace=False)).astype(np.int32)
    vals = rng.integers(0, 1 << min(bits, 8), K).astype(np.uint8)
    w = 12 + (0 if bits == 32 else bits)
    packed = wire.pack_entries(idx, vals, bits)
    assert packed.dtype == np.uint32 and packed.size == wire.packed_words(K, bits) == (K * w + 31) // 32
    np.testing.assert_array_equal(packed, _bitwise_pack(idx, vals, w))
    if K:
        i2, v2 = wire.unpack_entries(packed, _starts(idx, [n], [K]), [n], [K], bits)
        np.testing.assert_array_equal(i2, idx)
        np.testing.assert_array_equal(v2, vals if bits != 32 else np.zeros(K, np.uint8))


def test_unit_without_entries_and_partial_last_unit():
    # segment 0: 3 units, the middle one keeps nothing; segment 1: a partial only unit; segment 2: last unit partial
    ns, ks = [3 * UNIT, 100, UNIT + 5], [6, 3, 4]
    idx = np.array([0, 7, 4095, 8192, 9000, 12287, 1, 50, 99, 4095, 4096, 4099, 4100], dtype=np.int32)
    vals = np.arange(13, dtype=np.uint8) * 3
    ust = _starts(idx, ns, ks)
    assert ust.tolist() == [0, 3, 3, 0, 0, 1]
    i2, v2 = wire.unpack_entries(wire.pack_entries(idx, vals, 6), ust, ns, ks, 6)
    np.testing.assert_array_equal(i2, idx)
    np.testing.assert_array_equal(v2, vals)


def test_unpack_entries_clamps_wrong_starts():
    rng = np.random.default_rng(5)
    ns = HAND
    ks = [k_for(n, 0.3) for n in ns]
    idx = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for n, k in zip(ns, ks)]).astype(np.int32)
    packed = wire.pack_entries(idx, np.zeros(idx.size, np.uint8), 8)
    seg_of = np.repeat(np.arange(len(ns)), ks)
    for ust in (_starts(idx, ns, ks) + 1, rng.integers(-2 ** 31, 2 ** 31 - 1, len(_starts(idx, ns, ks))).astype(np.int32)):
        i2, _ = wire.unpack_entries(packed, ust, ns, ks, 8)
        assert i2.size == idx.size and (i2 >= 0).all()
        assert (i2 < (np.array(ns)[seg_of] + UNIT - 1) // UNIT * UNIT).all()
    with pytest.raises(ValueError):
        wire.unpack_entries(packed[:-1], _starts(idx, ns, ks), ns, ks, 8)
    with pytest.raises(ValueError):
        wire.unpack_entries(packed, _starts(idx, ns, ks)[:-1], ns, ks, 8)


# -- rejection of corrupt blobs -----------------------------------------------------------------------
def _reblob(blob, **changes):
    """The v3 blob with sections replaced (packed / ustart) or its header changed (header=fn)."""
    h, mn, sc, idx, vals, raw, ust = wire.unpack(blob)
    _, sec = wire.sections(blob)
    o, n = sec["packed"]
    packed = np.frombuffer(blob, dtype="<u4", count=n // 4, offset=o)
    hdr = changes.get("header", lambda x: x)(dict(h))
    return wire.pack(hdr, mn, sc, None, vals if h["bits"] == 32 else None, raw,
                     ustart=changes.get("ustart", ust), packed=changes.get("packed", packed))


def test_from_bytes_rejects_corrupt_compact_blobs():
    _, _, comp = _encode("hand", 0.3, 8, True)
    blob = comp.to_bytes()
    assert CompressedUpdate.from_bytes(_reblob(blob)).to_bytes() == blob  # (the helper rebuilds a good blob)
    _, sec = wire.sections(blob)
    o, n = sec["packed"]
    with pytest.raises(ValueError, match="truncated"):  # the blob ends inside the packed section
        CompressedUpdate.from_bytes(blob[:o + n // 2])
    # a v3 header without n_units
    h = dict(wire.unpack(blob)[0])
    del h["n_units"]
    hj = wire.encode_header(h)
    cut = blob[:8] + struct.pack("<II", 3, len(hj)) + hj + blob[16 + struct.unpack_from("<I", blob, 12)[0]:]
    with pytest.raises(ValueError, match="n_units"):
        CompressedUpdate.from_bytes(cut)
    # a low-12 field altered: two neighbouring entries of one unit swap their positions
    idx, vals = comp.encoded.idx.numpy().copy(), comp.encoded.vals.numpy()
    j = next(j for j in range(idx.size - 1) if 0 < idx[j] < idx[j + 1] and idx[j] >> 12 == idx[j + 1] >> 12)
    idx[j], idx[j + 1] = idx[j + 1], idx[j]
    with pytest.raises(ValueError, match="strictly increasing"):
        CompressedUpdate.from_bytes(_reblob(blob, packed=wire.pack_entries(idx, vals, 8)))
    # the starts shifted by one
    with pytest.raises(ValueError):
        CompressedUpdate.from_bytes(_reblob(blob, ustart=comp.encoded.ustart.numpy() + 1))
    # a version word that disagrees with the header
    with pytest.raises(ValueError):
        CompressedUpdate.from_bytes(blob[:8] + struct.pack("<I", 2) + blob[12:])


# -- backward compatibility ---------------------------------------------------------------------------
def test_v1_and_v2_blobs_still_load():
    h = {"ratio": 0.25, "bits": 8, "mode": "delta", "n_segments": 2, "total_k": 3,
         "entries": [{"name": "w", "dtype": "float32", "shape": [2, 3], "kind": "seg", "seg": 0, "off": 0, "n": 6},
                     {"name": "b", "dtype": "float32", "shape": [4], "kind": "seg", "seg": 1, "off": 32, "n": 4}]}
    mn, sc = np.array([-0.5, 0.0], np.float32), np.array([0.01, 0.0], np.float32)
    idx, vals = np.array([1, 4, 2], np.int32), np.array([0, 255, 7], np.uint8)
    v1 = wire.pack(h, mn, sc, idx, vals, b"")
    v2 = wire.pack(dict(h, n_units=2), mn, sc, idx, vals, b"", ustart=np.array([0, 0], np.int32))
    assert struct.unpack_from("<I", v1, 8)[0] == 1 and struct.unpack_from("<I", v2, 8)[0] == 2
    for blob, ust in ((v1, None), (v2, [0, 0])):
        u = CompressedUpdate.from_bytes(blob)
        assert u.packed is None and u.encoded.idx.tolist() == [1, 4, 2] and u.encoded.vals.tolist() == [0, 255, 7]
        assert (u.encoded.ustart is None) if ust is None else (u.encoded.ustart.tolist() == ust)
        assert u.nbytes == 8 * 2 + 5 * 3 + (8 if ust else 0)
        _, sec = wire.sections(blob)
        assert "idx" in sec and "packed" not in sec


@pytest.mark.parametrize("bits", [8, 32])
def test_compact_at_ratio_one_is_todays_dense_blob(bits):
    _, _, plain = _encode("lenet", 1.0, bits, False)
    _, _, comp = _encode("lenet", 1.0, bits, True)
    assert "compact" not in comp.header and comp.packed is None
    assert comp.to_bytes() == plain.to_bytes() and comp.nbytes == plain.nbytes


def test_all_kept_layout_below_ratio_one_stays_v2():
    """Every segment keeps all its elements (k == n) although ratio < 1: a dense plan, nothing to pack."""
    codec = UpdateCodec(0.9, 8, "weights", backend=OracleBackend(), compact=True)
    u = codec.encode(OrderedDict(a=torch.tensor([1.0]), b=torch.tensor([2.0, 3.0])))
    assert "compact" not in u.header and struct.unpack_from("<I", u.to_bytes(), 8)[0] == 2


def test_default_is_off_and_unchanged():
    assert UpdateCodec(backend=OracleBackend()).compact is False and CompressionClientMixin.codec_compact is False
    _, _, plain = _encode("lenet", 0.01, 8, False)
    assert struct.unpack_from("<I", plain.to_bytes(), 8)[0] == 2 and plain.packed is None


# -- the hook mixins in the loopback loop -------------------------------------------------------------
def _run(compact, fused=False, feedback=False, rounds=2):
    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.05, 4, "delta", EFOracleBackend()
        codec_compact, codec_error_feedback = compact, feedback

    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.05, 4, "delta", OracleBackend()
        codec_fused_aggregate = fused

    clients = [Client(f"c{i}", 10 + i, step_seed=i) for i in range(3)]
    server = Server(build_module("lenet", seed=5), clients)
    for r in range(rounds):
        server.round(r)
    return server.model.state_dict(), [c.upload_sizes for c in clients]


@pytest.mark.parametrize("fused,feedback", [(False, False), (True, False), (False, True)])
def test_loopback_run_is_bit_identical_and_smaller(fused, feedback):
    plain, plain_sizes = _run(False, fused, feedback)
    comp, comp_sizes = _run(True, fused, feedback)
    for (k, a), (k2, b) in zip(plain.items(), comp.items()):
        assert k == k2 and a.dtype == b.dtype and torch.equal(a, b), k
    for p, c in zip(plain_sizes, comp_sizes):
        assert len(p) == len(c) == 2 and all(x < y for x, y in zip(c, p))


def test_mixed_formats_fall_back_to_per_upload_decode():
    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.05, 8, "weights", OracleBackend()
        codec_fused_aggregate = True

    g = build_module("lenet", seed=5)
    ups = [UpdateCodec(0.05, 8, "weights", backend=OracleBackend(), compact=c).encode(
        build_module("lenet", seed=s).state_dict()) for c, s in ((True, 1), (False, 2))]
    ups = [pickle.loads(pickle.dumps(u)) for u in ups]
    server = Server(copy.deepcopy(g), [])
    mixed = server.aggregate(list(ups), [1, 3])
    with pytest.raises(ValueError, match="payload format"):
        server._codec().aggregate(ups, [1, 3], g)
    # ... and equals the aggregate of the same two updates both in the plain format
    ups[0] = pickle.loads(pickle.dumps(UpdateCodec(0.05, 8, "weights", backend=OracleBackend()).encode(
        build_module("lenet", seed=1).state_dict())))
    same = server.aggregate(list(ups), [1, 3])
    for a, b in zip(mixed.state_dict().values(), same.state_dict().values()):
        assert torch.equal(a, b)
