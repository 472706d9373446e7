"""Bit-packed dense codes (wire v4) without a GPU: the host model of the format
(wire.pack_dense_codes / wire.unpack_dense_codes), the blob, the carrier and the hook mixins, with the CPU oracle as
the codec backend. Every comparison is bit-exact: the repacking is lossless."""
import copy
import pickle
import struct

import numpy as np
import pytest
import torch

from coala_amd.compression import (CompressedModel, CompressedUpdate, CompressionClientMixin, CompressionServerMixin,
                                   Encoded, UpdateCodec, wire)
from coala_amd.fl import LoopbackClient, LoopbackServer
from coala_amd.layouts import build_module, fp32_sizes
from tests.ef_model import EFOracleBackend
from tests.oracle_backend import OracleBackend

SIZES = [1, 31, 32, 33, 0, 4095, 4096, 4097, 2 * 4096 + 5]


# -- the format model ---------------------------------------------------------------------------------
def _bitwise_pack(vals, sizes, b):
    """The format, literally: entry e of segment s at bits [e b, (e + 1) b) of the segment's own words, bit t of a
    stream being bit t % 32 of word t // 32."""
    words, o = [], 0
    for n in sizes:
        seg = [0] * ((n * b + 31) // 32)
        for e in range(n):
            for i in range(b):
                t = e * b + i
                seg[t // 32] |= ((int(vals[o + e]) >> i) & 1) << (t % 32)
        words += seg
        o += n
    return np.array(words, dtype=np.uint32)


@pytest.mark.parametrize("b", range(1, 9))
def test_format_model_round_trip(b):
    rng = np.random.default_rng(b)
    vals = rng.integers(0, 1 << b, sum(SIZES)).astype(np.uint8)
    packed = wire.pack_dense_codes(vals, SIZES, b)
    W = [(n * b + 31) // 32 for n in SIZES]
    assert packed.dtype == np.uint32 and packed.size == wire.dense_packed_words(SIZES, b) == sum(W)
    np.testing.assert_array_equal(packed, _bitwise_pack(vals, SIZES, b))
    # every segment starts at pw_s = the words of those before it, and its padding bits are zero
    pw = np.cumsum(W) - W
    o = 0
    for n, w, p in zip(SIZES, W, pw):
        np.testing.assert_array_equal(packed[p:p + w], wire.pack_dense_codes(vals[o:o + n], [n], b))
        stream = np.unpackbits(packed[p:p + w].view(np.uint8), bitorder="little")
        assert not stream[n * b:].any()
        o += n
    assert W[4] == 0 and pw[5] == pw[4]  # the empty segment owns no word
    np.testing.assert_array_equal(wire.unpack_dense_codes(packed, SIZES, b), vals)
    # padding bits of a received stream are ignored
    dirty = packed.copy()
    for n, w, p in zip(SIZES, W, pw):
        if w and (n * b) % 32:
            dirty[p + w - 1] |= np.uint32((0xFFFFFFFF << ((n * b) % 32)) & 0xFFFFFFFF)
    np.testing.assert_array_equal(wire.unpack_dense_codes(dirty, SIZES, b), vals)
    with pytest.raises(ValueError, match="truncated"):
        wire.unpack_dense_codes(packed[:-1], SIZES, b)


def test_out_off_does_not_move_the_stream():
    rng = np.random.default_rng(3)
    sizes, off = [33, 4097, 70], [7, 100, 5000]
    buf = rng.integers(0, 32, 5100).astype(np.uint8)
    back_to_back = np.concatenate([buf[o:o + n] for n, o in zip(sizes, off)])
    packed = wire.pack_dense_codes(buf, sizes, 5, out_off=off)
    np.testing.assert_array_equal(packed, wire.pack_dense_codes(back_to_back, sizes, 5))
    out = np.full(5100, 0xA5, dtype=np.uint8)
    wire.unpack_dense_codes(packed, sizes, 5, out_off=off, out=out)
    own = np.zeros(5100, dtype=bool)
    for n, o in zip(sizes, off):
        own[o:o + n] = True
    np.testing.assert_array_equal(out[own], buf[own])
    assert (out[~own] == 0xA5).all()


def test_hand_computed_example_at_three_bits():
    # segment 0: codes 5, 2, 7 -> 9 bits in one word: 5 | 2 << 3 | 7 << 6 = 0x1D5
    # segment 1: twelve codes 1 2 3 4 5 6 7 0 1 2 3 4 -> 36 bits, two words from word 1 on. Entries 0..9 fill bits
    #   0..29: 1 | 2<<3 | 3<<6 | 4<<9 | 5<<12 | 6<<15 | 7<<18 | 0<<21 | 1<<24 | 2<<27 = 0x111F58D1; entry 10 (3 = 0b011)
    #   straddles: its low two bits are bits 30, 31 (| 0xC0000000), its high bit (0) is bit 0 of the next word; entry 11
    #   (4 = 0b100) sits at bits 1..3 of that word: 4 << 1 = 8
    vals = np.array([5, 2, 7, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4], dtype=np.uint8)
    packed = wire.pack_dense_codes(vals, [3, 12], 3)
    assert packed.tolist() == [0x1D5, 0xD11F58D1, 0x8]
    assert wire.dense_packed_words([3, 12], 3) == 3
    np.testing.assert_array_equal(wire.unpack_dense_codes(packed, [3, 12], 3), vals)


# -- the blob -----------------------------------------------------------------------------------------
_STATES = {}


def _pair(layout):
    if layout not in _STATES:
        _STATES[layout] = (build_module(layout, seed=1).state_dict(), build_module(layout, seed=2).state_dict())
    return _STATES[layout]


def _encode(layout, bits, pack, ratio=1.0, mode="weights"):
    codec = UpdateCodec(ratio, bits, mode, backend=OracleBackend(), pack_dense=pack)
    state, base = _pair(layout)
    snap = codec.snapshot(base) if mode == "delta" else None
    return codec, snap, codec.encode(state, base=snap)


@pytest.mark.parametrize("bits", [1, 4, 6, 7])
@pytest.mark.parametrize("layout", ["lenet", "resnet18_split_cut4"])
def test_blob_shape_and_round_trip(layout, bits):
    codec, _, plain = _encode(layout, bits, False)
    _, _, dp = _encode(layout, bits, True)
    assert dp.header.get("dense_packed") is True and "dense_packed" not in plain.header and plain.packed is None
    blob = dp.to_bytes()
    assert struct.unpack_from("<I", blob, 8)[0] == 4
    h, sec = wire.sections(blob)
    assert h["dense"] is True and h["dense_packed"] is True and "n_units" not in h
    assert list(sec) == ["mn", "scale", "packed"]
    sizes = [e["n"] for e in h["entries"] if e["kind"] == "seg"]
    T, P = len(sizes), sum((n * bits + 31) // 32 for n in sizes)
    pos = 16 + struct.unpack_from("<I", blob, 12)[0]
    for name, nbytes in (("mn", 4 * T), ("scale", 4 * T), ("packed", 4 * P)):
        pos += -pos % 16
        assert sec[name] == (pos, nbytes)
        pos += nbytes
    pos += -pos % 16
    assert dp.nbytes == 8 * T + 4 * P + dp.raw.nbytes == 8 * T + 4 * P + (len(blob) - pos)
    assert dp.nbytes < plain.nbytes
    packed = np.frombuffer(blob, dtype="<u4", count=P, offset=sec["packed"][0])
    np.testing.assert_array_equal(packed, wire.pack_dense_codes(plain.encoded.vals.numpy(), sizes, bits))
    np.testing.assert_array_equal(packed, dp.packed.numpy())
    assert _encode(layout, bits, True)[2].to_bytes() == blob  # equal payloads give equal bytes
    # from_bytes, pickle and deepcopy: the carrier's buffers and its decode are those of the unpacked carrier
    want = codec.decode_state(plain)
    twin = copy.deepcopy(dp)
    assert twin.packed is dp.packed and twin.to_bytes() is blob
    for back in (CompressedUpdate.from_bytes(blob), pickle.loads(pickle.dumps(dp)), copy.deepcopy(pickle.loads(pickle.dumps(dp)))):
        assert back.nbytes == dp.nbytes and back.to_bytes() == blob
        np.testing.assert_array_equal(back.packed.numpy(), packed)
        for f in ("vals", "mn", "scale"):
            a, b = getattr(back.encoded, f), getattr(plain.encoded, f)
            assert a.dtype == b.dtype and torch.equal(a, b), f
        assert back.encoded.idx.numel() == 0 and back.encoded.ustart is None
        got = codec.decode_state(back)
        assert list(got) == list(want)
        for k in want:
            assert want[k].dtype == got[k].dtype and torch.equal(want[k], got[k]), k


def test_resnet50_payload_sizes():
    sizes = fp32_sizes("resnet50_tv")
    T = len(sizes)
    assert (sum(sizes), T) == (25_610_152, 267)
    assert 8 * T + sum(sizes) == 25_612_288  # today: one byte per code, whatever the width
    table = {6: 19_209_752, 4: 12_807_212, 2: 6_404_676, 1: 3_203_408}
    for b, nbytes in table.items():
        assert 8 * T + 4 * wire.dense_packed_words(sizes, b) == nbytes, b


# -- the off switch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio,bits", [(1.0, 8), (1.0, 32), (0.3, 4)])
def test_option_changes_nothing_at_eight_or_32_bits_or_for_a_sparse_plan(ratio, bits):
    _, _, plain = _encode("lenet", bits, False, ratio)
    _, _, dp = _encode("lenet", bits, True, ratio)
    assert "dense_packed" not in dp.header and dp.packed is None
    assert dp.to_bytes() == plain.to_bytes() and dp.nbytes == plain.nbytes


def test_default_is_off():
    assert UpdateCodec(backend=OracleBackend()).pack_dense is False
    assert CompressionServerMixin.codec_download_pack is False and CompressionClientMixin.codec_pack_dense is False
    _, _, plain = _encode("lenet", 4, False)
    assert struct.unpack_from("<I", plain.to_bytes(), 8)[0] == 1 and plain.packed is None


# -- rejected blobs -----------------------------------------------------------------------------------
def _with_header(blob, version, change):
    h = change(dict(wire.sections(blob)[0]))
    hj = wire.encode_header(h)
    end = 16 + struct.unpack_from("<I", blob, 12)[0]
    body = blob[end + -end % 16:]  # from the first section on: it starts 16-byte aligned, before and after
    head = blob[:8] + struct.pack("<II", version, len(hj)) + hj
    return head + b"\0" * (-len(head) % 16) + body


def test_from_bytes_rejects_corrupt_dense_packed_blobs():
    _, _, dp = _encode("lenet", 4, True)
    blob = dp.to_bytes()
    assert CompressedUpdate.from_bytes(_with_header(blob, 4, lambda h: h)).to_bytes() == blob  # (the helper is sound)
    o, n = wire.sections(blob)[1]["packed"]
    with pytest.raises(ValueError, match="truncated"):  # the blob ends inside the packed section
        CompressedUpdate.from_bytes(blob[:o + n // 2])
    with pytest.raises(ValueError):  # version word 2, dense_packed header
        CompressedUpdate.from_bytes(blob[:8] + struct.pack("<I", 2) + blob[12:])
    with pytest.raises(ValueError):  # version word 1, dense_packed header
        CompressedUpdate.from_bytes(blob[:8] + struct.pack("<I", 1) + blob[12:])
    with pytest.raises(ValueError):  # dense_packed without dense

        def no_dense(h):
            del h["dense"]
            return h
        CompressedUpdate.from_bytes(_with_header(blob, 4, no_dense))
    for bits in (8, 32):
        with pytest.raises(ValueError):
            CompressedUpdate.from_bytes(_with_header(blob, 4, lambda h: dict(h, bits=bits)))
    with pytest.raises(ValueError):  # version word 4 on a plain dense blob
        plain = _encode("lenet", 4, False)[2].to_bytes()
        CompressedUpdate.from_bytes(plain[:8] + struct.pack("<I", 4) + plain[12:])
    # wire.pack refuses the same combinations
    z = np.zeros(1, np.float32)
    with pytest.raises(ValueError):
        wire.pack({"dense_packed": True, "n_segments": 1, "total_k": 1, "bits": 4, "entries": []}, z, z, None, None, b"",
                  packed=np.zeros(1, np.uint32))


# -- the hook mixins in the loopback loop -------------------------------------------------------------
def _download_run(pack, rounds=2):
    sizes = []

    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.05, 8, "delta", OracleBackend()

    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.05, 8, "delta", OracleBackend()
        codec_download, codec_download_bits, codec_download_pack = True, 4, pack

        def compression(self):
            super().compression()
            assert isinstance(self.model, CompressedModel)
            assert bool(self.model.update.header.get("dense_packed")) == pack
            sizes.append(self.model.nbytes)

    clients = [Client(f"c{i}", 5 + i, step_seed=i) for i in range(2)]
    server = Server(build_module("lenet", seed=7), clients, remote=True)
    states = []
    for r in range(rounds):
        server.round(r)
        states += [c._codec_base.flat.clone() for c in clients]                       # what each client decoded
        states += [t.clone() for m in server.uploaded.values() for t in m.state_dict().values()]  # each decoded upload
        states += [t.clone() for t in server.model.state_dict().values()]              # the aggregate
    return states, sizes, [c.download_sizes for c in clients]


def test_download_loop_is_bit_identical_and_smaller():
    plain, plain_sizes, plain_down = _download_run(False)
    packed, packed_sizes, packed_down = _download_run(True)
    assert len(plain) == len(packed)
    for a, b in zip(plain, packed):
        assert a.dtype == b.dtype and torch.equal(a, b)
    sizes = [p.numel() for p in build_module("lenet", seed=7).state_dict().values() if p.dtype == torch.float32]
    T, raw = len(sizes), plain_sizes[0] - 8 * len(sizes) - sum(sizes)
    assert packed_sizes == [8 * T + 4 * wire.dense_packed_words(sizes, 4) + raw] * 2  # CompressedModel.nbytes
    assert plain_sizes == [8 * T + sum(sizes) + raw] * 2
    for p, c in zip(plain_down, packed_down):  # ... and what the clients' calculate_model_size reports
        assert len(p) == len(c) == 2 and all(x < 0.6 * y for x, y in zip(c, p))


def _upload_run(pack, fused, feedback, rounds=2):
    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "delta", EFOracleBackend()
        codec_pack_dense, codec_error_feedback = pack, feedback

    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "delta", OracleBackend()
        codec_fused_aggregate = fused

    clients = [Client(f"c{i}", 10 + i, step_seed=i) for i in range(3)]
    server = Server(build_module("lenet", seed=5), clients)
    for r in range(rounds):
        server.round(r)
        assert all(bool(getattr(m, "header", {}).get("dense_packed")) == pack for m in server.uploaded.values() if fused)
    return server.model.state_dict(), [c.upload_sizes for c in clients]


@pytest.mark.parametrize("fused,feedback", [(False, False), (True, False), (False, True)])
def test_ratio_one_upload_loop_is_bit_identical_and_smaller(fused, feedback):
    plain, plain_sizes = _upload_run(False, fused, feedback)
    packed, packed_sizes = _upload_run(True, fused, feedback)
    for (k, a), (k2, b) in zip(plain.items(), packed.items()):
        assert k == k2 and a.dtype == b.dtype and torch.equal(a, b), k
    for p, c in zip(plain_sizes, packed_sizes):
        assert len(p) == len(c) == 2 and all(x < 0.6 * y for x, y in zip(c, p))


def test_mixed_formats_fall_back_to_per_upload_decode():
    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "weights", OracleBackend()
        codec_fused_aggregate = True

    g = build_module("lenet", seed=5)
    enc = lambda pack, seed: pickle.loads(pickle.dumps(UpdateCodec(1.0, 4, "weights", backend=OracleBackend(), pack_dense=pack)
                                                       .encode(build_module("lenet", seed=seed).state_dict())))
    ups = [enc(True, 1), enc(False, 2)]
    server = Server(copy.deepcopy(g), [])
    mixed = server.aggregate(list(ups), [1, 3])
    with pytest.raises(ValueError, match="payload format"):
        server._codec().aggregate(ups, [1, 3], g)
    same = server.aggregate([enc(False, 1), ups[1]], [1, 3])
    for a, b in zip(mixed.state_dict().values(), same.state_dict().values()):
        assert torch.equal(a, b)


def test_encoded_carries_no_stream_for_a_backend_without_decode_packed():
    """The test backends decode the host-unpacked codes: encoded_to hands those out, as for a plain dense carrier."""
    codec, _, dp = _encode("lenet", 4, True)
    back = pickle.loads(pickle.dumps(dp))
    enc = back.encoded_to(torch.device("cpu"), plan=codec.plan_for(tuple(back._seg_sizes()), torch.device("cpu")))
    assert isinstance(enc, Encoded) and enc.packed is None and enc.vals.dtype == torch.uint8
