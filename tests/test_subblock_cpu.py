"""Block-wise dense quantisation with 256- and 1024-element blocks without a GPU: the model against the
4096-element one, the blob, the block order, the codec's refusals and the error ordering, with tests/subblock_model.py
as the codec backend. Every comparison is bit-exact."""
import copy
import pickle
import struct

import numpy as np
import pytest
import torch

from coala_amd.compression import CompressedUpdate, CompressionClientMixin, CompressionServerMixin, UpdateCodec, wire
from coala_amd.compression.spec import SegmentTable
from coala_amd.compression.validate import validate
from coala_amd.fl import LoopbackServer
from coala_amd.layouts import build_module
from tests import blockwise_model as BM
from tests import subblock_model as SM
from tests.blockwise_model import BlockOracleBackend
from tests.subblock_model import SubblockOracleBackend

UNIT = 4096
_STATES = {}


def _state(seed):
    if seed not in _STATES:
        _STATES[seed] = build_module("lenet", seed=seed).state_dict()
    return _STATES[seed]


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# -- the model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 3, 4, 8])
def test_model_at_4096_is_the_blockwise_model(bits):
    rng = np.random.default_rng(bits)
    sizes = [0, 1, 255, 4096, 4097, 2 * UNIT + 300]
    t = SegmentTable(sizes, 1.0, 1)
    flat = (rng.standard_normal(t.span) * 3).astype(np.float32)
    base = rng.standard_normal(t.span).astype(np.float32)
    for b in (None, base):
        got, want = SM.encode(flat, t.segs, bits, UNIT, base=b), BM.encode(flat, t.segs, bits, base=b)
        _bits_equal(got[0], want[0])
        _bits_equal(got[1], want[1])
        np.testing.assert_array_equal(got[2], want[2])
        np.testing.assert_array_equal(got[3], want[3])
        _bits_equal(SM.decode(got[3], got[0], got[1], t.segs, bits, t.span, UNIT, base=b),
                    BM.decode(want[3], want[0], want[1], t.segs, bits, t.span, base=b))


def test_block_count_and_table_against_hand_written_values():
    sizes = (0, 1, 255, 256, 257, 4097)
    assert [wire.block_count([n], 256) for n in sizes] == [0, 1, 1, 1, 2, 17]
    assert [wire.block_count([n], 1024) for n in sizes] == [0, 1, 1, 1, 1, 5]
    assert [wire.block_count([n], 4096) for n in sizes] == [0, 1, 1, 1, 1, 2]
    assert [wire.block_count([n]) for n in sizes] == [0, 1, 1, 1, 1, 2]  # (the default is the unit)
    assert wire.block_count(sizes, 256) == 22 and wire.block_count(sizes, 1024) == 9 and wire.block_count(sizes) == 6
    assert wire.block_table([0, 1, 257], 256).tolist() == [[0, 1], [1, 256], [257, 1]]
    assert wire.block_table([1025, 3], 1024).tolist() == [[0, 1024], [1024, 1], [1025, 3]]
    assert wire.block_table([4097]).tolist() == wire.block_table([4097], 4096).tolist() == [[0, 4096], [4096, 1]]
    assert wire.block_table([], 256).shape == (0, 2)
    t = wire.block_table(sizes, 256)
    assert len(t) == 22 and t[-1].tolist() == [sum(sizes) - 1, 1] and int(t[:, 1].sum()) == sum(sizes)


# -- the blob ---------------------------------------------------------------------------------------------
def _encode(bits, block, seed=1, backend=None):
    codec = UpdateCodec(1.0, bits, "weights", backend=backend or SubblockOracleBackend(), blockwise=True,
                        block_size=block)
    return codec, codec.encode(_state(seed))


@pytest.mark.parametrize("block", [256, 1024])
@pytest.mark.parametrize("bits", [2, 4])
def test_wire_round_trip(block, bits):
    codec, up = _encode(bits, block)
    h = up.header
    sizes = [e["n"] for e in h["entries"] if e["kind"] == "seg"]
    NB, P = wire.block_count(sizes, block), wire.dense_packed_words(sizes, bits)
    assert h["blockwise"] == block and h["n_blocks"] == NB > wire.block_count(sizes)
    assert up.encoded.mn.numel() == up.encoded.scale.numel() == NB and up.nbytes == 8 * NB + 4 * P + up.raw.nbytes
    blob = up.to_bytes()
    assert struct.unpack_from("<I", blob, 8)[0] == 5
    hh, sec = wire.sections(blob)
    assert hh["blockwise"] == block and sec["mn"][1] == sec["scale"][1] == 4 * NB and sec["packed"][1] == 4 * P
    validate(dict(hh), np.zeros(0, np.int32))
    # the sections are the model's
    t = SegmentTable(sizes, 1.0, 1)
    flat = np.zeros(t.span, np.float32)
    for e in h["entries"]:
        if e["kind"] == "seg":
            flat[e["off"]:e["off"] + e["n"]] = _state(1)[e["name"]].numpy().reshape(-1)
    mn, sc, codes, stream = SM.encode(flat, t.segs, bits, block)
    _, gmn, gsc, gidx, gvals, _, gust = wire.unpack(blob)
    assert gidx.size == 0 and gust is None
    _bits_equal(gmn, mn)
    _bits_equal(gsc, sc)
    np.testing.assert_array_equal(gvals, codes)
    np.testing.assert_array_equal(np.frombuffer(blob, "<u4", P, sec["packed"][0]), stream)
    ref = SM.decode(stream, mn, sc, t.segs, bits, t.span, block)
    want = codec.decode_state(up)
    for e in h["entries"]:
        if e["kind"] == "seg":
            _bits_equal(want[e["name"]].numpy().reshape(-1), ref[e["off"]:e["off"] + e["n"]])
    for back in (CompressedUpdate.from_bytes(blob), pickle.loads(pickle.dumps(up)), copy.deepcopy(up)):
        assert back.to_bytes() == blob and back.nbytes == up.nbytes and back.header["blockwise"] == block
        got = codec.decode_state(back)  # (the decoder takes the size from the header)
        for k in want:
            assert torch.equal(want[k], got[k]), k
    assert _encode(bits, block)[1].to_bytes() == blob  # equal payloads give equal bytes


def test_a_4096_blob_is_what_it_was():
    for bits in (2, 4, 8):
        old = UpdateCodec(1.0, bits, "weights", backend=BlockOracleBackend(), blockwise=True).encode(_state(1))
        assert _encode(bits, UNIT)[1].to_bytes() == old.to_bytes()
        assert _encode(bits, UNIT, backend=BlockOracleBackend())[1].to_bytes() == old.to_bytes()


def _with_header(blob, change):
    h = change(dict(wire.sections(blob)[0]))
    hj = wire.encode_header(h)
    end = 16 + struct.unpack_from("<I", blob, 12)[0]
    body = blob[end + -end % 16:]
    head = blob[:8] + struct.pack("<II", 5, len(hj)) + hj
    return head + b"\0" * (-len(head) % 16) + body


@pytest.mark.parametrize("block", [256, 1024])
def test_corrupt_blobs_are_rejected(block):
    blob = _encode(4, block)[1].to_bytes()
    assert CompressedUpdate.from_bytes(_with_header(blob, lambda h: h)).to_bytes() == blob  # (the helper is sound)
    for d in (1, -1):  # a wrong n_blocks
        with pytest.raises(ValueError, match="block count"):
            CompressedUpdate.from_bytes(_with_header(blob, lambda h: dict(h, n_blocks=h["n_blocks"] + d)))
    h = dict(wire.sections(blob)[0])
    with pytest.raises(ValueError, match="block count"):
        validate(dict(h, n_blocks=wire.block_count([e["n"] for e in h["entries"] if e["kind"] == "seg"])),
                 np.zeros(0, np.int32))  # (the 4096 count under another size)
    other = 1024 if block == 256 else 256
    with pytest.raises(ValueError, match="block count"):  # the header of one size over the sections of another
        CompressedUpdate.from_bytes(_with_header(blob, lambda h: dict(h, blockwise=other)))
    for size in (64, 2048, 8192, 0, True):
        with pytest.raises(ValueError, match="block size"):
            CompressedUpdate.from_bytes(_with_header(blob, lambda h: dict(h, blockwise=size)))
        with pytest.raises(ValueError, match="block size"):
            validate(dict(h, blockwise=size), np.zeros(0, np.int32))
    # a range section of the wrong length: wire.pack counts each section against the header
    _, mn, sc, _, _, raw, _ = wire.unpack(blob)
    o, n = wire.sections(blob)[1]["packed"]
    packed = np.frombuffer(blob, "<u4", n // 4, o)
    assert wire.pack(h, mn, sc, None, None, raw, packed=packed) == blob
    for bad_mn, bad_sc in ((mn[:-1], sc), (mn, sc[:-1]), (np.append(mn, 0), sc), (mn[:wire.block_count([1])], sc)):
        with pytest.raises(ValueError, match="section"):
            wire.pack(h, bad_mn, bad_sc, None, None, raw, packed=packed)
    for name in ("mn", "scale"):  # ... and a blob cut inside one is truncated
        o, n = wire.sections(blob)[1][name]
        with pytest.raises(ValueError, match="truncated"):
            CompressedUpdate.from_bytes(blob[:o + n - 4])


# -- the codec's refusals ---------------------------------------------------------------------------------
def test_block_size_value_errors():
    be = SubblockOracleBackend()
    for size in (64, 2048, 8192, 0, True, "256", None):
        with pytest.raises(ValueError, match="block size"):
            UpdateCodec(1.0, 4, "weights", backend=be, blockwise=True, block_size=size)
    assert UpdateCodec(backend=be).block_size == UNIT
    assert CompressionClientMixin.codec_block_size == UNIT and CompressionServerMixin.codec_download_block_size == UNIT
    for size in (256, 1024):
        with pytest.raises(ValueError, match="stochastic"):
            UpdateCodec(1.0, 4, "weights", backend=be, blockwise=True, block_size=size, stochastic=True)
        codec = UpdateCodec(1.0, 4, "delta", backend=be, blockwise=True, block_size=size)
        snap = codec.snapshot(_state(2))
        with pytest.raises(ValueError, match="error feedback"):
            codec.encode(_state(1), base=snap, residual=codec.new_residual(_state(1)))
        old = UpdateCodec(1.0, 4, "weights", backend=BlockOracleBackend(), blockwise=True, block_size=size)
        with pytest.raises(ValueError, match="encode_block_g"):  # a backend whose plan lacks the new methods
            old.encode(_state(1))
    UpdateCodec(1.0, 4, "weights", backend=be, blockwise=True, block_size=UNIT, stochastic=True)  # (4096: as before)


def test_mixed_block_sizes_are_decoded_one_by_one_and_one_size_is_fused():
    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "weights", SubblockOracleBackend()
        codec_fused_aggregate = codec_fused_dense_aggregate = True

    from coala_amd.fl.strategies import federated_averaging
    g = build_module("lenet", seed=5)
    server = Server(copy.deepcopy(g), [])

    def enc(block, seed):
        return pickle.loads(pickle.dumps(_encode(4, block, seed)[1]))
    calls = SM.SubblockOraclePlan.calls
    ups = [enc(256, 1), enc(256, 2), enc(256, 3)]
    fused = server.aggregate(list(ups), [1, 3, 2])
    assert SM.SubblockOraclePlan.calls == calls + 1  # one dense aggregate, with the header's size
    want = federated_averaging([server._decode_upload(u) for u in ups], [1, 3, 2])
    for a, b in zip(fused.state_dict().values(), want.state_dict().values()):
        assert torch.equal(a, b)
    calls = SM.SubblockOraclePlan.calls
    mixed = [enc(256, 1), enc(1024, 2), enc(UNIT, 3)]
    with pytest.raises(ValueError):
        server._codec().aggregate(mixed, [1, 3, 2], g, dense_kernel=True)
    got = server.aggregate(list(mixed), [1, 3, 2])
    assert SM.SubblockOraclePlan.calls == calls  # decoded upload by upload
    want = federated_averaging([server._decode_upload(u) for u in mixed], [1, 3, 2])
    for a, b in zip(got.state_dict().values(), want.state_dict().values()):
        assert torch.equal(a, b)


# -- what the knob buys -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def error_table():
    rng = np.random.default_rng(20)
    data = {"normal": rng.standard_normal(1 << 18).astype(np.float32),
            "student_t3": rng.standard_t(3, 1 << 18).astype(np.float32)}
    return {(name, bits): [SM.rms_error(x, bits, g) for g in (256, 1024, 4096)]
            for name, x in data.items() for bits in (2, 4)}


@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("name", ["normal", "student_t3"])
def test_smaller_blocks_have_strictly_smaller_error(error_table, name, bits):
    e256, e1024, e4096 = error_table[(name, bits)]
    print(f"{name} bits {bits}: RMS error relative to 4096: G=1024 {e1024 / e4096:.3f}, G=256 {e256 / e4096:.3f}")
    assert e256 < e1024 < e4096
