"""Rotated block-wise quantisation (wire v6) without a GPU: the model's own properties, the blob, the
codec's refusals and seeds, aggregation and the mixins, and the error ordering, with tests/rot_model.py as the codec
backend. Every comparison of payloads is bit-exact."""
import copy
import pickle
import struct
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

from coala_amd.compression import CompressedUpdate, CompressionClientMixin, CompressionServerMixin, UpdateCodec, wire
from coala_amd.compression.spec import SegmentTable, sr_call_seed
from coala_amd.fl import LoopbackClient, LoopbackServer
from coala_amd.layouts import build_module
from tests import blockwise_model as BM
from tests import rot_model as RM
from tests import sr_model as SM
from tests.blockwise_model import BlockOracleBackend
from tests.rot_model import RotOracleBackend
from tests.sr_model import SROracleBackend

UNIT = 4096
_STATES = {}


def _state(seed):
    """A small state: full units, ragged ends, small tensors and a passthrough counter."""
    if seed not in _STATES:
        g = torch.Generator().manual_seed(seed)
        shapes = {"a.weight": (3, UNIT), "a.bias": (300,), "b.weight": (2, UNIT + 9), "b.bias": (UNIT,), "c": (1,)}
        st = OrderedDict((k, torch.randn(s, generator=g) * 0.1) for k, s in shapes.items())
        st["steps"] = torch.tensor(seed, dtype=torch.int64)
        _STATES[seed] = st
    return _STATES[seed]


def _lenet(seed):
    return build_module("lenet", seed=seed).state_dict()


def _bits_equal(a, b):
    np.testing.assert_array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# -- the model --------------------------------------------------------------------------------------------
def test_transform_twice_is_the_identity_on_small_integers():
    rng = np.random.default_rng(1)
    x = rng.integers(-64, 65, size=(3, UNIT)).astype(np.float32)  # |every intermediate| <= 2^18: exact in fp32
    assert np.array_equal(RM.hadamard(RM.hadamard(x)), x)  # (as values: a zero may come back as -0.0)
    c0 = np.array([0, 4096, (1 << 32) - 100], dtype=np.uint64)
    s = RM.signs(x, 77, c0)
    assert np.array_equal(np.abs(s), np.abs(x)) and 0.4 < np.mean(s != x) < 0.6
    _bits_equal(RM.signs(s, 77, c0), x)
    assert np.array_equal(RM.signs(RM.hadamard(RM.hadamard(RM.signs(x, 77, c0))), 77, c0), x)


def test_transform_against_the_matrix():
    # the stages are the Sylvester matrix H[i, j] = (-1)^popcount(i & j): checked on unit vectors and one dense row
    x = np.zeros((3, UNIT), np.float32)
    x[0, 0], x[1, 5], x[2] = 64.0, 64.0, 1.0
    y = RM.hadamard(x)
    j = np.arange(UNIT)
    pop5 = np.array([bin(v & 5).count("1") for v in j])
    assert np.array_equal(y[0], np.ones(UNIT, np.float32))
    assert np.array_equal(y[1], np.where(pop5 % 2 == 0, 1.0, -1.0).astype(np.float32))
    assert y[2, 0] == 64.0 and not y[2, 1:].any()


def test_signs_follow_the_position_across_a_2_32_boundary():
    x = np.ones(UNIT, np.float32)
    c0 = (1 << 32) - 1000  # (a unit whose positions cross 2^32: the key's high word changes inside it)
    s = RM.signs(x, 123, [c0])[0]
    want = np.where(SM.sr_u24(123, np.uint64(c0) + np.arange(UNIT, dtype=np.uint64)) & 0x800000, -1.0, 1.0)
    assert np.array_equal(s, want.astype(np.float32))
    assert not np.array_equal(RM.signs(x, 123, [c0 + (1 << 32)])[0], s)  # (the high word counts)
    # ... and the quantised payload of such a unit follows: the stochastic draws use the same positions
    segs = np.array([[c0, UNIT, UNIT, 0]], dtype=np.int64)
    y = RM.hadamard(RM.signs(np.arange(UNIT, dtype=np.float32), 123, [c0]))[0]
    mn, sc = BM.encode(y, np.array([[0, UNIT, UNIT, 0]]), 4)[:2]
    assert np.array_equal(SM.sr_codes(y, mn[0], sc[0], 4, 9, c0), SM.sr_codes(y, mn[0], sc[0], 4, 9, int(segs[0, 0])))


@pytest.mark.parametrize("bits", [1, 3, 8])
def test_a_plan_of_short_segments_is_the_blockwise_payload(bits):
    rng = np.random.default_rng(bits)
    t = SegmentTable([0, 1, 255, 4095, 300], 1.0, 1)
    flat = rng.standard_normal(t.span).astype(np.float32)
    base = rng.standard_normal(t.span).astype(np.float32)
    for b in (None, base):
        for got, want in ((RM.encode(flat, t.segs, bits, 9, base=b), BM.encode(flat, t.segs, bits, base=b)),
                          (RM.encode(flat, t.segs, bits, 9, seed=5, base=b), SM.encode_block(flat, t.segs, bits, 5, base=b))):
            _bits_equal(got[0], want[0])
            _bits_equal(got[1], want[1])
            np.testing.assert_array_equal(got[3], want[3])
        mn, sc, _, stream = RM.encode(flat, t.segs, bits, 9, base=b)
        got, want = RM.decode(stream, mn, sc, t.segs, bits, t.span, 9, base=b), BM.decode(stream, mn, sc, t.segs, bits,
                                                                                          t.span, base=b)
        for off, n, _, _ in t.segs.tolist():
            _bits_equal(got[off:off + n], want[off:off + n])


def test_full_units_are_rotated_and_ragged_ones_are_not():
    rng = np.random.default_rng(3)
    t = SegmentTable([UNIT + 100], 1.0, 1)
    flat = rng.standard_t(3, t.span).astype(np.float32)
    mn, sc, codes, _ = RM.encode(flat, t.segs, 4, 11)
    bmn, bsc, bcodes, _ = BM.encode(flat, t.segs, 4)
    assert mn[0] != bmn[0] and not np.array_equal(codes[:UNIT], bcodes[:UNIT])
    _bits_equal(mn[1:], bmn[1:])
    _bits_equal(sc[1:], bsc[1:])
    np.testing.assert_array_equal(codes[UNIT:], bcodes[UNIT:])


# -- the blob ---------------------------------------------------------------------------------------------
def _codec(bits=4, mode="weights", **kw):
    return UpdateCodec(1.0, bits, mode, backend=kw.pop("backend", None) or RotOracleBackend(), blockwise=True,
                       rotate=True, **kw)


def _flat_of(h, state):
    sizes = [e["n"] for e in h["entries"] if e["kind"] == "seg"]
    t = SegmentTable(sizes, 1.0, 1)
    flat = np.zeros(t.span, np.float32)
    for e in h["entries"]:
        if e["kind"] == "seg":
            flat[e["off"]:e["off"] + e["n"]] = state[e["name"]].numpy().reshape(-1)
    return t, flat


@pytest.mark.parametrize("stochastic", [False, True])
@pytest.mark.parametrize("bits", [2, 4])
def test_wire_round_trip(bits, stochastic):
    codec = _codec(bits, rotate_seed=5, stochastic=stochastic, seed=6)
    up = codec.encode(_state(1))
    h = up.header
    rot_seed = sr_call_seed(5 ^ UpdateCodec.ROTATE_DOMAIN, 0)
    assert h["rotate"] == rot_seed and h["blockwise"] == UNIT and wire.format_of(h) is wire.FORMATS[5]
    t, flat = _flat_of(h, _state(1))
    U, P = int(t.n_units), wire.dense_packed_words(t.segs[:, 1], bits)
    assert h["n_blocks"] == U and up.nbytes == 8 * U + 4 * P + up.raw.nbytes  # (version 5's size)
    blob = up.to_bytes()
    assert struct.unpack_from("<I", blob, 8)[0] == 6
    mn, sc, codes, stream = RM.encode(flat, t.segs, bits, rot_seed, seed=sr_call_seed(6, 0) if stochastic else None)
    hh, gmn, gsc, gidx, gvals, _, gust = wire.unpack(blob)
    assert hh["rotate"] == rot_seed and gidx.size == 0 and gust is None
    _bits_equal(gmn, mn)
    _bits_equal(gsc, sc)
    np.testing.assert_array_equal(gvals, codes)
    ref = RM.decode(stream, mn, sc, t.segs, bits, t.span, rot_seed)
    want = codec.decode_state(up)
    for e in h["entries"]:
        if e["kind"] == "seg":
            _bits_equal(want[e["name"]].numpy().reshape(-1), ref[e["off"]:e["off"] + e["n"]])
    plain = UpdateCodec(1.0, bits, "weights", backend=RotOracleBackend())  # (a decoder has no switch)
    for back in (CompressedUpdate.from_bytes(blob), pickle.loads(pickle.dumps(up)), copy.deepcopy(up)):
        assert back.to_bytes() == blob and back.nbytes == up.nbytes and back.header["rotate"] == rot_seed
        got = plain.decode_state(back)
        for k in want:
            assert torch.equal(want[k], got[k]), k
    # the seed is used: under another one the decode is further from the input
    wrong = RM.decode(stream, mn, sc, t.segs, bits, t.span, rot_seed + 1)
    assert np.abs(wrong - flat).mean() > np.abs(ref - flat).mean()


def test_unrotated_blobs_are_what_they_were():
    kinds = [dict(), dict(pack_dense=True), dict(blockwise=True), dict(blockwise=True, stochastic=True, seed=3),
             dict(blockwise=True, block_size=256)]
    from tests.subblock_model import SubblockOracleBackend
    for kw in kinds:
        be = SubblockOracleBackend if "block_size" in kw else RotOracleBackend
        old = SubblockOracleBackend if "block_size" in kw else SROracleBackend
        new = UpdateCodec(1.0, 4, "weights", backend=be(), rotate=False, rotate_seed=99, **kw).encode(_state(1))
        was = UpdateCodec(1.0, 4, "weights", backend=old(), **kw).encode(_state(1))
        assert "rotate" not in new.header and new.to_bytes() == was.to_bytes(), kw
    for ratio, kw in ((0.1, dict()), (0.1, dict(compact=True))):  # versions 2 and 3
        new = UpdateCodec(ratio, 8, "weights", backend=RotOracleBackend(), rotate=False, **kw).encode(_state(1))
        was = UpdateCodec(ratio, 8, "weights", backend=SROracleBackend(), **kw).encode(_state(1))
        assert new.to_bytes() == was.to_bytes() and struct.unpack_from("<I", new.to_bytes(), 8)[0] == (3 if kw else 2)


def _with_header(blob, change, version=6):
    h = change(dict(wire.sections(blob)[0]))
    hj = wire.encode_header(h)
    end = 16 + struct.unpack_from("<I", blob, 12)[0]
    body = blob[end + -end % 16:]
    head = blob[:8] + struct.pack("<II", version, len(hj)) + hj
    return head + b"\0" * (-len(head) % 16) + body


def _without(h, key):
    h = dict(h)
    del h[key]
    return h


def test_corrupt_blobs_are_rejected():
    blob = _codec(4, rotate_seed=1).encode(_state(1)).to_bytes()
    assert CompressedUpdate.from_bytes(_with_header(blob, lambda h: h)).to_bytes() == blob  # (the helper is sound)
    with pytest.raises(ValueError, match="version word"):  # a reader that knows version 5 only would see this word
        CompressedUpdate.from_bytes(_with_header(blob, lambda h: h, version=5))
    with pytest.raises(ValueError, match="version word"):  # ... and a version-6 word over a version-5 header
        CompressedUpdate.from_bytes(_with_header(blob, lambda h: _without(h, "rotate")))
    with pytest.raises(ValueError, match="blockwise"):
        CompressedUpdate.from_bytes(_with_header(blob, lambda h: _without(_without(h, "blockwise"), "n_blocks")))
    for size in (256, 1024):
        sizes = [e["n"] for e in wire.sections(blob)[0]["entries"] if e["kind"] == "seg"]
        with pytest.raises(ValueError, match="4096-element blocks"):
            CompressedUpdate.from_bytes(_with_header(
                blob, lambda h: dict(h, blockwise=size, n_blocks=wire.block_count(sizes, size))))
    for seed in (-1, 1 << 64, 1.5, "7", True, None, [1]):
        with pytest.raises(ValueError, match="rotation seed"):
            CompressedUpdate.from_bytes(_with_header(blob, lambda h: dict(h, rotate=seed)))
    for seed in (0, (1 << 64) - 1):
        assert CompressedUpdate.from_bytes(_with_header(blob, lambda h: dict(h, rotate=seed))).header["rotate"] == seed
    for extra in (dict(dense_packed=True), dict(compact=True), dict(n_units=3)):
        with pytest.raises(ValueError, match="excludes"):
            CompressedUpdate.from_bytes(_with_header(blob, lambda h: dict(h, **extra)))
    with pytest.raises(ValueError, match="dense"):
        CompressedUpdate.from_bytes(_with_header(blob, lambda h: _without(h, "dense")))
    for name in ("mn", "scale", "packed"):  # a blob cut inside a section is truncated
        o, n = wire.sections(blob)[1][name]
        with pytest.raises(ValueError, match="truncated"):
            CompressedUpdate.from_bytes(blob[:o + n - 4])
    # wire.pack applies the same rules to the header it is given
    h, mn, sc, _, _, raw, _ = wire.unpack(blob)
    o, n = wire.sections(blob)[1]["packed"]
    packed = np.frombuffer(blob, "<u4", n // 4, o)
    assert wire.pack(h, mn, sc, None, None, raw, packed=packed) == blob
    with pytest.raises(ValueError, match="blockwise"):
        wire.pack(_without(h, "blockwise"), mn, sc, None, None, raw, packed=packed)
    with pytest.raises(ValueError, match="rotation seed"):
        wire.pack(dict(h, rotate=-5), mn, sc, None, None, raw, packed=packed)


# -- the codec's refusals and seeds -----------------------------------------------------------------------
def test_rotate_value_errors():
    be = RotOracleBackend()
    with pytest.raises(ValueError, match="blockwise"):
        UpdateCodec(1.0, 4, "weights", backend=be, rotate=True)
    with pytest.raises(ValueError, match="ratio"):
        UpdateCodec(0.5, 4, "weights", backend=be, blockwise=True, rotate=True)
    with pytest.raises(ValueError, match="bits"):
        UpdateCodec(1.0, 32, "weights", backend=be, blockwise=True, rotate=True)
    for size in (256, 1024):
        with pytest.raises(ValueError, match="4096-element blocks"):
            UpdateCodec(1.0, 4, "weights", backend=be, blockwise=True, rotate=True, block_size=size)
    codec = _codec(4, "delta")
    snap = codec.snapshot(_state(2))
    with pytest.raises(ValueError, match="error feedback"):
        codec.encode(_state(1), base=snap, residual=codec.new_residual(_state(1)))
    for old in (BlockOracleBackend(), SROracleBackend()):  # a backend whose plan lacks the new methods
        with pytest.raises(ValueError, match="encode_block_rot"):
            _codec(4, backend=old).encode(_state(1))
    up = _codec(4).encode(_state(1))
    with pytest.raises(ValueError, match="decode_block_rot"):
        UpdateCodec(1.0, 4, "weights", backend=BlockOracleBackend()).decode_state(up)
    assert not UpdateCodec(backend=be).rotate
    assert CompressionClientMixin.codec_rotate is False and CompressionClientMixin.codec_rotate_seed is None
    assert CompressionServerMixin.codec_download_rotate is False
    assert CompressionServerMixin.codec_download_rotate_seed is None


def test_call_seeds():
    codec = _codec(4, rotate_seed=42, stochastic=True, seed=42)  # equal configured seeds
    a, b = codec.encode(_state(1)), codec.encode(_state(1))
    assert a.header["rotate"] != b.header["rotate"]
    assert [a.header["rotate"], b.header["rotate"]] == [sr_call_seed(42 ^ UpdateCodec.ROTATE_DOMAIN, n) for n in (0, 1)]
    for n, up in enumerate((a, b)):
        assert up.header["rotate"] != sr_call_seed(42, n)  # never the call's stochastic-rounding seed
    assert a.to_bytes() != b.to_bytes()
    again = _codec(4, rotate_seed=42, stochastic=True, seed=42).encode(_state(1))
    assert again.to_bytes() == a.to_bytes()  # the same configuration: the same bytes
    r1, r2 = _codec(4), _codec(4)  # None: drawn per codec
    assert r1.rotate_seed != r2.rotate_seed and 0 <= r1.rotate_seed < 1 << 64
    # a failed encode draws no seed: the two counters stay together
    codec = _codec(4, "delta", rotate_seed=1, stochastic=True, seed=1)
    snap = codec.snapshot(_state(2))
    with pytest.raises(ValueError):
        codec.encode(_state(1), base=snap, residual=codec.new_residual(_state(1)))
    assert codec._rot_calls == codec._sr_calls == 0


# -- aggregation and the mixins ---------------------------------------------------------------------------
def test_rotated_rounds_are_decoded_one_by_one():
    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "weights", RotOracleBackend()
        codec_fused_aggregate = codec_fused_dense_aggregate = True

    from coala_amd.fl.strategies import federated_averaging
    g = build_module("lenet", seed=5)
    server = Server(copy.deepcopy(g), [])
    ups = [pickle.loads(pickle.dumps(_codec(4, rotate_seed=s).encode(_lenet(s)))) for s in (1, 2, 3)]
    calls = RM.RotOraclePlan.calls
    with pytest.raises(ValueError):
        server._codec().aggregate(list(ups), [1, 3, 2], g, dense_kernel=True)
    with pytest.raises(ValueError):
        server._codec().aggregate(ups[:1], [1], g, dense_kernel=True)  # also a round of one
    got = server.aggregate(list(ups), [1, 3, 2])
    assert RM.RotOraclePlan.calls == calls  # no fused aggregate
    want = federated_averaging([server._decode_upload(u) for u in ups], [1, 3, 2])
    for a, b in zip(got.state_dict().values(), want.state_dict().values()):
        assert torch.equal(a, b)
    plain = pickle.loads(pickle.dumps(UpdateCodec(1.0, 4, "weights", backend=RotOracleBackend(),
                                                  blockwise=True).encode(_lenet(4))))
    mixed = [ups[0], plain]
    got = server.aggregate(list(mixed), [1, 1])
    want = federated_averaging([server._decode_upload(u) for u in mixed], [1, 1])
    for a, b in zip(got.state_dict().values(), want.state_dict().values()):
        assert torch.equal(a, b)


def test_mixin_round_upload_and_download():
    be, seen = RotOracleBackend(), {}

    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "delta", be
        codec_blockwise = codec_rotate = True
        codec_rotate_seed = 23

        def compression(self):
            super().compression()
            seen.setdefault("uploads", {})[self.cid] = self.model

    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "delta", be
        codec_download, codec_download_bits = True, 4
        codec_download_blockwise = codec_download_rotate = True
        codec_download_rotate_seed = 17

        def compression(self):
            super().compression()
            seen.setdefault("sent", []).append(self.model)
            seen.setdefault("global", []).append(copy.deepcopy(self._real_global().state_dict()))

    clients = [Client(f"c{i}", 5 + i, step_seed=i) for i in range(2)]
    server = Server(build_module("lenet", seed=7), clients, remote=True)
    server.round(0)
    # the download: a rotated carrier under the server's first call seed, decoded by every client to the model's values
    up = seen["sent"][0].update
    h = up.header
    rot_seed = sr_call_seed(17 ^ UpdateCodec.ROTATE_DOMAIN, 0)
    assert h["rotate"] == rot_seed and h["blockwise"] == UNIT and struct.unpack_from("<I", up.to_bytes(), 8)[0] == 6
    t, flat = _flat_of(h, seen["global"][0])
    mn, sc, _, stream = RM.encode(flat, t.segs, 4, rot_seed)
    want = RM.decode(stream, mn, sc, t.segs, 4, t.span, rot_seed)
    for c in clients:
        np.testing.assert_array_equal(c._codec_base.flat.numpy()[:t.span].view(np.uint32), want.view(np.uint32))
    # the uploads: rotated, each client under a seed of its own, decoded by the server to base + the model's delta
    ups = seen["uploads"]
    assert ups["c0"].header["rotate"] != ups["c1"].header["rotate"]
    for c in clients:
        u = ups[c.cid]
        seed = sr_call_seed(sr_call_seed(23, zlib.crc32(repr(c.cid).encode())) ^ UpdateCodec.ROTATE_DOMAIN, 0)
        assert u.header["rotate"] == seed and struct.unpack_from("<I", u.to_bytes(), 8)[0] == 6
        _, x = _flat_of(u.header, c.model.state_dict())
        base = c._codec_base.flat.numpy()[:t.span]
        mn, sc, _, stream = RM.encode(x, t.segs, 4, seed, base=base)
        ref = RM.decode(stream, mn, sc, t.segs, 4, t.span, seed, base=base)
        got = server.uploaded[c.cid].state_dict()  # (decoded on arrival, against the round's base)
        for e in u.header["entries"]:
            if e["kind"] == "seg":
                _bits_equal(got[e["name"]].numpy().reshape(-1), ref[e["off"]:e["off"] + e["n"]])


# -- what the knob buys -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def student():
    return np.random.default_rng(22).standard_t(3, 1 << 18).astype(np.float32)


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_rotation_has_strictly_smaller_error_on_heavy_tails(student, bits):
    rot, plain = RM.rms_error(student, bits, rot_seed=7), RM.rms_error(student, bits)
    print(f"student_t3 bits {bits}: rotated / unrotated RMS error {rot / plain:.3f}")
    assert rot < plain


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_mean_of_16_stochastic_uploads_has_strictly_smaller_error(student, bits):
    x = student[:1 << 16]
    rot = np.mean([RM.roundtrip(x, bits, rot_seed=100 + c, seed=200 + c).astype(np.float64) for c in range(16)], axis=0)
    plain = np.mean([RM.roundtrip(x, bits, seed=200 + c).astype(np.float64) for c in range(16)], axis=0)
    e_rot, e_plain = np.sqrt(np.mean((rot - x) ** 2)), np.sqrt(np.mean((plain - x) ** 2))
    print(f"student_t3 bits {bits}: mean of 16 SR uploads, rotated / unrotated RMS error {e_rot / e_plain:.3f}")
    assert e_rot < e_plain
