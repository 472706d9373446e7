"""Stochastic (unbiased) rounding for the dense quantisers, without a GPU: the contract's known-answer
values, the model's properties (tests/sr_model.py), the seed policy, and the host code — UpdateCodec(stochastic=True)
and the mixins' switches — over SROracleBackend, through all three dense wire formats."""
import pickle
import threading
from collections import OrderedDict

import numpy as np
import pytest
import torch

from coala_amd.compression import CompressedUpdate, CompressionClientMixin, CompressionServerMixin, UpdateCodec, wire
from coala_amd.compression.spec import SegmentTable, sr_call_seed
from coala_amd.compression.validate import validate
from oracle import codec_oracle as O
from tests import blockwise_model as BM
from tests import sr_model as M
from tests.blockwise_model import BlockOracleBackend
from tests.oracle_backend import OracleBackend
from tests.sr_model import SROracleBackend

SIZES = [1, 3, 5, 1023, 4096, 4097, 2 * 4096 + 517]  # the layout tests/test_gpu_sr.py uses


def test_known_answer_draws():
    assert [int(x) for x in M.sr_u24(0, [0, 1, 2, 3])] == [0x944fb5, 0xb2fcf0, 0xfdd0ca, 0x1ece84]
    got = M.sr_u24(0xDEADBEEFCAFEF00D, [0, 1, 1 << 32, (1 << 32) + 1])
    assert [int(x) for x in got] == [0xb741a7, 0x05c4ca, 0x0f049b, 0xac3d96]


def test_call_seed_is_splitmix64():
    # splitmix64's published first outputs for the state 0 (Vigna's splitmix64.c; the same stream seeds Java's
    # SplittableRandom(0)): 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4 — its n-th output is the mix of (n + 1) * gamma
    assert sr_call_seed(0, 0) == 0xE220A8397B1DCDAF
    assert sr_call_seed(0, 1) == 0x6E789E6AA1B965F4
    # and, by hand for one more state: seed + 1 * gamma with seed = 2^64 - gamma wraps to 0, whose mix is 0
    assert sr_call_seed((1 << 64) - 0x9E3779B97F4A7C15, 0) == 0
    assert len({sr_call_seed(7, n) for n in range(1000)}) == 1000
    assert all(0 <= sr_call_seed(s, 3) < 1 << 64 for s in (0, 1, (1 << 64) - 1, -5))


@pytest.mark.parametrize("bits", [1, 2, 4, 8])
def test_codes_are_floor_or_floor_plus_one(bits):
    rng = np.random.default_rng(bits)
    x = rng.standard_normal(5000).astype(np.float32)
    _, mn, sc = O.quantize(x, bits)
    L = (1 << bits) - 1
    codes = M.sr_codes(x, mn, sc, bits, 11, 64).astype(np.int64)
    t = M.quotient(x, mn, sc).astype(np.float64)
    fl = np.minimum(np.floor(t), L).astype(np.int64)
    assert ((codes == fl) | (codes == np.minimum(fl + 1, L))).all()
    assert codes.min() == 0 and codes.max() == L  # the range's own ends: t = 0 and t >= L
    whole = t == np.floor(t)
    assert whole.any() and (codes[whole] == fl[whole]).all()
    assert (codes != np.clip(np.rint(t), 0, L)).any()  # not round-to-nearest


def test_integer_quotients_are_kept_for_every_draw():
    t = np.repeat(np.arange(16, dtype=np.float32), 3)
    u = np.tile(np.array([0, 0x800000, 0xFFFFFF], np.uint32), 16)
    assert (M.codes_of(t, u, 15) == t).all()
    # next to an integer the draw decides: u = 0 rounds any fraction up, the largest u only a fraction of 1 - 2^-24 or more
    assert M.codes_of(np.float32([3.0000002]), np.uint32([0]), 15)[0] == 4
    assert M.codes_of(np.float32([3.9999998]), np.uint32([0xFFFFFF]), 15)[0] == 3
    assert list(M.codes_of(np.float32([20.0, np.inf, -1.0, np.nan, -0.0]), np.uint32([5] * 5), 15)) == [15, 15, 0, 0, 0]


def test_nan_constant_and_zero_scale_give_code_zero():
    x = np.full(100, 7.5, np.float32)
    assert (M.sr_codes(x, np.float32(7.5), np.float32(0.0), 4, 3, 0) == 0).all()
    assert (M.sr_codes(x, np.float32(np.nan), np.float32(np.nan), 4, 3, 0) == 0).all()
    segs = SegmentTable([100, 50, 30], 1.0).segs.astype(np.int64)
    flat = np.zeros(int(segs[-1, 0] + segs[-1, 1]), np.float32)
    flat[:100] = 7.5                                  # constant: scale 0
    flat[segs[1, 0]:segs[1, 0] + 50] = np.nan         # all NaN: a NaN range
    y = np.linspace(-1, 1, 30).astype(np.float32)
    y[::4] = np.nan
    y[1] = np.inf
    flat[segs[2, 0]:segs[2, 0] + 30] = y              # NaN elements, an infinite range
    for enc in (M.encode(flat, segs, 4, 9), M.encode_block(flat, segs, 4, 9)[2:3] + M.encode_block(flat, segs, 4, 9)[:2]):
        codes, mn, sc = enc
        assert (codes == 0).all()
        assert mn[0] == 7.5 and sc[0] == 0 and np.isnan(mn[1]) and np.isinf(sc[2])


def test_seeds_change_the_codes_and_nothing_else():
    rng = np.random.default_rng(2)
    segs = SegmentTable(SIZES, 1.0).segs.astype(np.int64)
    flat = rng.standard_normal(int(segs[-1, 0] + segs[-1, 1])).astype(np.float32)
    for bits in (2, 8):
        a, b, c = (M.encode(flat, segs, bits, s) for s in (1, 1, 2))
        det = O.encode(flat, segs, bits)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
        assert (a[0] != c[0]).mean() > 0.2
        for r in (1, 2):  # the ranges are the deterministic encode's
            np.testing.assert_array_equal(a[r].view(np.uint32), det[r + 1].view(np.uint32))
            np.testing.assert_array_equal(c[r].view(np.uint32), det[r + 1].view(np.uint32))
        ba, bb = M.encode_block(flat, segs, bits, 1), M.encode_block(flat, segs, bits, 2)
        bd = BM.encode(flat, segs, bits)
        assert (ba[3] != bb[3]).any()
        np.testing.assert_array_equal(ba[0].view(np.uint32), bd[0].view(np.uint32))
        np.testing.assert_array_equal(ba[1].view(np.uint32), bd[1].view(np.uint32))
    # the position is the flat one: the same values at another in_off round differently
    v = flat[:1023]
    assert (M.sr_codes(v, -4, 0.5, 4, 1, 0) != M.sr_codes(v, -4, 0.5, 4, 1, 4096)).any()


def _state(seed=0):
    rng = np.random.default_rng(seed)
    st = OrderedDict()
    for i, n in enumerate(SIZES):
        st[f"w{i}"] = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    st["steps"] = torch.tensor(7, dtype=torch.int64)
    return st


FORMATS = [({}, 1), ({"pack_dense": True}, 4), ({"blockwise": True}, 5)]  # (plain dense: the first format + "dense")


@pytest.mark.parametrize("opts,version", FORMATS, ids=["dense", "v4", "v5"])
def test_stochastic_blobs_are_ordinary_blobs(opts, version):
    bits, seed = 4, 0x1234ABCD5678
    codec = UpdateCodec(1.0, bits, "weights", backend=SROracleBackend(), stochastic=True, seed=seed, **opts)
    plain = UpdateCodec(1.0, bits, "weights", backend=SROracleBackend(), **opts)
    st = _state()
    up, det = codec.encode(st), plain.encode(st)
    assert wire.format_of(up.header).version == version and wire.is_dense(up.header)
    assert set(up.header) == set(det.header) and up.nbytes == det.nbytes  # no key, no byte: not on the wire
    blob = up.to_bytes()
    assert len(blob) == len(det.to_bytes()) and blob != det.to_bytes()
    back = CompressedUpdate.from_bytes(blob)
    assert back.to_bytes() == blob and pickle.loads(pickle.dumps(up)).to_bytes() == blob
    validate(back.header, back.encoded.idx.numpy(), None)
    # the payload is the model's, at the codec's first call seed
    segs = SegmentTable(SIZES, 1.0).segs.astype(np.int64)
    flat = np.zeros(int(segs[-1, 0] + segs[-1, 1]), np.float32)
    for (off, n, _, _), t in zip(segs.tolist(), list(st.values())):
        flat[off:off + n] = t.numpy()
    s0 = sr_call_seed(seed, 0)
    if version == 5:
        mn, sc, _, stream = M.encode_block(flat, segs, bits, s0)
        np.testing.assert_array_equal(up.packed.numpy(), stream)
    else:
        codes, mn, sc = M.encode(flat, segs, bits, s0)
        np.testing.assert_array_equal(up.encoded.vals.numpy(), codes)
    np.testing.assert_array_equal(up.encoded.mn.numpy().view(np.uint32), mn.view(np.uint32))
    # decoding needs no switch, and every decoded value is within one step of its input
    dec = UpdateCodec(1.0, bits, "weights", backend=BlockOracleBackend())
    got, own = dec.decode_state(back), codec.decode_state(up)
    step = float(up.encoded.scale.max())
    for k, v in st.items():
        assert torch.equal(got[k], own[k])
        if v.dtype == torch.float32:
            assert float((got[k] - v).abs().max()) <= step * 1.0001
    # the next encode of the same state uses the next call seed
    assert codec.encode(st).to_bytes() != blob
    again = UpdateCodec(1.0, bits, "weights", backend=SROracleBackend(), stochastic=True, seed=seed, **opts)
    assert again.encode(st).to_bytes() == blob


def test_value_errors():
    for kw in ({"ratio": 0.5}, {"bits": 32}):
        with pytest.raises(ValueError, match="stochastic"):
            UpdateCodec(**{"ratio": 1.0, "bits": 4, "mode": "weights", "stochastic": True, **kw})
    st = _state()
    for backend, opts in ((OracleBackend(), {}), (BlockOracleBackend(), {}), (BlockOracleBackend(), {"blockwise": True})):
        with pytest.raises(ValueError, match="stochastic rounding is not available"):
            UpdateCodec(1.0, 4, "weights", backend=backend, stochastic=True, **opts).encode(st)
    codec = UpdateCodec(1.0, 4, "delta", backend=SROracleBackend(), stochastic=True)
    base = codec.snapshot(_state(1), device=torch.device("cpu"))
    with pytest.raises(ValueError, match="error feedback"):
        codec.encode(st, base=base, residual=torch.zeros(8))
    assert codec.encode(st, base=base).header["mode"] == "delta"  # delta mode itself is fine

    class Client(CompressionClientMixin):
        codec_ratio, codec_bits, codec_backend = 1.0, 4, SROracleBackend()
        codec_stochastic = codec_error_feedback = True

    with pytest.raises(ValueError, match="codec_stochastic"):
        Client()._codec()


def test_defaults_are_off_and_change_nothing():
    assert UpdateCodec().stochastic is False
    assert CompressionClientMixin.codec_stochastic is False and CompressionClientMixin.codec_stochastic_seed is None
    assert CompressionServerMixin.codec_download_stochastic is False
    assert CompressionServerMixin.codec_download_stochastic_seed is None
    st = _state()
    for opts, _ in FORMATS:
        new = UpdateCodec(1.0, 4, "weights", backend=SROracleBackend(), **opts).encode(st)
        old = UpdateCodec(1.0, 4, "weights", backend=BlockOracleBackend(), **opts).encode(st)  # the parent's route
        assert new.to_bytes() == old.to_bytes()


def test_seed_policy():
    a, b = UpdateCodec(1.0, 4, stochastic=True), UpdateCodec(1.0, 4, stochastic=True)
    assert a.seed != b.seed and 0 <= a.seed < 1 << 64  # os.urandom, once per codec
    codec = UpdateCodec(1.0, 4, stochastic=True, seed=99)
    got, lock = [], threading.Lock()

    def work():
        mine = [codec._next_sr_seed() for _ in range(300)]
        with lock:
            got.extend(mine)
    threads = [threading.Thread(target=work) for _ in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert sorted(got) == sorted(sr_call_seed(99, n) for n in range(2400))

    def client(cid, seed=5):
        class Client(CompressionClientMixin):
            codec_ratio, codec_bits, codec_mode, codec_backend = 1.0, 4, "weights", SROracleBackend()
            codec_stochastic, codec_stochastic_seed = True, seed
        c = Client()
        if cid is not None:
            c.cid = cid
        return c._codec()
    assert client("a").seed == client("a").seed != client("b").seed
    assert client(None).seed == 5 and client("a").seed not in (5, client("a", seed=6).seed)
    assert client(None).stochastic and client("a", seed=None).seed != client("a", seed=None).seed

    class Server(CompressionServerMixin):
        codec_download, codec_download_bits, codec_backend = True, 2, SROracleBackend()
        codec_download_stochastic, codec_download_stochastic_seed = True, 17
    d = Server()._download_codec()
    assert d.stochastic and d.seed == 17 and not Server()._codec().stochastic


def test_average_of_64_uploads_loses_the_rounding_bias():
    """64 block-wise 2-bit uploads of one N(0,1) tensor set, distinct seeds: the RMS error of their decoded mean is
    below 0.25 x that of the round-to-nearest encode's decode (the prediction for uniform fractions is
    1 / (8 sqrt(0.5)) = 0.177; identical deterministic uploads give 1.0), and its mean signed error vanishes."""
    bits, C = 2, 64
    segs = SegmentTable(SIZES, 1.0).segs.astype(np.int64)
    span = int(segs[-1, 0] + segs[-1, 1])
    inside = np.zeros(span, bool)
    for off, n, _, _ in segs.tolist():
        inside[off:off + n] = True
    flat = np.where(inside, np.random.default_rng(64).standard_normal(span), 0).astype(np.float32)
    mn, sc, codes, _ = BM.encode(flat, segs, bits)
    det = BM.decode_codes(codes, mn, sc, segs, bits, span)[inside].astype(np.float64)
    acc = np.zeros(int(inside.sum()))
    for i in range(C):
        m, s, c, _ = M.encode_block(flat, segs, bits, sr_call_seed(2024, i))
        acc += BM.decode_codes(c, m, s, segs, bits, span)[inside]
    x = flat[inside].astype(np.float64)
    err = acc / C - x
    rms, rms_det = np.sqrt((err ** 2).mean()), np.sqrt(((det - x) ** 2).mean())
    print(f"rms(mean of {C} stochastic) / rms(round to nearest) = {rms / rms_det:.4f}; mean signed error {err.mean():.2e}")
    assert rms < 0.25 * rms_det
    assert abs(err.mean()) < 5e-3 * rms_det
