"""Error feedback for the top-k upload, without a GPU: the CPU model (tests/ef_model.py) against a literal loop and
the telescoping identity, then the codec and the hook mixins running it through an oracle-backed plan, and the
argument checks of the two new C entry points. Every comparison is bit-exact.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from coala_amd.compression import CompressionClientMixin, CompressionServerMixin, UpdateCodec, _lib, flatten_state
from coala_amd.compression.spec import SegmentTable
from coala_amd.fl import LoopbackClient, LoopbackServer, unmarshal
from coala_amd.layouts import build_module
from oracle import codec_oracle as O
from tests import ef_model as M
from tests.ef_model import EFOracleBackend, bits_of
from tests.oracle_backend import OracleBackend

F32 = np.float32


def eq(a, b, msg=""):
    np.testing.assert_array_equal(bits_of(a), bits_of(b), err_msg=msg)


# -- the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [3, 8, 32])
@pytest.mark.parametrize("with_base", [False, True])
def test_model_equals_literal_loop(bits, with_base):
    table = SegmentTable([1, 5, 7, 10], 0.3, 1)  # in_off multiples of 4: gaps after the 1-, 5-, 7- and 10-element segments
    segs = table.segs.astype(np.int64)
    rng = np.random.default_rng(bits)
    x = rng.standard_normal(table.span).astype(F32)
    base = rng.standard_normal(table.span).astype(F32) if with_base else None
    r0 = rng.standard_normal(table.span).astype(F32)
    a = M.accumulate(x, r0, segs, base)
    inside = np.zeros(table.span, bool)
    for off, n, k, oo in segs:
        for i in range(off, off + n):
            inside[i] = True
            d = F32(x[i] - base[i]) if with_base else x[i]
            assert bits_of(a[i:i + 1])[0] == bits_of(np.array([F32(d + r0[i])]))[0]
    assert not inside.all()
    eq(a[~inside], r0[~inside])  # the padding is not written
    (idx, vals, mn, sc), r1 = M.ef_round(x, r0, segs, bits, base)
    want = a.copy()
    for s, (off, n, k, oo) in enumerate(segs):
        for e in range(oo, oo + k):
            xhat = F32(vals[e]) if bits == 32 else F32(F32(mn[s]) + F32(F32(vals[e]) * F32(sc[s])))
            want[off + idx[e]] = F32(a[off + idx[e]] - xhat)
    eq(r1, want)
    eq(M.commit(a, idx, vals, mn, sc, segs, bits), r1)


def test_model_commit_stores_plus_zero_for_non_finite():
    segs = np.array([[0, 8, 4, 0]])
    a = np.array([np.nan, np.inf, -np.inf, 5.0, 1.0, -0.0, 0.0, 0.5], dtype=F32)
    idx, vals, mn, sc = O.encode(a, segs, 32)
    assert idx.tolist() == [0, 1, 2, 3]
    r = M.commit(a, idx, vals, mn, sc, segs, 32)
    eq(r, np.array([0.0, 0.0, 0.0, 0.0, 1.0, -0.0, 0.0, 0.5], dtype=F32))


def test_telescoping_identity_raw_values():
    """bits 32, integer-valued updates (every fp32 operation exact): after T rounds everything that was ever sent in
    is delivered or still in the residual — sum_t decoded_t + r_T == sum_t delta_t."""
    table = SegmentTable([1, 5, 300, 4097], 0.05, 1)
    segs = table.segs.astype(np.int64)
    rng = np.random.default_rng(7)
    r = np.zeros(table.span, F32)
    delivered = np.zeros(table.span, F32)
    total = np.zeros(table.span, F32)
    inside = np.zeros(table.span, bool)
    for off, n, _, _ in segs:
        inside[off:off + n] = True
    for t in range(4):
        base = rng.integers(-(1 << 18), 1 << 18, table.span).astype(F32)
        delta = rng.integers(-(1 << 19), 1 << 19, table.span).astype(F32)
        delta[rng.random(table.span) < 0.3] = 0.0
        x = base + delta
        (idx, vals, mn, sc), r = M.ef_round(x, r, segs, 32, base)
        delivered += O.decode(idx, vals, mn, sc, segs, 32, table.span)
        total += np.where(inside, delta, F32(0))
    assert np.abs(total).max() < (1 << 22)
    np.testing.assert_array_equal(delivered + r, total)
    assert np.count_nonzero(r)  # (something was in fact delayed)


# -- the codec ------------------------------------------------------------------------------------
def _perturb(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 1e-2)


def test_codec_three_rounds_equal_model():
    codec = UpdateCodec(0.02, 8, "delta", backend=EFOracleBackend())
    g = build_module("lenet", seed=2)
    m = copy.deepcopy(g)
    snap = codec.snapshot(g)
    res = codec.new_residual(m)
    assert res.dtype == torch.float32 and res.device.type == "cpu" and not res.any()
    plain = UpdateCodec(0.02, 8, "delta", backend=OracleBackend())
    r = res.numpy().copy()
    for t in range(3):
        _perturb(m, 10 + t)
        up = codec.encode_module(m, base=snap, residual=res)
        x = flatten_state(m.state_dict()).flat.numpy()
        table = SegmentTable(_sizes(m), 0.02, 1)
        segs = table.segs
        assert res.numel() == table.span
        (idx, vals, mn, sc), r = M.ef_round(x, r, segs, 8, snap.flat.numpy())
        np.testing.assert_array_equal(up.encoded.idx.numpy(), idx)
        np.testing.assert_array_equal(up.encoded.vals.numpy(), vals)
        eq(up.encoded.mn, mn)
        eq(up.encoded.scale, sc)
        eq(res, r, f"round {t}")
        assert up.header["mode"] == "delta"
        # an ordinary delta-mode payload: the plain codec's header, field by field
        ref = plain.encode_module(m, base=snap)
        assert up.header.keys() == ref.header.keys()
        assert all(up.header[k] == ref.header[k] for k in ("ratio", "bits", "mode", "n_segments", "total_k", "entries"))
        assert plain.decode_state(up, base=snap).keys() == m.state_dict().keys()
    assert np.count_nonzero(r)
    # encode(state_dict) takes the residual too
    res2 = codec.new_residual(m.state_dict())
    up2 = codec.encode(m.state_dict(), base=snap, residual=res2)
    (idx, *_), r2 = M.ef_round(flatten_state(m.state_dict()).flat.numpy(), np.zeros_like(r), segs, 8, snap.flat.numpy())
    np.testing.assert_array_equal(up2.encoded.idx.numpy(), idx)
    eq(res2, r2)


def _sizes(m):
    return [int(v.numel()) for v in m.state_dict().values() if v.dtype == torch.float32]


def test_codec_rejects_weights_mode_wrong_span_and_plain_backend():
    m = build_module("lenet", seed=2)
    snap = UpdateCodec(0.02, 8, "delta", backend=EFOracleBackend()).snapshot(m)
    with pytest.raises(ValueError, match="delta"):
        UpdateCodec(0.02, 8, "weights", backend=EFOracleBackend()).encode_module(m, residual=torch.zeros(8))
    codec = UpdateCodec(0.02, 8, "delta", backend=EFOracleBackend())
    good = codec.new_residual(m)
    with pytest.raises(ValueError, match="residual"):
        codec.encode_module(m, base=snap, residual=torch.zeros(good.numel() + 4))
    with pytest.raises(ValueError, match="residual"):
        codec.encode_module(m, base=snap, residual=good.double())
    with pytest.raises(RuntimeError, match="ef_accumulate"):
        UpdateCodec(0.02, 8, "delta", backend=OracleBackend()).encode_module(m, base=snap, residual=good)


# -- the hooks ------------------------------------------------------------------------------------
def _classes(feedback, mode="delta", backend=EFOracleBackend):
    class Client(CompressionClientMixin, LoopbackClient):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.02, 8, mode, backend()
        codec_error_feedback = feedback

        def compression(self):  # what the codec is about to see, for the independent restatement below
            self.seen = (flatten_state(self.model.state_dict()).flat.numpy().copy(),
                         None if mode != "delta" else self._codec_base.flat.numpy().copy(),
                         self.model)
            super().compression()

    class Server(CompressionServerMixin, LoopbackServer):
        codec_ratio, codec_bits, codec_mode, codec_backend = 0.02, 8, mode, OracleBackend()

    return Client, Server


def test_hooks_two_clients_three_rounds():
    Client, Server = _classes(True)
    g0 = build_module("lenet", seed=5)
    clients = [Client(f"c{i}", 20 + i, step_seed=i) for i in range(2)]
    server = Server(copy.deepcopy(g0), clients)
    segs = SegmentTable(_sizes(g0), 0.02, 1).segs
    rs = [np.zeros(SegmentTable(_sizes(g0), 0.02, 1).span, F32) for _ in clients]
    for t in range(3):
        server.uploaded, server.weights = {}, {}
        for i, c in enumerate(clients):
            req = c.run_train(server.model, t)
            x, base, _ = c.seen
            (idx, vals, mn, sc), rs[i] = M.ef_round(x, rs[i], segs, 8, base)
            up = unmarshal(req.content.data)
            assert up.header["mode"] == "delta"
            np.testing.assert_array_equal(up.encoded.idx.numpy(), idx)
            np.testing.assert_array_equal(up.encoded.vals.numpy(), vals)
            eq(c._codec_residual[1], rs[i], f"client {i} round {t}")
            # an unmodified server decodes it: w_global + decode(payload)
            dec = server.decompression(up)
            want = O.decode(idx, vals, mn, sc, segs, 8, len(base), base=base)
            eq(flatten_state(dec.state_dict()).flat, want)
            server.uploaded[c.cid], server.weights[c.cid] = dec, req.content.data_size
        server.aggregation()
    a, b = (c._codec_residual[1] for c in clients)
    assert a.data_ptr() != b.data_ptr() and not torch.equal(a, b) and a.any() and b.any()
    clients[0].reset_error_feedback()
    assert not clients[0]._codec_residual[1].any() and clients[1]._codec_residual[1].any()
    assert clients[0]._codec_residual[1].data_ptr() == a.data_ptr()


def test_hooks_residual_follows_the_model_layout():
    Client, _ = _classes(True)
    c = Client("c0", 3)
    c.run_train(build_module("lenet", seed=1), 0)
    first = c._codec_residual[1]
    assert first.any()
    c.model = None  # a new task with another model
    c.__dict__.pop("_codec_base", None)
    c.run_train(build_module("simple_cnn_split_cut1", seed=1), 0)
    second = c._codec_residual[1]
    assert second is not first and second.numel() != first.numel()


def test_hooks_flag_off_is_todays_upload():
    Off, _ = _classes(False)
    c = Off("c0", 7, step_seed=3)
    g0 = build_module("lenet", seed=5)
    req = c.run_train(copy.deepcopy(g0), 0)
    assert "_codec_residual" not in c.__dict__
    codec = UpdateCodec(0.02, 8, "delta", backend=OracleBackend())
    want = codec.encode_module(c.seen[2], base=codec.snapshot(g0))
    assert unmarshal(req.content.data).to_bytes() == want.to_bytes()
    reset = c.reset_error_feedback()  # nothing to reset: no error
    assert reset is None


def test_hooks_weights_mode_with_flag_raises():
    Client, _ = _classes(True, mode="weights")
    c = Client("c0", 7)
    with pytest.raises(ValueError, match="codec_error_feedback.*delta"):
        c.run_train(build_module("lenet", seed=5), 0)


# -- the C ABI ------------------------------------------------------------------------------------
def test_new_entry_points_check_their_arguments():
    lib = _lib.load()
    err = lambda: lib.coalac_last_error().decode()
    assert lib.coalac_ef_accumulate(None, None, None, None, None, None) == -1 and "plan is NULL" in err()
    assert lib.coalac_ef_commit(None, None, None, None, None, None, None, None) == -1 and "plan is NULL" in err()
    # both or neither input: rejected before the plan is used (any non-NULL handle shows it)
    handle = ctypes.create_string_buffer(4096)
    buf = ctypes.create_string_buffer(64)
    plan, p = ctypes.addressof(handle), ctypes.addressof(buf) // 16 * 16 + 16
    assert lib.coalac_ef_accumulate(plan, None, None, None, p, None) == -1 and "exactly one" in err()
    assert lib.coalac_ef_accumulate(plan, p, p, None, p, None) == -1 and "exactly one" in err()
    assert _lib.ERRORS[-1] == "COALAC_EINVAL"


def test_loader_reports_an_old_library_by_its_version(monkeypatch):
    """A library of another ABI lacks symbols this binding names: the version is compared first, so the failure is
    the ABI message, not an AttributeError."""
    class Old:
        class _Fn:
            restype = argtypes = None

            def __call__(self):
                return _lib.ABI_VERSION - 1

        def __init__(self, path):
            self.coalac_version = self._Fn()

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", Old)
    monkeypatch.setenv("COALAC_LIB", "/nonexistent/libcoalac_old.so")
    with pytest.raises(_lib.CodecError, match="ABI version"):
        _lib.load()
