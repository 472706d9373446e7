"""The compact payload's kernels (k_pack / k_unpack) against the host model of the format,
wire.pack_entries / wire.unpack_entries. Every comparison is bit-exact. Small plans: the kernels have one path per
field width, a full-lane and a tail-lane load in k_pack, and the clamped unit ranges in k_unpack."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, Encoded, UpdateCodec, _lib, wire
from coala_amd.compression.spec import UNIT
from coala_amd.layouts import build_module

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 4095, 4096, 4097, 8193, 70001]
CANARY = -7


def _input(plan, seed, empty_unit=False):
    """A flat input of the plan's layout; empty_unit: the middle 4096-element unit of the 70001-element segments is
    all zeros and the rest of those segments large, so that unit keeps nothing."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(plan.span).astype(np.float32)
    if empty_unit:
        for off, n, _, _ in plan.table.segs.astype(np.int64):
            if n == 70001:
                x[off:off + n] = (10.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n)
                x[off + 8 * UNIT:off + 9 * UNIT] = 0.0
    return torch.from_numpy(x).cuda()


def _check_round_trip(plan, enc):
    """pack == the host model's bytes; unpack gives idx / vals back; decode of the unpacked == decode of the original."""
    packed = plan.pack(enc)
    assert packed.dtype == torch.uint32 and packed.numel() == plan.packed_words == wire.packed_words(plan.total_k, plan.bits)
    want = wire.pack_entries(enc.idx.cpu().numpy(), enc.vals.cpu().numpy().view(np.uint8)[:plan.total_k], plan.bits)
    np.testing.assert_array_equal(packed.cpu().numpy(), want)
    idx, vals = plan.unpack(packed, enc.ustart)
    assert torch.equal(idx, enc.idx)
    if plan.bits == 32:  # (not written: the fp32 values travel in their own section)
        vals = enc.vals
    else:
        assert vals.dtype == torch.uint8 and torch.equal(vals, enc.vals)
    zeros = lambda: torch.zeros(plan.span, dtype=torch.float32, device="cuda")  # (decode leaves the padding alone)
    a = plan.decode(enc, out=zeros())
    b = plan.decode(Encoded(idx, vals, enc.mn, enc.scale, enc.ustart), out=zeros())
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    return packed


@pytest.mark.parametrize("bits", [1, 5, 8, 32])
@pytest.mark.parametrize("ratio", [0.01, 0.9])
def test_small_plan(cuda, ratio, bits):
    plan = CodecPlan(SIZES, ratio, bits)
    for empty_unit in (False, True):
        enc = plan.encode(_input(plan, 3, empty_unit))
        if empty_unit:
            ust = enc.ustart.cpu().numpy()
            first = int(sum((n + UNIT - 1) // UNIT for n in SIZES[:-1]))
            assert ust[first + 8] == ust[first + 9]  # the unit owns no entry
        _check_round_trip(plan, enc)


@pytest.mark.parametrize("sizes", [[6400], [6400, 100]])  # total_k 64 (whole lanes only) and 65 (a tail lane)
@pytest.mark.parametrize("bits", [4, 7])
def test_total_k_multiple_of_32_and_not(cuda, sizes, bits):
    plan = CodecPlan(sizes, 0.01, bits)
    assert plan.total_k == 64 + (len(sizes) - 1) and (plan.total_k % 32 == 0) == (len(sizes) == 1)
    packed = _check_round_trip(plan, plan.encode(_input(plan, 4)))
    stream = np.unpackbits(packed.cpu().numpy().view(np.uint8), bitorder="little")
    assert not stream[plan.total_k * (12 + bits):].any()  # the tail word is zero-padded


def test_batched_plan(cuda):
    plan = CodecPlan(SIZES, 0.05, 6, clients=3)
    _check_round_trip(plan, plan.encode(_input(plan, 5, True)))


def test_explicit_row_plan_leaves_other_positions(cuda):
    whole = CodecPlan(SIZES, 0.1, 8)
    enc = whole.encode(_input(whole, 6))
    segs = whole.table.segs
    part = CodecPlan.from_segments(segs[3:6], 8)  # absolute in_off / out_off: a slice inside the whole buffers
    lo, hi = int(segs[3, 3]), int(segs[5, 3] + segs[5, 2])
    assert part.total_k == hi and lo > 0 and hi < whole.total_k
    assert part.n_units == 1 + 2 + 3 and whole.n_units == 1 + 1 + 1 + 1 + 2 + 3 + 18
    ustart = enc.ustart[3:9].contiguous()  # the units of segments 3..5
    packed = part.pack(Encoded(enc.idx, enc.vals, enc.mn[3:6].contiguous(), enc.scale[3:6].contiguous(), ustart))
    np.testing.assert_array_equal(
        packed.cpu().numpy(), wire.pack_entries(enc.idx[:hi].cpu().numpy(), enc.vals[:hi].cpu().numpy(), 8))
    idx = torch.full((whole.total_k,), CANARY, dtype=torch.int32, device="cuda")
    vals = torch.full((whole.total_k,), 0xA5, dtype=torch.uint8, device="cuda")
    part.unpack(packed, ustart, out=(idx, vals))
    assert torch.equal(idx[lo:hi], enc.idx[lo:hi]) and torch.equal(vals[lo:hi], enc.vals[lo:hi])
    assert (idx[:lo] == CANARY).all() and (idx[hi:] == CANARY).all()
    assert (vals[:lo] == 0xA5).all() and (vals[hi:] == 0xA5).all()


@pytest.mark.parametrize("starts", ["plus_one", "random", "random_small"])
@pytest.mark.parametrize("clients", [1, 3])
def test_unpack_clamps_wrong_starts(cuda, starts, clients):
    """Wrong per-unit starts (the blob may be untrusted) can mis-unpack but never write outside the segments' own
    positions: canaries before and after the plan's entries survive, and every index stays inside its segment's units."""
    plan = CodecPlan(SIZES, 0.3, 8, clients=clients)
    enc = plan.encode(_input(plan, 7))
    packed = plan.pack(enc)
    rng = np.random.default_rng(13)
    if starts == "plus_one":
        ust = enc.ustart + 1
    elif starts == "random":  # any int32: most ranges clamp to nothing
        ust = torch.from_numpy(rng.integers(-(2 ** 31), 2 ** 31 - 1, plan.n_units, dtype=np.int64).astype(np.int32)).cuda()
    else:  # ... and starts of the right magnitude: overlapping, reversed and oversized ranges
        ust = torch.from_numpy(rng.integers(0, 2 * int(plan.table.segs[:, 2].max()), plan.n_units).astype(np.int32)).cuda()
    K, pad = plan.total_k, 256
    ibuf = torch.full((K + 2 * pad,), CANARY, dtype=torch.int32, device="cuda")
    vbuf = torch.full((K + 2 * pad,), 0xA5, dtype=torch.uint8, device="cuda")
    plan.unpack(packed, ust, out=(ibuf[pad:pad + K + pad], vbuf[pad:pad + K + pad]))
    torch.cuda.synchronize()
    i, v = ibuf.cpu().numpy(), vbuf.cpu().numpy()
    assert (i[:pad] == CANARY).all() and (i[pad + K:] == CANARY).all()
    assert (v[:pad] == 0xA5).all() and (v[pad + K:] == 0xA5).all()
    segs = plan.table.segs.astype(np.int64)
    limit = np.concatenate([np.full(k, (n + UNIT - 1) // UNIT * UNIT) for _, n, k, _ in segs])
    body = i[pad:pad + K]
    written = body != CANARY
    assert written.any() or starts == "random"
    assert (body[written] >= 0).all() and (body[written] < limit[written]).all()
    # ... and the host model clamps the same way: the same positions written, with the same values
    hi_, hv = wire.unpack_entries(packed.cpu().numpy(), ust.cpu().numpy(), segs[:, 1], segs[:, 2], 8)
    if starts == "plus_one":  # (ranges of different units do not overlap: one writer per position)
        np.testing.assert_array_equal(body[written], hi_[written])


def test_abi_errors(cuda):
    lib = _lib.load()
    plan = CodecPlan([5000, 300], 0.1, 8)
    dense = CodecPlan([64, 8], 1.0, 8)
    enc = plan.encode(_input(plan, 8))
    packed = plan.pack(enc)
    nbytes = ctypes.c_uint64(4 * plan.packed_words)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N = ctypes.c_void_p(0)
    b = ctypes.c_uint64()
    assert lib.coalac_plan_packed_bytes(plan._h, ctypes.byref(b)) == 0 and b.value == nbytes.value
    assert lib.coalac_plan_packed_bytes(None, ctypes.byref(b)) == -1 and lib.coalac_plan_packed_bytes(plan._h, None) == -1
    good_pack = (plan._h, p(enc.idx), p(enc.vals), p(packed), nbytes, N)
    good_unpack = (plan._h, p(packed), nbytes, p(enc.ustart), p(enc.idx), p(enc.vals), N)
    for i in (0, 1, 2, 3):  # every pointer NULL in turn
        assert lib.coalac_pack(*[N if j == i else a for j, a in enumerate(good_pack)]) == -1
    for i in (0, 1, 3, 4, 5):
        assert lib.coalac_unpack(*[N if j == i else a for j, a in enumerate(good_unpack)]) == -1
    short = ctypes.c_uint64(nbytes.value - 4)
    assert lib.coalac_pack(plan._h, p(enc.idx), p(enc.vals), p(packed), short, N) == -1
    assert b"packed_bytes" in lib.coalac_last_error()
    assert lib.coalac_unpack(plan._h, p(packed), short, p(enc.ustart), p(enc.idx), p(enc.vals), N) == -1
    assert lib.coalac_pack(dense._h, p(enc.idx), p(enc.vals), p(packed), nbytes, N) == -1
    assert b"dense" in lib.coalac_last_error()
    assert lib.coalac_unpack(dense._h, p(packed), nbytes, p(enc.ustart), p(enc.idx), p(enc.vals), N) == -1
    # the typed wrapper checks before any launch
    with pytest.raises(ValueError):
        dense.pack(enc)
    with pytest.raises(ValueError):
        plan.unpack(packed[:-1], enc.ustart)
    with pytest.raises(ValueError):
        plan.unpack(packed.view(torch.int32), enc.ustart)
    with pytest.raises(ValueError):
        plan.unpack(packed, enc.ustart[:-1])
    with pytest.raises(ValueError):
        plan.unpack(packed.cpu(), enc.ustart)
    assert lib.coalac_pack(*good_pack) == 0 and lib.coalac_unpack(*good_unpack) == 0
    torch.cuda.synchronize()


def test_end_to_end_codec(cuda):
    """encode_module -> pickle -> unpickle -> decode_module with compact=True equals the non-compact path bit for bit,
    and the server side moved the packed region (not idx / vals) to the device and unpacked it there."""
    trained = build_module("resnet18_split_cut4", seed=1).cuda()
    glob = build_module("resnet18_split_cut4", seed=2).cuda()
    results, staged, blobs = [], {}, {}
    for compact in (False, True):
        codec = UpdateCodec(0.01, 4, "delta", compact=compact, recycle=False)
        base = codec.snapshot(glob)
        up = codec.encode_module(trained, base=base)
        assert (up.packed is not None) == compact and (not compact or up.packed.is_cuda)
        blob = blobs[compact] = pickle.dumps(up)
        back = pickle.loads(blob)
        assert back.encoded.idx.device.type == "cpu" and torch.equal(back.encoded.idx, up.encoded.idx.cpu())
        assert torch.equal(back.encoded.vals, up.encoded.vals.cpu())
        sizes = staged[compact] = []
        inner = codec._staging
        codec._staging = lambda n, inner=inner, sizes=sizes: (sizes.append(n), inner(n))[1]
        results.append((codec.decode_module(back, glob, base=base).state_dict(), back))
    (plain, pu), (comp, cu) = results
    for (k, a), (k2, b) in zip(plain.items(), comp.items()):
        assert k == k2 and a.dtype == b.dtype and torch.equal(a, b), k
    for compact, u in ((False, pu), (True, cu)):
        _, sec = wire.sections(u.to_bytes())
        assert staged[compact] == [sec["ustart"][0] + sec["ustart"][1] - sec["mn"][0]]
    h = cu.header
    T, K, U = h["n_segments"], h["total_k"], h["n_units"]
    assert staged[True][0] <= 8 * T + 4 * ((K * 16 + 31) // 32) + 4 * U + 4 * 16  # mn, scale, packed, ustart (+ padding)
    assert staged[True][0] < staged[False][0] - 2 * K  # 2 bytes per entry instead of 5
    assert cu.nbytes < pu.nbytes and len(blobs[True]) < len(blobs[False])
