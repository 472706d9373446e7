"""The stochastic-rounding kernels (k_dense_quant_sr / k_dense_block_quant_sr) against the numpy model
(tests/sr_model.py) through the C ABI: every comparison is bit-exact (a NaN range compares as NaN). One layout for all
tests — its odd sizes leave later segments' codes off a dword (the byte-store branch), its last units are ragged, one
segment has a single element — with N(0,1) data plus a segment of NaN / +-inf, a constant one and one whose values sit
within a few ulps of integer quotients."""
import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, wire
from oracle import codec_oracle as O
from tests import blockwise_model as BM
from tests import dense_aggregate_model as DM
from tests import sr_model as M

pytestmark = pytest.mark.gpu

UNIT = 4096
SIZES = [1, 3, 5, 1023, 4096, 4097, 2 * 4096 + 517]
SEED = 0xC0FFEE1234567890
SENTINEL = 123.25
_PLANS = {}


def _plan(kind, bits):
    key = (kind, bits)
    if key not in _PLANS:
        _PLANS[key] = CodecPlan(SIZES if kind == "plain" else SIZES[:4] + [0] + SIZES[4:], 1.0, bits)
    return _PLANS[key]


def _near_integer_quotients(rng, n, bits):
    """mn, mx and n - 2 values within 3 ulps of mn + k * scale, inside [mn, mx]: the quotients land on, just below and
    just above integers."""
    levels = np.float32((1 << bits) - 1)
    mn, mx = np.float32(-1.375), np.float32(2.640625)
    sc = np.float32((mx - mn) / levels)
    ks = rng.integers(0, int(levels) + 1, n - 2).astype(np.float32)
    x = (mn + ks * sc).astype(np.float32)
    x = (x.view(np.int32) + rng.integers(-3, 4, n - 2).astype(np.int32)).view(np.float32)
    return np.concatenate([[mn, mx], np.clip(x, mn, mx)]).astype(np.float32)


def _data(plan, bits, seed):
    rng = np.random.default_rng(seed)
    segs = plan.table.segs.astype(np.int64)
    flat = np.zeros(plan.span, np.float32)
    for off, n, _, _ in segs.tolist():
        flat[off:off + n] = rng.standard_normal(n).astype(np.float32)
    by_n = {int(n): int(off) for off, n, _, _ in segs.tolist()}
    flat[by_n[3]:by_n[3] + 3] = -2.5                                    # a constant segment: scale 0
    o = by_n[1023]
    flat[o + 5:o + 1023:97] = np.nan
    flat[o + 7], flat[o + 11] = np.inf, -np.inf                          # an infinite range
    flat[by_n[4096]:by_n[4096] + 4096] = _near_integer_quotients(rng, 4096, bits)
    o = by_n[4097]
    flat[o + 1:o + 4097:211] = np.nan                                    # NaN elements inside a finite range
    return flat


def _same_ranges(got, want):
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def _inputs(plan, flat, segptr):
    if segptr:
        segs = plan.table.segs.astype(np.int64).tolist()
        return {"tensors": [torch.from_numpy(flat[off:off + n].copy()).cuda() for off, n, _, _ in segs]}
    return {"flat": torch.from_numpy(flat).cuda()}


@pytest.mark.parametrize("segptr", [False, True], ids=["flat", "segptr"])
@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("bits", [1, 2, 4, 7, 8])
@pytest.mark.parametrize("kind", ["plain", "empty"])  # (an empty segment: k_dense_seg, the quantise without SEGRED)
def test_encode_sr(cuda, kind, bits, delta, segptr):
    plan = _plan(kind, bits)
    segs = plan.table.segs.astype(np.int64)
    flat = _data(plan, bits, bits)
    base = np.random.default_rng(50 + bits).standard_normal(plan.span).astype(np.float32) if delta else None
    codes, mn, sc = M.encode(flat, segs, bits, SEED, base=base)
    K = plan.total_k
    assert (codes != O.encode(flat, segs, bits, base=base)[1]).any()
    out = plan.empty_encoded(with_idx=False)
    vbuf = torch.full((16 + K + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    out.vals = vbuf[16:16 + K]
    dbase = None if base is None else torch.from_numpy(base).cuda()
    enc = plan.encode_sr(base=dbase, seed=SEED, out=out, **_inputs(plan, flat, segptr))
    torch.cuda.synchronize()
    v = vbuf.cpu().numpy()
    np.testing.assert_array_equal(v[16:16 + K], codes)
    assert (v[:16] == 0xAB).all() and (v[16 + K:] == 0xAB).all()
    _same_ranges(enc.mn.cpu().numpy(), mn)
    _same_ranges(enc.scale.cpu().numpy(), sc)
    # the codes are ordinary codes: pack_dense and the decode of the stream read them as they are
    packed = plan.pack_dense(enc)
    dec = plan.decode_packed(packed, enc.mn, enc.scale, base=dbase)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(packed.cpu().numpy(), wire.pack_dense_codes(codes, segs[:, 1], bits, out_off=segs[:, 3]))
    idx = np.concatenate([np.arange(n, dtype=np.int32) for n in segs[:, 1]])
    ref = O.decode(idx, codes, mn, sc, segs, bits, plan.span, base=base)
    got = dec.cpu().numpy()
    for off, n, _, _ in segs.tolist():
        _same_ranges(got[off:off + n], ref[off:off + n])


@pytest.mark.parametrize("segptr", [False, True], ids=["flat", "segptr"])
@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
@pytest.mark.parametrize("bits", [1, 2, 3, 4, 5, 8])  # (3, 5: the fields straddle words)
def test_encode_block_sr(cuda, bits, delta, segptr):
    plan = _plan("plain", bits)
    segs = plan.table.segs.astype(np.int64)
    U, P = plan.n_units, plan.dense_packed_words
    flat = _data(plan, bits, 20 + bits)
    base = np.random.default_rng(70 + bits).standard_normal(plan.span).astype(np.float32) if delta else None
    bmn, bsc, _, stream = M.encode_block(flat, segs, bits, SEED, base=base)
    assert (stream != BM.encode(flat, segs, bits, base=base)[3]).any()
    rbuf = torch.full((2, 64 + U + 64), SENTINEL, dtype=torch.float32, device="cuda")
    obuf = torch.full((16 + P + 64,), 0xFFFFFFFF, dtype=torch.uint32, device="cuda")
    dbase = None if base is None else torch.from_numpy(base).cuda()
    plan.encode_block_sr(base=dbase, seed=SEED, out=(rbuf[0, 64:64 + U], rbuf[1, 64:64 + U], obuf[16:]),
                         **_inputs(plan, flat, segptr))
    dec = plan.decode_block(obuf[16:], rbuf[0, 64:64 + U], rbuf[1, 64:64 + U], base=dbase)
    torch.cuda.synchronize()
    r, o = rbuf.cpu().numpy(), obuf.cpu().numpy()
    _same_ranges(r[0, 64:64 + U], bmn)
    _same_ranges(r[1, 64:64 + U], bsc)
    np.testing.assert_array_equal(o[16:16 + P], stream)  # (the padding bits and the codes past a ragged unit's end: zero)
    assert (r[:, :64] == SENTINEL).all() and (r[:, 64 + U:] == SENTINEL).all()
    assert (o[:16] == 0xFFFFFFFF).all() and (o[16 + P:] == 0xFFFFFFFF).all()
    ref = BM.decode(stream, bmn, bsc, segs, bits, plan.span, base=base)
    got = dec.cpu().numpy()
    for off, n, _, _ in segs.tolist():
        _same_ranges(got[off:off + n], ref[off:off + n])


@pytest.mark.parametrize("delta", [False, True], ids=["weights", "delta"])
def test_batch_plan_reaches_the_xcd_unit_order(cuda, delta):
    """More than 8192 units (most of them tiny, so the model stays quick): both stochastic kernels take the XCD-aware
    unit order."""
    sizes, clients, bits = [1, 3, 5, 33, UNIT + 1], 1400, 4
    plan = CodecPlan(sizes, 1.0, bits, clients=clients)
    assert plan.n_units == 6 * clients > 8192
    segs = plan.table.segs.astype(np.int64)
    rng = np.random.default_rng(5)
    flat = rng.standard_normal(plan.span, dtype=np.float32)
    base = rng.standard_normal(plan.span, dtype=np.float32) if delta else None
    dflat, dbase = torch.from_numpy(flat).cuda(), None if base is None else torch.from_numpy(base).cuda()
    enc = plan.encode_sr(flat=dflat, base=dbase, seed=SEED)
    bmn, bsc, packed = plan.encode_block_sr(flat=dflat, base=dbase, seed=SEED + 1)
    torch.cuda.synchronize()
    codes, mn, sc = M.encode(flat, segs, bits, SEED, base=base)
    np.testing.assert_array_equal(enc.vals.cpu().numpy(), codes)
    _same_ranges(enc.mn.cpu().numpy(), mn)
    _same_ranges(enc.scale.cpu().numpy(), sc)
    wmn, wsc, _, stream = M.encode_block(flat, segs, bits, SEED + 1, base=base)
    np.testing.assert_array_equal(packed.cpu().numpy(), stream)
    _same_ranges(bmn.cpu().numpy(), wmn)
    _same_ranges(bsc.cpu().numpy(), wsc)


@pytest.mark.parametrize("bits", [2, 8])
def test_positions_beyond_2_32(cuda, bits):
    """An explicit-row plan whose in_off lie at and beyond 2^32, read through tensors= without a base (in_off indexes no
    memory there): the high word of the position enters the hash — per lane in the unit that crosses 2^32, once per
    wave in the others."""
    rows = np.array([((1 << 32) - 400, UNIT + 50, UNIT + 50, 0),      # its first unit crosses 2^32
                     ((1 << 32) + 8192, 1000, 1000, UNIT + 50),
                     ((5 << 32) - 4, 7, 7, UNIT + 1050),               # crosses 5 * 2^32 inside a 7-element unit
                     ((1 << 45) + 64, UNIT, UNIT, UNIT + 1057)], dtype=np.uint64)
    plan = CodecPlan.from_segments(rows, bits)
    assert plan.dense and plan.n_units == 5
    rng = np.random.default_rng(bits)
    xs = [rng.standard_normal(int(n)).astype(np.float32) for n in rows[:, 1]]
    tensors = [torch.from_numpy(x).cuda() for x in xs]
    enc = plan.encode_sr(tensors=tensors, seed=SEED)
    bmn, bsc, packed = plan.encode_block_sr(tensors=tensors, seed=SEED)
    torch.cuda.synchronize()
    got, K = enc.vals.cpu().numpy(), plan.total_k
    want, bwant = np.zeros(K, np.uint8), np.zeros(K, np.uint8)
    low = np.zeros(K, np.uint8)  # what the low word alone would give
    u = 0
    for (off, n, _, oo), x in zip(rows.astype(np.int64).tolist(), xs):
        _, mn, sc = O.quantize(x, bits)
        want[oo:oo + n] = M.sr_codes(x, mn, sc, bits, SEED, off)
        low[oo:oo + n] = M.sr_codes(x, mn, sc, bits, SEED, off & 0xFFFFFFFF)
        for a in range(0, n, UNIT):
            xb = x[a:a + UNIT]
            _, m, s = O.quantize(xb, bits)
            bwant[oo + a:oo + a + xb.size] = M.sr_codes(xb, m, s, bits, SEED, off + a)
            assert bmn[u].item() == m and bsc[u].item() == s
            u += 1
    np.testing.assert_array_equal(got, want)
    assert (want != low).any()
    segs = rows.astype(np.int64)
    np.testing.assert_array_equal(packed.cpu().numpy(), wire.pack_dense_codes(bwant, segs[:, 1], bits, out_off=segs[:, 3]))


def test_abi_errors(cuda):
    plan = _plan("plain", 4)
    sparse, raw = CodecPlan([5000, 300], 0.1, 4), CodecPlan([64, 8], 1.0, 32)
    x = torch.zeros(plan.span, device="cuda")
    for wrong in (sparse, raw):
        with pytest.raises(ValueError):
            wrong.encode_sr(flat=x, seed=1)
        with pytest.raises(ValueError):
            wrong.encode_block_sr(flat=x, seed=1)
    for call in (lambda: plan.encode_sr(seed=1), lambda: plan.encode_sr(flat=x, tensors=[x], seed=1),
                 lambda: plan.encode_sr(flat=x[:-8], seed=1), lambda: plan.encode_sr(flat=x.cpu(), seed=1),
                 lambda: plan.encode_block_sr(seed=1), lambda: plan.encode_block_sr(flat=x, tensors=[x], seed=1),
                 lambda: plan.encode_block_sr(flat=x[4:], seed=1)):
        with pytest.raises(ValueError):
            call()
    a, b = plan.encode_sr(flat=x, seed=1), plan.encode_sr(flat=x, seed=1 + (1 << 64))  # (the seed is taken mod 2^64)
    assert torch.equal(a.vals, b.vals)


def test_fused_average_of_64_stochastic_uploads(cuda):
    """The point of the feature, on the fused path: 64 block-wise 2-bit stochastic uploads of one N(0,1) tensor set,
    distinct seeds, through coalac_aggregate_dense (kind BLOCK, equal weights). Bit-identical to the model's
    decode-each + FedAvg, and its RMS error against the input is below 0.25 x that of the deterministic block-wise
    encode's decode (the model alone: 0.15-0.18; identical round-to-nearest uploads: 1.0)."""
    bits, C = 2, 64
    plan = _plan("plain", bits)
    segs = plan.table.segs.astype(np.int64)
    inside = np.zeros(plan.span, bool)
    for off, n, _, _ in segs.tolist():
        inside[off:off + n] = True
    flat = np.where(inside, np.random.default_rng(64).standard_normal(plan.span), 0).astype(np.float32)
    dflat = torch.from_numpy(flat).cuda()
    ups = [plan.encode_block_sr(flat=dflat, seed=M_seed) for M_seed in (SEED + 977 * i for i in range(C))]
    det = plan.decode_block(*[plan.encode_block(flat=dflat)[i] for i in (2, 0, 1)])
    out = plan.aggregate_dense([u[2] for u in ups], [u[0] for u in ups], [u[1] for u in ups], [1] * C, kind="block",
                               mode="recip", out=torch.zeros(plan.span, device="cuda"))
    torch.cuda.synchronize()
    model = [M.encode_block(flat, segs, bits, SEED + 977 * i) for i in range(C)]
    for u, m in zip(ups[::21], model[::21]):
        np.testing.assert_array_equal(u[2].cpu().numpy(), m[3])
    want = DM.expected("block", [m[3] for m in model], [m[0] for m in model], [m[1] for m in model], segs, bits,
                       [1] * C, float(C), "recip", plan.span)
    got = out.cpu().numpy()
    DM.same_bits(got[inside], want[inside])
    x = flat[inside].astype(np.float64)
    rms = np.sqrt(((got[inside] - x) ** 2).mean())
    rms_det = np.sqrt(((det.cpu().numpy()[inside] - x) ** 2).mean())
    print(f"rms(fused mean of {C} stochastic uploads) / rms(round to nearest) = {rms / rms_det:.4f}")
    assert rms < 0.25 * rms_det
