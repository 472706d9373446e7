"""coalac_aggregate (k_aggregate) on hand-built uploads: every kernel path, the whole output buffer, corrupt uploads.

Payloads come from tests/aggregate_inputs.py, placed entry by entry into plan.empty_encoded(): per client and unit a
count and a set of positions, which is what picks k_aggregate's branch per (unit, 64-client chunk, wave). The expected
result is tests/aggregate_model.py (the oracle's arithmetic, decoded unit by unit from the payload's own starts), whose
equality with oracle.codec_oracle.aggregate on valid payloads and whose race-freedom on the corrupt ones
tests/test_aggregate_model_cpu.py proves without a GPU.

`out` is always span_per_client + 64 elements of a sentinel and the WHOLE buffer is compared bit for bit (NaN for NaN):
the segments' elements, the sentinel in every alignment pad between segments and in the tail. No tolerance anywhere."""
import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan
from oracle import codec_oracle as O
from tests import aggregate_inputs as I
from tests import aggregate_model as M

pytestmark = pytest.mark.gpu

MODES = {"recip": O.AGG_RECIP, "div": O.AGG_DIV, "sum": O.AGG_SUM}
_plans = {}


def plan_of(p):
    key = (tuple(p.table.sizes), p.table.ratio, p.bits, p.clients)
    if key not in _plans:
        _plans[key] = CodecPlan(p.table.sizes, p.table.ratio, p.bits, clients=p.clients)
    return _plans[key]


def upload(plan, p):
    """The payload in the plan's own encoded buffers (one allocation, as an encode leaves it), and its base."""
    enc = plan.empty_encoded()
    for name in ("idx", "vals", "mn", "scale", "ustart"):
        dst, src = getattr(enc, name), getattr(p, name)
        assert dst.numel() == src.size, name
        dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    return enc, None if p.base is None else torch.from_numpy(p.base).cuda()


def sentinel_out(p):
    return torch.full((p.table.span_per_client + I.PAD,), float(I.SENTINEL), dtype=torch.float32, device="cuda")


def expected(p, mode):
    out = np.full(p.table.span_per_client + I.PAD, I.SENTINEL, np.float32)
    counts = M.aggregate(p.idx, p.vals, p.mn, p.scale, p.ustart, p.segs, p.bits, p.clients, p.weights,
                         sum(p.weights), MODES[mode], out, base=p.base, avg_mask=p.mask)
    return out, counts


def same_bits(g, ref):
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(g), nan)
    np.testing.assert_array_equal(g[~nan].view(np.uint32), ref[~nan].view(np.uint32))


def check_whole_buffer(p, mode):
    plan = plan_of(p)
    enc, base = upload(plan, p)
    out = sentinel_out(p)
    got = plan.aggregate(enc, p.weights, base=base, out=out, mode=mode, avg_mask=p.mask)
    torch.cuda.synchronize()
    assert got is out
    ref, counts = expected(p, mode)
    same_bits(out.cpu().numpy(), ref)
    return plan, enc, base, out, counts


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("base", [True, False])
@pytest.mark.parametrize("bits", [1, 5, 8, 32])
def test_mixed_paths_across_chunks(cuda, bits, base, mode):
    """aggregate_inputs.mixed: in one unit the first 64-client chunk on the fast path and the second on the generic
    one, in another the reverse (heavy clients at j = 0, 15, 16, 63 and at 64), with per-client counts that differ
    across the AGG_DEPTH batches. Every code width class and every division mode."""
    check_whole_buffer(I.mixed(bits, base), mode)


STRUCTURE_REST = [n for n in I.STRUCTURE if n not in (I.ALL_BITS_CASE, "mask_passthrough", "odd_base_half")]


@pytest.mark.parametrize("base", [True, False])
@pytest.mark.parametrize("name", STRUCTURE_REST)
def test_structure_case(cuda, name, base):
    """threshold (exactly 64 / 65 entries), empty ranges (lo == hi == k, lo == hi == 0, k below the unit count),
    half-unit edges (0 / 2047 / 2048 / len - 1, one wave's half only, len 2049), same and disjoint positions over 37
    clients, special mn / scale / weights (Inf, NaN, -0.0, denormals, scale 0; compared NaN for NaN — the kernel's
    fp32 multiply and add keep denormals, as numpy's do): see each generator's docstring for the path it reaches."""
    check_whole_buffer(I.STRUCTURE[name](8, base), "recip")


@pytest.mark.parametrize("base", [True, False])
def test_mask_passthrough_heavy_and_light_client0(cuda, base):
    """70 clients, mode sum: in a non-averaged segment only client 0 is read and only its count picks the path —
    client 0 heavy among light clients, and light among heavy ones."""
    check_whole_buffer(I.mask_passthrough(8, base), "sum")


def test_odd_base_in_one_half_only(cuda):
    """-0.0 / NaN bases in one 2048-element half of a unit: that wave goes generic, its sibling fast, with light and
    with heavy clients in the unit. (A base is what makes a wave odd: there is no run without one.)"""
    check_whole_buffer(I.odd_base_half(8, True), "recip")


@pytest.mark.parametrize("kind,clients,bits,base", I.CORRUPT_CASES)
def test_corrupt_upload_matches_model_and_decode(cuda, kind, clients, bits, base):
    """Wrong starts (+1, random in [0, k], int32 garbage, all 0xFFFFFFFF) and wrong indices (moved into the
    neighbouring unit, top bit set, >= n) — uploads whose result the model defines. (a) the whole buffer equals the
    model: what the clamp lets through is aggregated, nothing is written outside the segments; (b) the segments equal
    coalac_decode of the same corrupt payload per client followed by torch's weighted sum and division on the GPU.
    Together: aggregate and decode clamp identically."""
    p = I.corrupt(kind, clients, bits, base)
    plan, enc, b, out, counts = check_whole_buffer(p, "recip")
    C, S = clients, p.table.span_per_client
    dense = torch.empty(C * S, dtype=torch.float32, device="cuda")
    plan.decode(enc, base=None if b is None else b.repeat(C), out=dense)
    acc = dense[0:S].clone()
    acc *= p.weights[0]
    for i in range(1, C):
        acc += dense[i * S:(i + 1) * S] * p.weights[i]
    ref = torch.div(acc, sum(p.weights))
    torch.cuda.synchronize()
    for off, n in zip(p.table.offsets, p.table.sizes):
        assert torch.equal(out[off:off + n].view(torch.int32), ref[off:off + n].view(torch.int32))


@pytest.mark.parametrize("base", [True, False])
@pytest.mark.parametrize("kind", I.RACY)
def test_racy_upload_stays_in_bounds(cuda, kind, base):
    """All-zero (duplicate) and reversed indices: which of two entries of one range wins a position is a race, so
    only this is asserted — the sentinels are intact, and every segment element is base + 0 or base + (1 + 0.5 q) for
    a code q (one client, weight 1, mode sum, mn 1, scale 0.5)."""
    p = I.racy(kind, base)
    plan = plan_of(p)
    enc, b = upload(plan, p)
    out = sentinel_out(p)
    plan.aggregate(enc, p.weights, base=b, out=out, mode="sum")
    torch.cuda.synchronize()
    g = out.cpu().numpy()
    d = np.concatenate([[np.float32(0)], np.float32(1) + np.arange(256, dtype=np.float32) * np.float32(0.5)])
    ins = np.zeros(g.size, bool)
    for off, n in zip(p.table.offsets, p.table.sizes):
        ins[off:off + n] = True
        seg = g[off:off + n]
        allowed = d[None, :] if p.base is None else p.base[off:off + n, None] + d[None, :]
        assert np.all((seg[:, None] == allowed).any(axis=1))
    assert np.all(g[~ins] == I.SENTINEL)
