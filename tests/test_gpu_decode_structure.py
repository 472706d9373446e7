"""coalac_decode (k_decode_lds) and coalac_ef_commit (k_ef_commit) on hand-built payloads: all 16 variants of the decode
kernel (raw or codes x base or none x high_ratio or not x latency or batch plan), the whole output buffer, in place, from
device-computed starts, corrupt batch payloads.

Payloads come from tests/decode_inputs.py, placed entry by entry into plan.empty_encoded(): per unit a count and a set
of positions, which is what decides the register chunks against the reload loop, and whether a slot of the LDS tile is
used by one pass and read by the next. The expected buffer is tests/aggregate_model.decode (the oracle's arithmetic,
decoded unit by unit from the payload's own starts); tests/test_decode_model_cpu.py proves it equal to
oracle.codec_oracle.decode on every valid payload, race-free on the corrupt ones, and every case's claim true, without
a GPU.

`out` is always span + 64 elements of a sentinel and the WHOLE buffer is compared bit for bit (NaN for NaN): the
segments' elements, the sentinel in every alignment pad and in the tail. No tolerance anywhere."""
import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, Encoded
from tests import aggregate_inputs as I
from tests import decode_inputs as D
from tests import ef_model as EF

pytestmark = pytest.mark.gpu

_plans = {}
_inside = {}


def plan_of(p):
    key = (tuple(p.table.sizes), p.table.ratio, p.bits)
    if key not in _plans:
        _plans[key] = CodecPlan(p.table.sizes, p.table.ratio, p.bits)
    return _plans[key]


def upload(plan, p):
    """The payload in the plan's own encoded buffers (one allocation, as an encode leaves it)."""
    enc = plan.empty_encoded()
    for name in ("idx", "vals", "mn", "scale", "ustart"):
        dst, src = getattr(enc, name), getattr(p, name)
        assert dst.numel() == src.size, name
        dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))
    return enc


def inside_dev(table):
    """bool[span + PAD] on the device: the segments' elements (one mask per layout, at most two kept)."""
    key = tuple(table.sizes)
    if key not in _inside:
        if len(_inside) >= 2:
            _inside.pop(next(iter(_inside)))
        _inside[key] = torch.from_numpy(D.inside(table, table.span_per_client + I.PAD)).cuda()
    return _inside[key]


def sentinel_out(p):
    return torch.full((p.table.span_per_client + I.PAD,), float(I.SENTINEL), dtype=torch.float32, device="cuda")


def same_bits(g, ref):
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(g), nan)
    np.testing.assert_array_equal(g[~nan].view(np.uint32), ref[~nan].view(np.uint32))


def same_bits_dev(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def decode_whole_buffer(p):
    """decode(p) into a sentinel buffer == the model, over the whole buffer; returns what the other checks reuse."""
    plan = plan_of(p)
    assert plan.n_units == p.table.n_units and not plan.dense
    enc = upload(plan, p)
    base = None if p.base is None else torch.from_numpy(p.base).cuda()
    out = sentinel_out(p)
    got = plan.decode(enc, base=base, out=out)
    torch.cuda.synchronize()
    assert got is out
    ref, counts = D.expected_decode(p)
    same_bits(out.cpu().numpy(), ref)
    return plan, enc, base, out, counts


@pytest.mark.parametrize("name,ratio,batch,bits,base", D.VALID_CASES)
def test_valid_payload(cuda, name, ratio, batch, bits, base):
    """Every valid case of decode_inputs.CASES (each generator's comment says which path it reaches), in every plan
    class it applies to, with and without a base, at bits 8 and 32 (1 and 5 too for one case per plan class):

    (a) the whole buffer equals the model;
    (b) without the payload's starts (a v1 payload: CodecPlan.unit_starts on the device) the buffer is identical;
    (c) with a base, decoding in place (out is the base tensor, sentinel beyond the span) gives the same segments and
        leaves every other element as it was;
    (d) ef_commit of the same payload on a residual with the sentinel in its pads equals ef_model.commit over the whole
        buffer, and changes something (not the special-value cases, which the commit model leaves out)."""
    p = D.valid(name, ratio, batch, bits, base)
    plan, enc, b, out, counts = decode_whole_buffer(p)
    assert (counts.applied, counts.dropped) == (p.table.total_k, 0)

    out_v1 = sentinel_out(p)
    plan.decode(Encoded(enc.idx, enc.vals, enc.mn, enc.scale), base=b, out=out_v1)
    assert same_bits_dev(out_v1, out), "decode from device-computed starts differs"
    del out_v1

    ins = inside_dev(p.table)
    if b is not None:
        span = p.table.span_per_client
        buf = sentinel_out(p)
        buf[:span] = b
        want = torch.where(ins, out, buf)
        got = plan.decode(enc, base=buf, out=buf)
        assert got is buf
        assert same_bits_dev(buf, want), "in-place decode (out is base) differs"
        del buf, want

    if D.CASES[name].commit:
        a = D.residual(p.table)
        resid = torch.from_numpy(a.copy()).cuda()
        plan.ef_commit(enc, resid)
        ref = EF.commit(a, p.idx, p.vals, p.mn, p.scale, p.segs, p.bits)
        assert np.any(ref.view(np.uint32) != a.view(np.uint32))
        same_bits(resid.cpu().numpy(), ref)


@pytest.mark.parametrize("kind,ratio,bits,base", D.CORRUPT_CASES)
def test_corrupt_batch_payload_matches_model(cuda, kind, ratio, bits, base):
    """The batch plan's decode of wrong starts (+1, random in [0, k], int32 garbage, all 0xFFFFFFFF) and wrong
    indices (moved into the neighbouring unit, top bit set, >= n, and len <= pos < 4096 in a partial last unit):
    the whole buffer equals the model — what the clamp lets through is decoded, what lies outside its unit is
    dropped, the pad after every segment keeps the sentinel."""
    p = D.corrupt(kind, ratio, bits, base)
    plan, enc, b, out, counts = decode_whole_buffer(p)
    assert counts.applied < p.table.total_k
