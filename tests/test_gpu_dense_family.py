"""The dense codec's kernels share one copy of the unit's code addressing, the stream's addressing, the range rule and
the store tail, so the paths through them must agree with each other bit for bit: the plain dense decode,
the stream decoder with one range per segment and per unit, the fused aggregate of one upload in its three kinds, and
pack / unpack as inverses. One plan: test_gpu_dense_pack's SIZES (units whose length is no multiple of 4, a full unit, a
multi-unit segment) and its ROWS (codes that start off a dword, so both branches of the whole-dwords rule run). Code
widths 1 (aligned fields), 3 (fields that straddle a word) and 8 (full width: through the entry points themselves)."""
import ctypes

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan, Encoded, _lib
from tests.test_gpu_dense_pack import ROWS, SENTINEL, SIZES

pytestmark = pytest.mark.gpu

UNIT = 4096
KINDS = ("codes", "packed", "block")


def _rows():
    """SIZES as contiguous rows (in_off a multiple of 4), then ROWS behind them with their own gaps and odd out_off."""
    rows, in_off, out_off = [], 0, 0
    for n in SIZES:
        rows.append((in_off, n, n, out_off))
        in_off, out_off = (in_off + n + 3) // 4 * 4, out_off + n
    rows += [(in_off + i, n, k, out_off + o) for i, n, k, o in ROWS]
    return np.array(rows, dtype=np.uint64)


class _Case:
    def __init__(self, bits):
        self.plan = plan = CodecPlan.from_segments(_rows(), bits)
        assert plan.dense
        rng = np.random.default_rng(bits)
        segs = plan.table.segs.astype(np.int64)
        codes = np.full(plan.total_k, 0xFF, dtype=np.uint8)
        self.own = np.zeros(plan.total_k, dtype=bool)
        for _, n, _, oo in segs:
            codes[oo:oo + n] = rng.integers(0, 1 << bits, n)
            self.own[oo:oo + n] = True
        assert any((oo % 4 == 0 and n % 4 == 0) for _, n, _, oo in segs) and any(oo % 4 for _, n, _, oo in segs)
        mn = rng.standard_normal(len(segs)).astype(np.float32)
        scale = (np.abs(rng.standard_normal(len(segs))) * 0.01).astype(np.float32)
        scale[::3] = 0.0
        unit_seg = np.repeat(np.arange(len(segs)), (segs[:, 1] + UNIT - 1) // UNIT)
        assert unit_seg.size == plan.n_units
        d = lambda a: torch.from_numpy(a).cuda()
        self.codes, self.mn, self.scale = d(codes), d(mn), d(scale)
        self.bmn, self.bscale = d(mn[unit_seg]), d(scale[unit_seg])  # every unit's range: its segment's
        self.base = d(rng.standard_normal(plan.span).astype(np.float32))
        self.weight = torch.ones(1, device="cuda")
        self.abi = bits == 8
        self.lib = _lib.load()

    def fresh(self):
        return torch.full((self.plan.span + 64,), SENTINEL, dtype=torch.float32, device="cuda")

    def _call(self, name, *args):
        def p(a):  # a tensor's address, NULL for None; everything else is a ctypes value already
            if a is None:
                return ctypes.c_void_p(0)
            return ctypes.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a

        assert getattr(self.lib, name)(self.plan._h, *[p(a) for a in args]) == 0, self.lib.coalac_last_error()

    def pack(self):
        if not self.abi:
            return self.plan.pack_dense(self.codes)
        out = torch.empty(self.plan.dense_packed_words, dtype=torch.uint32, device="cuda")
        self._call("coalac_pack_dense", self.codes, out, ctypes.c_uint64(4 * out.numel()), None)
        return out

    def unpack(self, stream, out):
        if not self.abi:
            return self.plan.unpack_dense(stream, out=out)
        self._call("coalac_unpack_dense", stream, ctypes.c_uint64(4 * stream.numel()), out, None)
        return out

    def decode_stream(self, per_unit, stream, r0, r1, base):
        out = self.fresh()
        if not self.abi:
            return (self.plan.decode_block if per_unit else self.plan.decode_packed)(stream, r0, r1, base=base, out=out)
        self._call("coalac_decode_block" if per_unit else "coalac_decode_packed", stream,
                   ctypes.c_uint64(4 * stream.numel()), r0, r1, base, out, None)
        return out

    def aggregate(self, kind, c, m, s, base):
        """one client, weight 1, mode sum: -0.0 + x * 1.0 is x itself"""
        out = self.fresh()
        if not self.abi:
            return self.plan.aggregate_dense([c], [m], [s], [1.0], total=1.0, base=base, out=out, mode="sum", kind=kind)
        ptrs = torch.tensor([c.data_ptr(), m.data_ptr(), s.data_ptr()], dtype=torch.int64).cuda()
        at = lambda i: ctypes.c_void_p(ptrs.data_ptr() + 8 * i)
        self._call("coalac_aggregate_dense", 1, CodecPlan.AGG_DENSE_KINDS[kind], at(0),
                   ctypes.c_uint64(c.numel() * c.element_size()), at(1), at(2), self.weight, ctypes.c_float(1.0),
                   _lib.COALAC_AGG_SUM, None, base, out, None)
        torch.cuda.synchronize()  # (ptrs lives until the kernel has read it)
        return out


_CASES = {}


def _case(bits):
    if bits not in _CASES:
        _CASES[bits] = _Case(bits)
    return _CASES[bits]


def _same(a, b):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("bits", [1, 3, 8])
def test_unpack_inverts_pack(cuda, bits):
    c = _case(bits)
    back = c.unpack(c.pack(), torch.full((c.plan.total_k,), 0xA5, dtype=torch.uint8, device="cuda")).cpu().numpy()
    np.testing.assert_array_equal(back[c.own], c.codes.cpu().numpy()[c.own])
    assert (back[~c.own] == 0xA5).all()  # positions no segment owns are not written


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("bits", [1, 3, 8])
def test_decoders_agree(cuda, bits, with_base):
    c = _case(bits)
    base = c.base if with_base else None
    stream = c.pack()
    want = c.plan.decode(Encoded(torch.empty(0, dtype=torch.int32, device="cuda"), c.codes, c.mn, c.scale), base=base,
                         out=c.fresh())
    assert (want[c.plan.span:] == SENTINEL).all() and (want[:c.plan.span] != SENTINEL).any()
    # whole buffers compare: the values, and the sentinel wherever no segment lies
    _same(c.decode_stream(False, stream, c.mn, c.scale, base), want)
    _same(c.decode_stream(True, stream, c.bmn, c.bscale, base), want)
    operands = {"codes": (c.codes, c.mn, c.scale), "packed": (stream, c.mn, c.scale), "block": (stream, c.bmn, c.bscale)}
    for kind in KINDS:
        _same(c.aggregate(kind, *operands[kind], base), want)
