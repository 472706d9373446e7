"""The model of block-wise dense quantisation with 256- and 1024-element blocks — a helper, not a test.

The contract restated on the CPU: a block-wise encode with block size G is the existing oracle's dense encode of the
same data over a segment table in which every segment has been cut into its G-element blocks (split_table) — CodecSpec
v1 applied to each block as if it were a segment of its own with k = n. Blocks are numbered segment by segment in row
order, ceil(n / G) each. The code stream is wire v4's over the ORIGINAL segments (wire.pack_dense_codes), whatever G is.
At G = 4096 this is tests/blockwise_model.py. SubblockOraclePlan puts the model behind the plan interface
(encode_block_g / decode_block_g / aggregate_dense_g), so the host code runs on the CPU.
"""
import numpy as np
import torch

from coala_amd.compression import wire
from oracle import codec_oracle as O
from tests.dense_aggregate_model import MODES, DenseAggOracleBackend, DenseAggOraclePlan, clients_table, codes_of

SIZES = (256, 1024, 4096)


def split_table(segs, block):
    """Rows (in_off, n, k = n, out_off) -> one row per `block`-element block, in block order."""
    rows = []
    for off, n, k, oo in np.asarray(segs, dtype=np.int64).reshape(-1, 4).tolist():
        assert k == n, "block-wise quantisation is defined for dense plans"
        rows += [(off + a, min(block, n - a), min(block, n - a), oo + a) for a in range(0, n, block)]
    return np.asarray(rows, dtype=np.int64).reshape(-1, 4)


def _total(segs):
    return int((segs[:, 3] + segs[:, 2]).max()) if len(segs) else 0


def encode(flat, segs, bits, block, base=None):
    """-> (bmn fp32[NB], bscale fp32[NB], codes uint8[max(out_off + n)], stream uint32[P])."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    _, vals, mn, sc = O.encode(flat, split_table(segs, block), bits, base=base)
    codes = np.zeros(_total(segs), dtype=np.uint8)
    codes[:vals.size] = vals
    return mn, sc, codes, wire.pack_dense_codes(codes, segs[:, 1], bits, out_off=segs[:, 3])


def _implied(rows, total):
    idx = np.zeros(total, dtype=np.int32)
    for _, n, _, oo in rows.tolist():
        idx[oo:oo + n] = np.arange(n, dtype=np.int32)
    return idx


def decode(stream, mn, scale, segs, bits, span, block, base=None, out=None):
    """The oracle's decode of the stream's codes over the split table (padding bits ignored; positions outside the
    segments: 0 / base, or `out`'s own)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    codes = codes_of(stream, segs, bits)
    rows = split_table(segs, block)
    return O.decode(_implied(rows, _total(rows)), codes, mn, scale, rows, bits, span, base=base, out=out)


def aggregate(streams, mns, scales, segs, bits, block, weights, total, mode, span, base=None, avg_mask=None):
    """Decode each upload and FedAvg, in client order (oracle.codec_oracle.aggregate over the clients' split tables):
    streams / mns / scales per client, one range per block. -> fp32[span] (positions outside the segments: 0)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    C = len(streams)
    rows, K = clients_table(segs, C)
    vals = np.zeros(C * K, dtype=np.uint8)
    for c, q in enumerate(streams):
        vals[c * K:c * K + K] = codes_of(np.asarray(q), segs, bits)[:K]
    mask = None
    if avg_mask is not None:
        mask = [bool(m) for m, n in zip(avg_mask, segs[:, 1].tolist()) for _ in range((n + block - 1) // block)]
    rows = split_table(rows, block)
    mn = np.concatenate([np.asarray(m, dtype=np.float32) for m in mns])
    sc = np.concatenate([np.asarray(s, dtype=np.float32) for s in scales])
    assert len(mn) == len(sc) == len(rows), "one range per block and client"
    return O.aggregate(_implied(rows, C * K), vals, mn, sc, rows, bits, C, weights, total, MODES[mode], base=base,
                       out_span=span, avg_mask=mask)


def rms_error(x, bits, block):
    """RMS of x - decode(encode(x)) for one dense segment holding x, with `block`-element blocks."""
    x = np.asarray(x, dtype=np.float32)
    segs = np.array([[0, x.size, x.size, 0]], dtype=np.int64)
    mn, sc, _, stream = encode(x, segs, bits, block)
    d = decode(stream, mn, sc, segs, bits, x.size, block)
    return float(np.sqrt(np.mean((d.astype(np.float64) - x.astype(np.float64)) ** 2)))


class SubblockOraclePlan(DenseAggOraclePlan):
    has_block_g = True

    def block_count(self, block=4096):
        return wire.block_count(self.table.segs[:, 1], block)

    def encode_block_g(self, block, flat=None, tensors=None, base=None, **_):
        segs = self.table.segs.astype(np.int64)
        if tensors is not None:
            x = np.zeros(self.table.span, dtype=np.float32)
            for (off, n, _, _), t in zip(segs.tolist(), tensors):
                x[off:off + n] = t.detach().cpu().numpy().reshape(-1)
        else:
            x = flat.detach().cpu().numpy()
        b = None if base is None else base.detach().cpu().numpy()
        mn, sc, _, stream = encode(x, segs, self.bits, block, base=b)
        return torch.from_numpy(mn), torch.from_numpy(sc), torch.from_numpy(stream)

    def decode_block_g(self, block, packed, bmn, bscale, base=None, out=None, **_):
        b = None if base is None else base.detach().cpu().numpy()
        res = np.zeros(self.table.span, dtype=np.float32) if b is None else b.copy()
        decode(packed.numpy(), bmn.numpy(), bscale.numpy(), self.table.segs.astype(np.int64), self.bits, self.table.span,
               block, base=b, out=res)
        if out is not None:
            out[:res.size].copy_(torch.from_numpy(res))
            return out
        return torch.from_numpy(res)

    def aggregate_dense_g(self, block, codes, mns, scales, weights, total=None, base=None, out=None, mode="div",
                          avg_mask=None, **_):
        type(self).calls += 1
        total = float(sum(weights)) if total is None else float(total)
        b = None if base is None else base.detach().cpu().numpy()
        res = aggregate([c.numpy() for c in codes], [m.numpy() for m in mns], [s.numpy() for s in scales],
                        self.table.segs.astype(np.int64), self.bits, block, weights, total, mode, self.table.span, base=b,
                        avg_mask=avg_mask)
        if out is not None:
            out[:res.size].copy_(torch.from_numpy(res))
            return out
        return torch.from_numpy(res)


class SubblockOracleBackend(DenseAggOracleBackend):
    name = "subblock-oracle"

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        return SubblockOraclePlan(sizes, ratio, bits, clients)
