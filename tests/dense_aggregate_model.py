"""The model of the dense fused aggregate (coalac_aggregate_dense) — a helper, not a test.

The expected output is the existing oracle's aggregate (oracle.codec_oracle.aggregate: decode every client, then the
reference's weighted sum and division) over IMPLIED indices: a ratio-1 upload keeps every element, so client c's entry
e of a segment is element e. Per-tensor payloads (kinds "codes" and "packed") run over the `clients`-copies table of
the layout; a block-wise payload (kind "block") over tests/blockwise_model.split_table of that table — every
4096-element block a segment of its own, with the avg mask repeated per block. DenseAggOraclePlan puts the model behind
the plan interface (aggregate_dense), so the host routing runs on the CPU.
"""
import numpy as np
import torch

from coala_amd.compression import wire
from oracle import codec_oracle as O
from tests.blockwise_model import UNIT, BlockOracleBackend, BlockOraclePlan, split_table

KINDS = ("codes", "packed", "block")
MODES = {"div": O.AGG_DIV, "recip": O.AGG_RECIP, "sum": O.AGG_SUM}


def clients_table(segs, clients):
    """Rows (in_off, n, k = n, out_off) of ONE layout -> `clients` copies, client-major: client c's entries sit
    c * K behind client 0's (K = the layout's entry count); in_off stays client 0's (the output is indexed by it)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    K = int((segs[:, 3] + segs[:, 2]).max()) if len(segs) else 0
    rows = np.concatenate([segs + np.array([0, 0, 0, c * K], dtype=np.int64) for c in range(clients)])
    return rows, K


def codes_of(stream, segs, bits):
    """A wire v4 stream -> the uint8 codes at out_off + e (padding bits ignored)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    K = int((segs[:, 3] + segs[:, 2]).max()) if len(segs) else 0
    return wire.unpack_dense_codes(np.ascontiguousarray(stream), segs[:, 1], bits, out_off=segs[:, 3],
                                   out=np.zeros(K, dtype=np.uint8))


def expected(kind, codes, mns, scales, segs, bits, weights, total, mode, span, base=None, avg_mask=None):
    """codes: per client, the uint8 codes (kind "codes") or the wire v4 stream (the stream kinds); mns / scales: per
    client, one pair per segment, or per block for kind "block". -> fp32[span] (positions outside the segments: 0)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    C = len(codes)
    rows, K = clients_table(segs, C)
    vals = np.zeros(C * K, dtype=np.uint8)
    for c, q in enumerate(codes):
        q = np.asarray(q)
        vals[c * K:c * K + K] = (q if kind == "codes" else codes_of(q, segs, bits))[:K]
    mask = None if avg_mask is None else [bool(m) for m in avg_mask]
    if kind == "block":
        if mask is not None:
            mask = [m for m, n in zip(mask, segs[:, 1].tolist()) for _ in range((n + UNIT - 1) // UNIT)]
        rows = split_table(rows)
    idx = np.zeros(C * K, dtype=np.int32)
    for _, n, _, oo in rows.tolist():
        idx[oo:oo + n] = np.arange(n, dtype=np.int32)
    mn = np.concatenate([np.asarray(m, dtype=np.float32) for m in mns])
    sc = np.concatenate([np.asarray(s, dtype=np.float32) for s in scales])
    assert len(mn) == len(sc) == len(rows), "one range per segment (or block) and client"
    return O.aggregate(idx, vals, mn, sc, rows, bits, C, weights, total, MODES[mode], base=base, out_span=span,
                       avg_mask=mask)


def same_bits(got, want):
    """Bit-exact; a NaN compares as NaN (its payload is not part of the spec, tests/test_gpu_blockwise.py)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan)
    np.testing.assert_array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


class DenseAggOraclePlan(BlockOraclePlan):
    calls = 0  # (class-wide: the routing tests count the launches)

    def aggregate_dense(self, codes, mns, scales, weights, total=None, base=None, out=None, mode="div",
                        avg_mask=None, kind="codes", **_):
        type(self).calls += 1
        total = float(sum(weights)) if total is None else float(total)
        b = None if base is None else base.detach().cpu().numpy()
        res = expected(kind, [c.numpy() for c in codes], [m.numpy() for m in mns], [s.numpy() for s in scales],
                       self.table.segs.astype(np.int64), self.bits, weights, total, mode, self.table.span, base=b,
                       avg_mask=avg_mask)
        if out is not None:
            out[:res.size].copy_(torch.from_numpy(res))
            return out
        return torch.from_numpy(res)


class DenseAggOracleBackend(BlockOracleBackend):
    name = "dense-aggregate-oracle"

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        return DenseAggOraclePlan(sizes, ratio, bits, clients)
