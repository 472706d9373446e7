"""The model of block-wise quantisation with error feedback in one pass — a helper, not a test.

No arithmetic of its own: one round is tests/ef_model.py's accumulate, tests/blockwise_model.py's encode of the
accumulated update, and ef_model's commit over the split table (every 4096-element block a segment with k = n, every
position a kept entry), so xhat is the oracle's dequantize with the block's own range. BlockEFOracleBackend puts that
behind the plan interface (encode_block_ef) and declares the capability, so the codec and the client mixin run it on
the CPU.
"""
import numpy as np
import torch

from tests import blockwise_model as BM
from tests import ef_model as EF
from tests.blockwise_model import BlockOraclePlan
from tests.ef_model import EFOraclePlan
from tests.oracle_backend import OracleBackend

F32 = np.float32


def _implied_idx(bsegs):
    total = int((bsegs[:, 3] + bsegs[:, 2]).max()) if len(bsegs) else 0
    idx = np.zeros(total, dtype=np.int32)
    for _, n, _, oo in bsegs.tolist():
        idx[oo:oo + n] = np.arange(n, dtype=np.int32)
    return idx


def block_ef_round(x, r, segs, bits, base=None):
    """One round -> (bmn fp32[U], bscale fp32[U], codes uint8, stream uint32[P], the new residual). r is not changed."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    a = EF.accumulate(x, r, segs, base)
    bmn, bsc, codes, stream = BM.encode(a, segs, bits)
    bsegs = BM.split_table(segs)
    r1 = EF.commit(a, _implied_idx(bsegs), codes, bmn, bsc, bsegs, bits)
    return bmn, bsc, codes, stream, r1


def three_step(x, r, segs, bits, base=None):
    """The same round as the existing entry points compose it: accumulate; the block-wise encode of the residual
    without a base; residual -= the block-wise decode of that payload without a base (+0.0 where not finite)."""
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 4)
    span = len(r)
    a = EF.accumulate(x, r, segs, base)
    bmn, bsc, codes, stream = BM.encode(a, segs, bits)
    d = BM.decode(stream, bmn, bsc, segs, bits, span)
    r1 = a.copy()
    with np.errstate(all="ignore"):
        for off, n, _, _ in segs.tolist():
            v = a[off:off + n] - d[off:off + n]
            v[~np.isfinite(v)] = F32(0.0)
            r1[off:off + n] = v
    return bmn, bsc, codes, stream, r1


class BlockEFOraclePlan(BlockOraclePlan, EFOraclePlan):
    def encode_block_ef(self, residual, flat=None, tensors=None, base=None, **_):
        if (flat is None) == (tensors is None):
            raise ValueError("encode_block_ef: give exactly one of flat and tensors")
        segs = self.table.segs.astype(np.int64)
        if tensors is not None:
            x = np.zeros(self.table.span, dtype=np.float32)
            for (off, n, _, _), t in zip(segs.tolist(), tensors):
                x[off:off + n] = t.detach().cpu().numpy().reshape(-1)
        else:
            x = flat.detach().cpu().numpy()
        b = None if base is None else base.detach().cpu().numpy()
        mn, sc, _, stream, r1 = block_ef_round(x, residual.numpy(), segs, self.bits, base=b)
        residual.copy_(torch.from_numpy(r1))
        return torch.from_numpy(mn), torch.from_numpy(sc), torch.from_numpy(stream)


class BlockEFOracleBackend(OracleBackend):
    name = "block-ef-oracle"
    block_error_feedback = True  # (what the client mixin asks a backend before it combines the two switches)

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        return BlockEFOraclePlan(sizes, ratio, bits, clients)
