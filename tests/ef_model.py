"""CPU restatement of the upload codec's error feedback — TEST INFRASTRUCTURE ONLY.

numpy fp32, elementwise, on top of oracle.codec_oracle for the encode and the dequantise arithmetic. Per client,
with a persistent residual r (fp32, the plan's flat input layout, zero at the start), one round is

  accumulate  a[i] = (x[i] - base[i]) + r[i] inside every segment (fp32 subtract, then fp32 add; no base:
              x[i] + r[i]); the padding between segments is not touched
  encode      the codec's ordinary payload of `a`
  commit      r[pos] = a[pos] - xhat at every kept entry, xhat = what the decoder writes there
              (mn + float(q) * scale, or the stored fp32 value at bits 32); +0.0 where that is NaN or +-Inf;
              every other position keeps a

Also: an oracle-backed plan with ef_accumulate / ef_commit, so the codec and the hook mixins run error feedback
without a GPU (tests/oracle_backend.py is the plain one).
"""
import numpy as np
import torch

from oracle import codec_oracle as O
from tests.oracle_backend import OracleBackend, OraclePlan

F32 = np.float32


def _segs(segs):
    return np.asarray(segs, dtype=np.int64).reshape(-1, 4)


def accumulate(x, r, segs, base=None):
    """The accumulated update: a copy of r with (x - base) + r inside every segment."""
    a = np.array(r, dtype=F32, copy=True)
    with np.errstate(all="ignore"):
        for off, n, _, _ in _segs(segs):
            d = x[off:off + n].astype(F32, copy=False)
            if base is not None:
                d = d - base[off:off + n]
            a[off:off + n] = d + r[off:off + n]
    return a


def commit(a, idx, vals, mn, scale, segs, bits):
    """The new residual: a copy of a with a[pos] - xhat (non-finite: +0.0) at every kept entry."""
    r = np.array(a, dtype=F32, copy=True)
    with np.errstate(all="ignore"):
        for s, (off, n, k, oo) in enumerate(_segs(segs)):
            pos = off + idx[oo:oo + k].astype(np.int64)
            v = vals[oo:oo + k]
            xhat = v.astype(F32) if bits == O.RAW_BITS else O.dequantize(v, mn[s], scale[s])
            d = a[pos] - xhat
            d[~np.isfinite(d)] = F32(0.0)
            r[pos] = d
    return r


def ef_round(x, r, segs, bits, base=None):
    """One round: ((idx, vals, mn, scale) of the payload, the new residual)."""
    a = accumulate(x, r, segs, base)
    enc = O.encode(a, _segs(segs), bits)
    return enc, commit(a, *enc, segs, bits)


class EFOraclePlan(OraclePlan):
    """OraclePlan + the error-feedback pair, in place on CPU tensors, as CodecPlan has them."""

    def ef_accumulate(self, resid, flat=None, tensors=None, base=None, **_):
        if (flat is None) == (tensors is None):
            raise ValueError("ef_accumulate: give exactly one of flat and tensors")
        segs = _segs(self.table.segs)
        if flat is None:
            flat = torch.zeros(self.table.span)
            for (off, n, _, _), t in zip(segs, tensors):
                flat[off:off + n] = t.detach().reshape(-1)
        b = None if base is None else base.detach().numpy()
        resid.copy_(torch.from_numpy(accumulate(flat.detach().numpy(), resid.numpy(), segs, b)))
        return resid

    def ef_commit(self, enc, resid, **_):
        r = commit(resid.numpy(), self._idx(enc), enc.vals.numpy(), enc.mn.numpy(), enc.scale.numpy(),
                   _segs(self.table.segs), self.bits)
        resid.copy_(torch.from_numpy(r))
        return resid


class EFOracleBackend(OracleBackend):
    name = "oracle-ef"

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        return EFOraclePlan(sizes, ratio, bits, clients)


def bits_of(a):
    """uint32 view of an fp32 array or tensor (every comparison of the error-feedback tests is bit-exact)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)
