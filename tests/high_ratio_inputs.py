"""Inputs of the high-ratio / explicit-k tests (tests/test_gpu_high_ratio.py on the GPU, tests/test_high_ratio_cpu.py
for the expected values alone). Test infrastructure only.

The small layout, about 1.4 M elements (a latency-bound plan): 1025 is the smallest large segment (sampler m = 1024,
as 4097, 4096 * 3 + 5 and 50000 have), ragged tails with n % 4 in {1, 0}; 4096 * 40 samples m = 5120 keys and 2^20 the
m = 8192 cap; two small segments sit behind the large ones, so a slot that is reserved but never written would spill
into them.
"""
import functools

import numpy as np

from coala_amd.compression.spec import ALIGN, align_up, k_for

SIZES = [1025, 4097, 4096 * 3 + 5, 50000, 4096 * 40, 1 << 20, 700, 1]
LARGE = [i for i, n in enumerate(SIZES) if n > 1024]
KINDS = ("gauss", "zeros30", "grid", "equal", "special")
PAD = 4096 * 8200  # one more segment of this size makes a batch plan (> 8192 units)

F32 = np.float32


def _gauss(rng, n):
    return (rng.standard_normal(n) * 10 ** rng.uniform(-4, -2)).astype(F32)


def _signed_zeros(rng, n):
    return np.where(rng.random(n) < 0.5, F32(0.0), F32(-0.0)).astype(F32)


def segment(rng, kind, n):
    """One segment of n elements:
      "gauss"    plain Gaussian, no zeros
      "zeros30"  Gaussian with 30 % of the positions +-0 (mixed signs): from ratio ~0.7 on the k-th key is a zero and
                 the quota over the zeros, in index order, decides
      "grid"     round(g * 4) / 4: heavy nonzero ties on every level (and ~10 % zeros)
      "equal"    every |x| equal, random sign
      "special"  Gaussian with NaN (both signs), +-inf and denormals in the first, a middle and the last 4096-element unit
      "one"      all +-0 but one element (tie quota k - 1 of n - 1 zeros, or none at k = 1)"""
    g = _gauss(rng, n)
    if kind == "gauss":
        return g
    if kind == "zeros30":
        z = rng.random(n) < 0.3
        g[z] = _signed_zeros(rng, n)[z]
        return g
    if kind == "grid":
        return (np.round(rng.standard_normal(n) * 4) / 4).astype(F32)
    if kind == "equal":
        return np.where(rng.random(n) < 0.5, F32(-1e-3), F32(1e-3)).astype(F32)
    if kind == "special":
        nu = (n + 4095) // 4096
        sp = np.array([np.nan, -np.nan, np.nan, np.inf, -np.inf, 1e-40, -1e-41, 1e-45], F32)
        sp[1] = np.array([0xFFC00000], np.uint32).view(F32)[0]  # a NaN with the sign bit set
        for u in sorted({0, nu // 2, nu - 1}):
            lo, hi = u * 4096, min(n, u * 4096 + 4096)
            m = min(sp.size, hi - lo)
            g[lo + rng.choice(hi - lo, m, replace=False)] = sp[:m]
        return g
    if kind == "one":
        x = _signed_zeros(rng, n)
        x[int(rng.integers(0, n))] = F32(-0.5)
        return x
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def layout(kind, seed=0, sizes=tuple(SIZES)):
    """The small layout's segments of one kind (cached: the tests share them and leave them unchanged)."""
    rng = np.random.default_rng([seed, KINDS.index(kind) if kind in KINDS else 99])
    xs = [segment(rng, kind, n) for n in sizes]
    for x in xs:
        x.setflags(write=False)
    return xs


@functools.lru_cache(maxsize=None)
def base_layout(seed=0, sizes=tuple(SIZES)):
    rng = np.random.default_rng([seed, 1234])
    xs = [(rng.standard_normal(n) * 10 ** rng.uniform(-2, -1)).astype(F32) for n in sizes]
    for x in xs:
        x.setflags(write=False)
    return xs


def with_base(ds, bases):
    """Delta-mode inputs x = base + d and the fp32 deltas x - base the codec then sees (d's zeros stay exact zeros:
    base + +-0 = base)."""
    xs = [(b + d).astype(F32) for b, d in zip(bases, ds)]
    with np.errstate(all="ignore"):
        return xs, [(x - b).astype(F32) for x, b in zip(xs, bases)]


def explicit_rows(sizes, ks):
    """coalac_seg_t rows (in_off, n, k, out_off): 32-aligned in_off, contiguous out_off (a SegmentTable's layout with
    per-segment k)."""
    rows, off, oo = [], 0, 0
    for n, k in zip(sizes, ks):
        rows.append((off, n, k, oo))
        off = align_up(off + n, ALIGN)
        oo += k
    return np.array(rows, dtype=np.uint64)


def extreme_ks(order=0):
    """k per segment of the small layout: the large segments get, in order, 1, 2, n - 1, n, n // 2 + 1 and
    k_for(n, 0.001) (order 1: that list reversed, so the 2^20-element segment keeps one element and the 1025-element
    one k_for(n, 0.001) = 2); the small ones k = n and k = 1."""
    pick = [lambda n: 1, lambda n: 2, lambda n: n - 1, lambda n: n, lambda n: n // 2 + 1, lambda n: k_for(n, 0.001)]
    if order:
        pick = pick[::-1]
    ks = [0] * len(SIZES)
    for f, i in zip(pick, LARGE):
        ks[i] = f(SIZES[i])
    ks[6], ks[7] = SIZES[6], 1
    return ks


MIXED_RATIOS = (0.001, 0.9, 0.01, 0.999, 0.3, 0.6)  # of the large segments, in order (rmax > 0.475)


def mixed_ks():
    ks = [0] * len(SIZES)
    for r, i in zip(MIXED_RATIOS, LARGE):
        ks[i] = k_for(SIZES[i], r)
    ks[6], ks[7] = k_for(SIZES[6], 0.5), 1
    return ks
