"""Test-side restatement of the encode's route decision for one large segment (coala_amd/csrc/coalac.hip: k_scan's
per-unit counts, `Band`, `segment_pick` and `group_window` in k_gwin, `select_from_groups` and the first lines of
`select_fallback` in k_select), in integer arithmetic on uint32 keys as the kernel does. The bracket comes from
tests/sampler_model.py. Test infrastructure only: it says WHICH route a segment takes and with which counts, so that a
hand-built case can be shown to reach the code it claims; what the route must produce is oracle/codec_oracle.py's
business, never this file's.

Routes (the kernel's code in brackets):
  window           sa < k <= sc, the k-th key's band bin picked, every group hands over <= GCAP in-window entries and the
                   segment's list holds <= WLIST (select_from_groups -> window_resolve)
  window_gcap      ... but one group counted more than GCAP in-window entries (select_from_groups returns false:
                   select_generic from scratch, no fallback)
  window_wlist     ... every group within GCAP but the segment's list longer than WLIST (the same)
  generic_rank0    sa == k: segment_pick wants sa < k, select_fallback accepts sa <= k (select_generic, rank 0: T = T_hi)
  generic_forced   more than UCAP units, or COALAC_FLAG_GENERIC_SELECT (select_generic)
  tie_shortcut     tie mode and sc < k <= sc + sz (segment_pick's path 2: zero_tie_ranks, no select at all)
  raw_miss_high    sa > k            } select_fallback's raw-data path: the fallback counter counts these
  raw_miss_low     k > sc (in tie mode: k > sc + sz, or the shortcut skipped by a forced generic select)
  raw_ccap         a unit found more candidates than its ccap record slots
  raw_forced       COALAC_FLAG_FORCE_EXACT
"""
from dataclasses import dataclass, field

import numpy as np

from tests.sampler_model import KEY_MAX, SAMPLE_MAX, TIE_FLAG, _band_shift, _hash32, bracket, takes_raw_path

UNIT = 4096
GU = 32        # units per select group
HB2 = 512      # bins of the band histogram
GCAP = 256     # in-window entries a group may hand over
WLIST = 1024   # in-window entries the window route can hold
UCAP = 2048    # units per k_select chunk
SELECT_SPEC = 64
FLAG_FORCE_EXACT = 1   # COALAC_FLAG_FORCE_EXACT
FLAG_GENERIC_SELECT = 2  # COALAC_FLAG_GENERIC_SELECT
NT = {"latency": dict(gwin=512, select=512), "batch": dict(gwin=256, select=256)}  # block sizes per plan class
RAW_ROUTES = ("raw_miss_high", "raw_miss_low", "raw_ccap", "raw_forced")
ROUTES = ("window", "window_gcap", "window_wlist", "generic_rank0", "generic_forced", "tie_shortcut") + RAW_ROUTES


def sample_positions(n, seg_index):
    """The element positions the sampler reads (sampler_model.sample_keys): they depend on n and the segment's row only."""
    R = max(64, min(SAMPLE_MAX // 16, n // 512)) & ~63
    stride = n // R
    room = stride - 16
    pos = np.empty((R, 16), np.int64)
    for run in range(R):
        h = _hash32(((run * 0x9E3779B9) & 0xFFFFFFFF) ^ (((seg_index + 1) * 0x85EBCA6B) & 0xFFFFFFFF))
        pos[run] = ((run * stride + h % (room + 1)) & ~3) + np.arange(16)
    return pos.ravel()


def per_unit(mask_or_counts, n):
    return np.add.reduceat(mask_or_counts.astype(np.int64), np.arange(0, n, UNIT))


@dataclass
class Band:
    """coalac.hip `struct Band`: bins of 2^shift keys over [tlo, hhi]; keys in (hhi, thi] clamped into the last bin."""
    tlo: int
    thi: int
    hhi: int
    shift: int = field(init=False)
    last: int = field(init=False)

    def __post_init__(self):
        self.shift = _band_shift(self.tlo, self.hhi, 9)
        self.last = ((self.hhi - self.tlo) & 0xFFFFFFFF) >> self.shift

    def bin(self, keys):
        keys = np.asarray(keys, np.int64)
        return np.where(keys > self.hhi, self.last, (keys - self.tlo) >> self.shift)

    def wlo(self, b):
        return self.tlo + (b << self.shift)

    def whi(self, b):
        return self.thi if b == self.last else min(self.thi, self.wlo(b) + (1 << self.shift) - 1)


@dataclass
class Route:
    route: str
    tlo: int            # as the kernel stores it (TIE_FLAG included)
    thi: int
    outcome: str        # the sampler's (sampler_model.bracket)
    tie: bool           # tie mode: T_lo == 0 or flagged
    shhi: int
    cntA: np.ndarray    # per unit: keys above T_hi
    cntC: np.ndarray    # per unit: candidates (keys >= T_lo; tie mode: keys above K)
    cntZ: np.ndarray    # per unit: keys equal to K (tie mode; zeros otherwise)
    sa: int
    sc: int
    sz: int
    band: Band
    hist: np.ndarray = None   # the summed HB2-bin band histogram
    bin: int = None           # the picked bin
    wlo: int = None
    whi: int = None
    rank: int = None          # rank inside the window; tie_shortcut: the tie quota k - sc
    gcnt: np.ndarray = None   # per group: in-window entries
    W: int = None

    @property
    def raw(self):
        return self.route in RAW_ROUTES


def hist_pick(hist, r):
    """coalac.hip hist_pick: (bin of the r-th largest key, rank inside it), or (None, r) when the bins hold fewer."""
    above = 0
    for bb in range(len(hist) - 1, -1, -1):
        if above + hist[bb] >= r:
            return bb, r - above
        above += int(hist[bb])
    return None, r


def band_hist(x, R, groups=None):
    """The band histogram summed over the given groups only (default: all) — what segment_pick would sum if one of its
    two loops over the group histograms left groups out."""
    keys = (x.view(np.uint32) & np.uint32(KEY_MAX)).astype(np.int64)
    K = R.tlo & KEY_MAX
    inband = (keys > K if R.tie else keys >= K) & (keys <= R.thi)
    if groups is not None:
        g = np.arange(x.size) // (GU * UNIT)
        inband &= np.isin(g, np.asarray(list(groups)))
    return np.bincount(R.band.bin(keys[inband]), minlength=HB2)


def loop_boundaries(plan_class):
    """The unit counts at which a block loop of the select chain starts another round in this plan class: one group
    (GU), segment_pick's and select_from_groups' CB * NT unit counts, the GB * GU units of 24 group histograms,
    select_finish's and zero_tie_ranks' NT-unit chunks, UCAP."""
    nt = NT[plan_class]
    return sorted({GU, 3 * nt["gwin"], 3 * nt["select"], 24 * GU, nt["select"], UCAP})


def route_of(x, k, seg_index, ccap, flags=0):
    """The route of large segment x (float32, the values the codec sees) keeping k, at row seg_index of a plan with ccap
    record slots per unit (the decision is the same in both plan classes: they differ in block sizes only)."""
    n = x.size
    nu = (n + UNIT - 1) // UNIT
    keys = (x.view(np.uint32) & np.uint32(KEY_MAX)).astype(np.int64)
    tlo_raw, thi, outcome = bracket(x, k, seg_index)
    tie = tlo_raw == 0 or bool(tlo_raw & TIE_FLAG)
    K = tlo_raw & KEY_MAX
    shhi = min(thi, int(keys[sample_positions(n, seg_index)].max()))
    cand = keys > K if tie else keys >= K
    cntC = per_unit(cand, n)
    cntA = per_unit(cand & (keys > thi), n)
    cntZ = per_unit(keys == K, n) if tie else np.zeros(nu, np.int64)
    sa, sc, sz = int(cntA.sum()), int(cntC.sum()), int(cntZ.sum())
    band = Band(K, thi, shhi)
    R = Route("", tlo_raw, thi, outcome, tie, shhi, cntA, cntC, cntZ, sa, sc, sz, band)
    ov = bool((cntC > ccap).any())

    def fallback():  # select_fallback's first lines
        if flags & FLAG_FORCE_EXACT:
            return "raw_forced"
        if ov:
            return "raw_ccap"
        if sa > k:
            return "raw_miss_high"
        if k > sc:
            return "raw_miss_low"
        if (flags & FLAG_GENERIC_SELECT) or nu > UCAP:
            return "generic_forced"
        assert sa == k, "a segment with sa < k <= sc that is not forced takes the window"
        return "generic_rank0"

    forced = bool(flags & (FLAG_FORCE_EXACT | FLAG_GENERIC_SELECT)) or nu > UCAP or ov
    if not forced and tie and sc < k and k - sc <= sz:
        R.route, R.rank = "tie_shortcut", k - sc
        return R
    if forced or not (sa < k <= sc):
        R.route = fallback()
        return R
    # the stored records in the band [K, thi] (no unit overflowed here, so every candidate is stored)
    inband = cand & (keys >= K) & (keys <= thi)
    R.hist = np.bincount(band.bin(keys[inband]), minlength=HB2)
    assert R.hist.size == HB2, "a band key fell outside the HB2 bins"
    b, r = hist_pick(R.hist, k - sa)
    assert b is not None, "hist_pick found no bin although sa < k <= sc"  # (pinned: tests/test_select_model_cpu.py)
    R.bin, R.wlo, R.whi, R.rank = b, band.wlo(b), band.whi(b), r
    inwin = cand & (keys >= R.wlo) & (keys <= R.whi)
    R.gcnt = np.add.reduceat(per_unit(inwin, n), np.arange(0, nu, GU))
    R.W = int(R.gcnt.sum())
    if (R.gcnt > GCAP).any():
        R.route = "window_gcap"
    elif R.W > WLIST:
        R.route = "window_wlist"
    else:
        R.route = "window"
    return R


def agrees_with_sampler_model(x, k, R, ccap, flags=0):
    """The raw half of the decision restated independently in sampler_model.takes_raw_path (which knows nothing of
    COALAC_FLAG_FORCE_EXACT)."""
    if flags & FLAG_FORCE_EXACT:
        return R.route == "raw_forced"
    return R.raw == takes_raw_path(x, k, R.tlo, R.thi, ccap, generic=bool(flags & FLAG_GENERIC_SELECT))
