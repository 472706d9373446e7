"""Hand-built large segments for the encode's select chain (k_ghist -> k_gwin -> k_select in coala_amd/csrc/coalac.hip):
one case per route of tests/select_model.py and per loop boundary, each with its own k and the claim it is built for.

How a case is built. The sampler reads R runs of 16 elements whose positions depend only on the segment's size and row
(select_model.sample_positions), and the bracket {T_lo, T_hi} depends only on the keys found there. So a case first
writes the sampled positions (distinct random keys, or in tie mode the tie key K everywhere), computes the bracket, and
then writes every OTHER position itself: keys below T_lo by default (0x20000000 + position: distinct, never candidates),
and on top of them, entry by entry, the keys above T_hi, the band keys above the window, the in-window entries and the
ties, in the units it chooses. The bracket cannot move, and sa, sc, the band histogram, each group's in-window count and
the tie ranks are what the case put there plus what the sampled keys contribute (counted here directly, not through the
model). tests/test_select_model_cpu.py checks every claim against the model.

Sizes. Every route at 40 units; the window, generic_rank0, tie_shortcut and tie-quota cases also at 32, 33, 768, 769,
1536, 1537, 2048 and 2049 units (last unit TAIL elements, TAIL % 4 == 1), with the entries placed from the boundary
unit on (Case.boundary): the first unit of the last group / CB * NT block / UCAP chunk the size reaches.

window_hist_tail_1500 (47 groups) is the case for segment_pick's `g >= GB` histogram tail: see window_case.

Two limits of the sampler decide what can be built where (pinned in test_select_model_cpu.py):
  * T_hi is closed only if floor(p m - 6 sqrt(p m) - 8) >= 1 (m sampled keys, p = k / n): at 32, 33 and 40 units
    (m <= 5120) that needs p >= 0.0128, so sa > 0 — generic_rank0, raw_miss_high — exists there only in plans whose rmax
    is 0.05 (Case.min_rmax).
  * One unit holds at most ccap candidates, so where a single (partial) unit lies beyond the boundary — 33, 769, 1537,
    2049 units — a case that keeps half its entries there has k <= ~1000, its T_hi is open and sa = 0. generic_rank0
    at 769 and 1537 units therefore fills the last unit and keeps the rest from the previous boundary on.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

from tests import select_model as M
from tests.sampler_model import KEY_MAX, TIE_FLAG, bracket, ccap_for

F32 = np.float32
UNIT = 4096
TAIL = 3001                      # elements of every case's last unit
SMALL_N, SMALL_K = 512, 37       # the small segment after every case
LOW = 0x20000000                 # keys of the filler elements: LOW + position
KEY_LO, KEY_HI = 0x30000000, 0x3F000000  # range of the sampled keys
K_TIE = 0x3A83126F               # tie key of the tie-mode cases (0.001f)
RMAX = (0.01, 0.05)
CCAP = {r: ccap_for([r]) for r in RMAX}   # 576, 896
ROOM = CCAP[0.01] - 16           # candidates a case puts into one unit at most (within every plan's ccap)
BOUNDARY_SIZES = (32, 33, 768, 769, 1536, 1537, 2048, 2049)
BOUNDARY_OF = {32: 0, 33: 32, 40: 0, 768: 512, 769: 768, 1536: 768, 1537: 1536, 2048: 1536, 2049: 2048}


def n_of(nu):
    return (nu - 1) * UNIT + TAIL


@dataclass
class Case:
    name: str
    x: np.ndarray            # the values the codec sees
    k: int
    row: int                 # the segment's row in its plan (the sampler hashes it)
    route: str               # the claim
    counts: dict             # ... and the counts that make it non-vacuous (fields of select_model.Route, or `kth_*`)
    boundary: int = 0        # first unit "beyond the boundary"
    min_rmax: float = 0.01   # smallest plan rmax the case's k allows
    only_rmax: float = None  # built against one plan's ccap
    ties: np.ndarray = None  # positions of the elements equal to the k-th key
    bracket0: tuple = None   # the bracket before the edits
    flags: int = 0

    @property
    def nu(self):
        return (self.x.size + UNIT - 1) // UNIT


class Skeleton:
    """A segment with its sampled positions written and its bracket fixed; everything else is LOW + position until put."""

    def __init__(self, nu, k, row, seed, tie_key=None):
        self.nu, self.n, self.k, self.row = nu, n_of(nu), k, row
        self.rng = np.random.default_rng(seed)
        n = self.n
        self.keys = (LOW + np.arange(n, dtype=np.int64)).astype(np.uint32)
        self.neg = self.rng.random(n) < 0.5
        self.spos = M.sample_positions(n, row)
        if tie_key is None:
            m = self.spos.size
            step = (KEY_HI - KEY_LO) // m
            sk = KEY_LO + np.arange(m, dtype=np.int64) * step + self.rng.integers(0, step, m)
            self.keys[self.spos] = self.rng.permutation(sk).astype(np.uint32)
        else:
            self.keys[self.spos] = tie_key
            if tie_key == 0:
                self.keys[:] = 0
        self.tlo, self.thi, self.outcome = bracket(self.values(), k, row)
        self.bracket0 = (self.tlo, self.thi, self.outcome)
        self.K = self.tlo & KEY_MAX
        self.tie = self.tlo == 0 or bool(self.tlo & TIE_FLAG)
        self.skeys = self.keys[self.spos].astype(np.int64)
        self.band = M.Band(self.K, self.thi, min(self.thi, int(self.skeys.max())))
        self.sampled = np.zeros(n, bool)
        self.sampled[self.spos] = True
        self._free = {}
        lo = self.K + 1 if self.tie else self.K
        self.ncand = np.bincount(self.spos[self.skeys >= lo] // UNIT, minlength=nu)  # candidates per unit so far

    def free(self, u):
        """[positions, next]: the unit's positions the sampler does not read, ascending, and how many are used."""
        if u not in self._free:
            lo, hi = u * UNIT, min(self.n, u * UNIT + UNIT)
            self._free[u] = [np.flatnonzero(~self.sampled[lo:hi]) + lo, 0]
        return self._free[u]

    def take(self, u, c):
        f = self.free(u)
        assert f[1] + c <= f[0].size, (u, c)
        pos = f[0][f[1]:f[1] + c]
        f[1] += c
        return pos

    def left(self, u):
        f = self.free(u)
        return f[0].size - f[1]

    def values(self):
        return (self.keys | (self.neg.astype(np.uint32) << np.uint32(31))).view(F32)

    def sampled_above(self, key):
        return int((self.skeys > key).sum())

    def put(self, unit, keys, neg=None, candidate=True):
        """Write keys to the unit's next free positions (ascending index, in call order); returns the positions."""
        keys = np.atleast_1d(np.asarray(keys, np.int64))
        pos = self.take(unit, keys.size)
        self.keys[pos] = keys.astype(np.uint32)
        if neg is not None:
            self.neg[pos] = neg
        if candidate:
            self.ncand[unit] += keys.size
            assert self.ncand[unit] <= ROOM + 16, (unit, self.ncand[unit])
        return pos

    def spread(self, keys, units, neg=None):
        """Write keys over the units in order, each filled up to ROOM candidates before the next is touched."""
        keys = np.asarray(keys, np.int64)
        done = 0
        for u in units:
            if done == keys.size:
                break
            c = int(min(keys.size - done, max(0, ROOM - self.ncand[u]), self.left(u)))
            if c > 0:
                self.put(u, keys[done:done + c], neg)
                done += c
        assert done == keys.size, f"no room for {keys.size - done} of {keys.size} keys in the chosen units"

    def free_bin(self, want=0.5):
        """A band bin with no sampled key in it, not the first and not the last, near fraction `want` of the band."""
        used = set(self.band.bin(self.skeys[(self.skeys >= self.K) & (self.skeys <= self.thi)]).tolist())
        b0 = max(1, int(self.band.last * want))
        for b in list(range(b0, self.band.last)) + list(range(b0, 0, -1)):
            if b not in used:
                return b
        raise AssertionError("no free band bin")


def units_from(nu, boundary):
    """The units from the boundary on first, then the others downwards from it."""
    return list(range(boundary, nu)) + list(range(boundary - 1, -1, -1))


def k_for_size(nu, boundary, p=0.0099):
    """k at ratio p, but no more than 1.8 x what the units beyond the boundary can hold."""
    beyond = (nu - boundary) * (ROOM - 8)
    return int(min(p * n_of(nu), 1.8 * beyond))


def closed_thi(nu, k):
    n = n_of(nu)
    m = (max(64, min(512, n // 512)) & ~63) * 16
    se = k / n * m
    return math.floor(se - (6.0 * math.sqrt(se) + 8.0)) >= 1


# ---------------------------------------------------------------------------------------------------------------
# the window route and its neighbours
# ---------------------------------------------------------------------------------------------------------------
def window_case(name, nu, row, *, W=40, kth="mid", order="mid", wbin=0.5, sizes=None, k=None, p=0.0099, repeat=(),
                signs=None, extra=0, boundary=None, hist_tail=False):
    """An ordinary window. The window's bin holds exactly the W entries put here (W + its sampled keys for wbin 0 /
    "last"), keys wlo + 16 i; the k-th key is entry `kth` by value ("first": rank 1, "last": rank W, "mid") and sits at
    list position `order` ("first" / "last" / "mid": index order = list order). sizes: in-window entries per group
    {group: count} (default: all W in the boundary's group and after). repeat: units that get one more copy of the k-th
    key each (the tie quota), after the entry itself; signs: (sign of every kept value above the k-th key, [sign of
    each tie in index order])."""
    boundary = BOUNDARY_OF[nu] if boundary is None else boundary
    k = k_for_size(nu, boundary, p) if k is None else k
    S = Skeleton(nu, k, row, seed=1000 + nu + row)
    assert not S.tie and S.outcome == "none", S.bracket0
    band = S.band
    if wbin == "last":
        b = band.last
    elif wbin == 0:
        b = 0
    else:
        b = S.free_bin(wbin)
    wlo, whi = band.wlo(b), band.whi(b)
    inwin_s = S.skeys[(S.skeys >= wlo) & (S.skeys <= whi)]
    if wbin == "last":  # keys in (shhi, T_hi] are clamped into the last bin: put the entries there
        assert S.thi == KEY_MAX and band.hhi < S.thi
        ekeys = band.hhi + 1 + 16 * np.arange(1, W + 1, dtype=np.int64)
    else:
        step = max(1, (whi - wlo) // (W + 2))
        ekeys = wlo + step * np.arange(1, W + 1, dtype=np.int64)
        ekeys = ekeys[~np.isin(ekeys, inwin_s)][:W]
        W = ekeys.size
    assert ekeys.max() <= whi and ekeys.min() >= wlo
    # rank of the k-th key among the put entries (1 = largest), and that key
    rput = {"first": 1, "last": W, "mid": (W + 1) // 2}[kth]
    T = int(np.sort(ekeys)[::-1][rput - 1])
    rank = rput + int((inwin_s > T).sum())
    # which entry goes where: the units of the window entries, in index order
    hot = units_from(nu, boundary)
    given_sizes = None if sizes is None else dict(sizes)
    if sizes is None:
        sizes = {}
        left, u = W, boundary
        while left:  # at most 6 entries per unit from the boundary on
            g = u // M.GU
            c = min(left, 6)
            sizes.setdefault(g, []).append((u, c))
            left -= c
            u = u + 1 if u + 1 < nu else boundary
        plan = [uc for g in sorted(sizes) for uc in sizes[g]]
    else:  # {group: count}: spread over the group's units
        plan = []
        for g in sorted(sizes):
            us = list(range(g * M.GU, min(nu, g * M.GU + M.GU)))
            per = -(-sizes[g] // len(us))
            left = sizes[g]
            for u in us:
                c = min(left, per)
                if c:
                    plan.append((u, c))
                left -= c
        assert sum(c for _, c in plan) == W
    others = S.rng.permutation(ekeys[ekeys != T])
    pos_T = {"first": 0, "last": W - 1, "mid": W // 2}[order]
    seq = np.concatenate([others[:pos_T], [T], others[pos_T:]])
    above_neg = None if signs is None else signs[0]
    done, tie_pos = 0, []
    for u, c in plan:
        part = seq[done:done + c]
        pos = S.put(u, part, None)
        if above_neg is not None:
            S.neg[pos[part > T]] = above_neg
        tie_pos += list(pos[part == T])
        done += c
    for u in repeat:
        tie_pos += list(S.put(u, [T]))
    tie_pos = np.sort(np.array(tie_pos, np.int64))
    if signs is not None:
        S.neg[tie_pos] = signs[1]
        S.neg[S.spos[S.skeys > T]] = above_neg
    # the keys above the window: k - rank of them, sampled ones included; half above T_hi where it is closed
    need = k - rank - extra - S.sampled_above(whi)  # (extra: that many more of the ties are kept)
    assert need >= 0, need
    n_hi = need // 2 if S.thi != KEY_MAX else 0
    room_band = S.thi - whi if S.thi != KEY_MAX else band.hhi - whi
    assert need - n_hi == 0 or room_band > 0
    kb = whi + 1 + (np.arange(need - n_hi, dtype=np.int64) % max(1, room_band))
    ka = S.thi + 1 + np.arange(n_hi, dtype=np.int64)
    sa = n_hi + S.sampled_above(S.thi)
    if hist_tail:
        assert boundary == 24 * M.GU and S.thi != KEY_MAX
        ng = (nu + M.GU - 1) // M.GU
        late = list(range((ng - 1) * M.GU, nu))
        S.spread(kb[:kb.size // 3], late, above_neg)
        S.spread(np.concatenate([ka, kb[kb.size // 3:]]), list(range(boundary, (ng - 1) * M.GU)), above_neg)
        b2 = S.free_bin(0.2)
        assert 0 < b2 < b
        lo2, hi2 = band.wlo(b2), band.whi(b2)
        S.spread(lo2 + (np.arange(k - sa + 500, dtype=np.int64) % (hi2 - lo2 + 1)), list(range(boundary)))
    else:
        S.spread(np.concatenate([ka, kb]), hot, above_neg)
    x = S.values()
    counts = dict(sa=sa, rank=rank + extra, bin=b, kth_key=T)
    if wbin not in (0, "last"):
        counts["W"] = W + len(repeat)
    if given_sizes:
        gc = np.zeros((nu + M.GU - 1) // M.GU, np.int64)
        for g, c in given_sizes.items():
            gc[g] = c
        counts["gcnt"] = gc
    return Case(name, x, k, row, "window", counts, boundary, ties=tie_pos, bracket0=S.bracket0)


def overflow_case(name, nu, row, kind, groups):
    """window_gcap / window_wlist and their neighbours: `groups` = {group: in-window entries}; the k-th key is the
    smallest entry's neighbour in the middle, the entries of a group over GCAP are EQUAL keys just below it."""
    k = k_for_size(nu, 0)
    S = Skeleton(nu, k, row, seed=2000 + nu + row)
    assert not S.tie and S.outcome == "none"
    b = S.free_bin()
    wlo, whi = S.band.wlo(b), S.band.whi(b)
    W = sum(groups.values())
    T = wlo + 3 * ((whi - wlo) // 4)
    n_above = 20
    above = T + 16 * np.arange(1, n_above + 1, dtype=np.int64)
    assert above.max() <= whi
    first = True
    for g in sorted(groups):
        us = list(range(g * M.GU, min(nu, g * M.GU + M.GU)))
        c = groups[g]
        if first:  # the k-th key and the entries above it, in the first group named
            keys = np.concatenate([above, [T], np.full(c - n_above - 1, T - 8, np.int64)])
            first = False
        else:
            keys = np.full(c, T - 8, np.int64) if c > M.GCAP else T - 8 - 16 * np.arange(1, c + 1, dtype=np.int64)
        assert keys.min() >= wlo
        per = -(-c // len(us))
        for i, u in enumerate(us):
            part = keys[i * per:(i + 1) * per]
            if part.size:
                S.put(u, S.rng.permutation(part))
    rank = n_above + 1
    need = k - rank - S.sampled_above(whi)
    n_hi = need // 2 if S.thi != KEY_MAX else 0
    kb = whi + 1 + (np.arange(need - n_hi, dtype=np.int64) % (min(S.thi, S.band.hhi) - whi))
    S.spread(np.concatenate([S.thi + 1 + np.arange(n_hi, dtype=np.int64), kb]), units_from(nu, 0))
    gc = np.zeros((nu + M.GU - 1) // M.GU, np.int64)
    for g, c in groups.items():
        gc[g] = c
    return Case(name, S.values(), k, row, kind, dict(W=W, rank=rank, gcnt=gc, kth_key=T), bracket0=S.bracket0)


def sa_case(name, nu, row, delta, p, boundary=None):
    """sa == k + delta exactly: delta 0 generic_rank0, -1 window (the k-th key is the largest band key), +1
    raw_miss_high. Every key above T_hi that is not sampled is put here, from the boundary on."""
    boundary = BOUNDARY_OF[nu] if boundary is None else boundary
    k = int(p * n_of(nu))
    S = Skeleton(nu, k, row, seed=3000 + nu + row)
    assert not S.tie and S.thi != KEY_MAX, S.bracket0
    need = k + delta - S.sampled_above(S.thi)
    hot = [nu - 1] + [u for u in units_from(nu, boundary) if u != nu - 1]  # the last unit first
    S.spread(S.thi + 1 + np.arange(need, dtype=np.int64), hot)
    route = {0: "generic_rank0", -1: "window", 1: "raw_miss_high"}[delta]
    counts = dict(sa=k + delta)
    if delta == -1:
        counts["rank"] = 1
    return Case(name, S.values(), k, row, route, counts, boundary, min_rmax=0.01 if p <= 0.01 else 0.05,
                bracket0=S.bracket0)


def sc_case(name, nu, row, delta):
    """sc == k + delta: delta -1 raw_miss_low; 0 window, the k-th key is the smallest candidate (rank sc - sa)."""
    k = k_for_size(nu, 0)
    S = Skeleton(nu, k, row, seed=4000 + nu + row)
    assert not S.tie
    sampled_c = int((S.skeys >= S.K).sum())
    need = k + delta - sampled_c
    lo = int(S.skeys[S.skeys >= S.K].min())  # put everything above the smallest sampled candidate
    b = int(S.band.bin(lo))  # the lowest candidate's bin: sampled keys only
    S.spread(S.band.wlo(b + 1) + np.arange(need, dtype=np.int64) * 3, units_from(nu, 0))
    sa = int((S.keys.astype(np.int64) > S.thi).sum())
    if delta == -1:
        return Case(name, S.values(), k, row, "raw_miss_low", dict(sc=k - 1, sa=sa), bracket0=S.bracket0)
    return Case(name, S.values(), k, row, "window", dict(sc=k, sa=sa, bin=b, kth_key=lo), bracket0=S.bracket0)


def ccap_case(name, nu, row, ccap, over):
    """The segment's last unit holds ccap + over candidates (over 1: raw_ccap, 0: window), every other unit few."""
    k = k_for_size(nu, 0)
    S = Skeleton(nu, k, row, seed=5000 + nu + row + ccap)
    assert not S.tie and S.outcome == "none"
    b = S.free_bin()
    wlo, whi = S.band.wlo(b), S.band.whi(b)
    last = nu - 1
    fill = ccap + over - int(S.ncand[last])
    keys = whi + 1 + np.arange(fill, dtype=np.int64)
    pos = S.take(last, fill)  # (past ROOM on purpose)
    S.keys[pos] = keys.astype(np.uint32)
    S.ncand[last] += fill
    T = wlo + 64
    S.put(last - 1, [T])
    need = k - 1 - S.sampled_above(whi) - fill
    assert need >= 0
    S.spread(whi + 1 + np.arange(need, dtype=np.int64), list(range(last - 1, -1, -1)))
    cnt = np.zeros(nu, np.int64)
    cnt[last] = ccap + over
    return Case(name, S.values(), k, row, "raw_ccap" if over else "window",
                dict(cntC_last=ccap + over, kth_key=T), only_rmax={v: r for r, v in CCAP.items()}[ccap],
                bracket0=S.bracket0)


# ---------------------------------------------------------------------------------------------------------------
# tie mode
# ---------------------------------------------------------------------------------------------------------------
def tie_case(name, nu, row, *, K=K_TIE, sc=None, sz=60, dk=None, rt=None, signs=None, tie_units=None, boundary=None):
    """Tie mode (every sampled key is K): sc keys above K and (K > 0) sz ties put from the boundary on, k = sc + rt
    (or dk: k = sc + dk relative to the edges). signs: "kept" / "dropped": every key above K positive, every tie
    positive except the tie of rank rt - 1 ("kept": mn = -K) or rt ("dropped": mn > 0), all later ties negative too."""
    boundary = BOUNDARY_OF[nu] if boundary is None else boundary
    n = n_of(nu)
    nsamp = M.sample_positions(n, row).size
    sz_all = n - (sc or 0) if K == 0 else sz + nsamp
    if dk is not None:
        rt = {"sc": 0, "sc+1": 1, "sc+sz": sz_all, "sc+sz+1": sz_all + 1}[dk]
    elif rt is None:  # the quota ends 5 ties before the last one, if a ratio allows that many kept ties
        rt = sz_all - 5
        if rt + 200 > int(0.0099 * n) and boundary == 0:
            rt = int(0.0099 * n) - 600
    budget = int((0.0099 if rt + 200 <= int(0.0099 * n) else 0.049) * n)
    if sc is None:
        sc = min(k_for_size(nu, boundary), budget - rt)
    assert sc > 0 and sc + rt <= 0.05 * n
    k = sc + rt
    S = Skeleton(nu, k, row, seed=6000 + nu + row, tie_key=K)
    assert S.tie and S.K == K, S.bracket0
    hot = units_from(nu, boundary)
    pos_neg = False if signs else None
    S.spread(K + 1 + 5 * np.arange(sc, dtype=np.int64), hot, pos_neg)
    tie_pos = S.spos.copy()
    if K != 0:
        tu = list(range(boundary, nu))[:8] if tie_units is None else tie_units
        per = -(-sz // min(len(tu), 8))
        left = sz
        for u in tu:
            c = min(left, per)
            if c:
                tie_pos = np.concatenate([tie_pos, S.put(u, np.full(c, K), candidate=False)])
            left -= c
        assert left == 0
        tie_pos = np.sort(tie_pos)
        if signs:
            j = rt - 1 if signs == "kept" else rt
            S.neg[tie_pos[:j]] = False
            S.neg[tie_pos[j:]] = True
    else:
        tie_pos = np.flatnonzero(S.keys == 0)
    if nu > M.UCAP:
        route = "generic_forced" if rt == 0 else "raw_miss_low"
    elif rt == 0:
        route = "generic_rank0" if S.thi == K and K != 0 else "window"
    elif rt <= sz_all:
        route = "tie_shortcut"
    else:
        route = "raw_miss_low"
    counts = dict(sc=sc, sz=sz_all)
    if route == "tie_shortcut":
        counts["rank"] = rt
    c = Case(name, S.values(), k, row, route, counts, boundary, min_rmax=0.01 if k <= 0.01 * n else 0.05, ties=tie_pos,
             bracket0=S.bracket0)
    c.kept_tie_units = None if K == 0 or rt == 0 else (int(tie_pos[0]) // UNIT, int(tie_pos[min(rt, tie_pos.size) - 1]) // UNIT)
    return c


# ---------------------------------------------------------------------------------------------------------------
# the case list: builders by name, rows assigned by the plan parts
# ---------------------------------------------------------------------------------------------------------------
def _builders():
    B = {}

    def add(name, nu, fn, **kw):
        B[name] = (nu, functools.partial(fn, name, nu, **kw))

    # every route at 40 units
    add("window_first_in_list", 40, lambda nm, nu, row: window_case(nm, nu, row, order="first"))
    add("window_last_in_list", 40, lambda nm, nu, row: window_case(nm, nu, row, order="last"))
    add("window_rank_1", 40, lambda nm, nu, row: window_case(nm, nu, row, kth="first"))
    add("window_rank_W", 40, lambda nm, nu, row: window_case(nm, nu, row, kth="last"))
    add("window_bin_0", 40, lambda nm, nu, row: window_case(nm, nu, row, wbin=0))
    add("window_bin_last_clamped", 40, lambda nm, nu, row: window_case(nm, nu, row, wbin="last", k=20))
    add("window_list_65_256", 40, lambda nm, nu, row: window_case(nm, nu, row, W=65 + 256, sizes={0: 65, 1: 256}))
    add("gcap_257", 40, lambda nm, nu, row: overflow_case(nm, nu, row, "window_gcap", {0: 257, 1: 60}))
    add("gcap_257_last_group", 40, lambda nm, nu, row: overflow_case(nm, nu, row, "window_gcap", {0: 60, 1: 257}))
    add("wlist_1025", 200, lambda nm, nu, row: overflow_case(nm, nu, row, "window_wlist",
                                                             {0: 256, 1: 256, 2: 256, 3: 200, 4: 57}))
    add("wlist_1024", 200, lambda nm, nu, row: overflow_case(nm, nu, row, "window",
                                                             {0: 256, 1: 256, 2: 256, 3: 200, 4: 56}))
    for d, nm in ((0, "rank0_sa_eq_k"), (-1, "rank0_sa_eq_k_minus_1"), (1, "miss_high_sa_eq_k_plus_1")):
        add(nm, 40, lambda nm, nu, row, d=d: sa_case(nm, nu, row, d, 0.03))
    add("miss_low_sc_eq_k_minus_1", 40, lambda nm, nu, row: sc_case(nm, nu, row, -1))
    add("window_sc_eq_k", 40, lambda nm, nu, row: sc_case(nm, nu, row, 0))
    for r in RMAX:
        add(f"ccap_plus_1_rmax{r}", 40, lambda nm, nu, row, r=r: ccap_case(nm, nu, row, CCAP[r], 1))
        add(f"ccap_exact_rmax{r}", 40, lambda nm, nu, row, r=r: ccap_case(nm, nu, row, CCAP[r], 0))
    for dk in ("sc", "sc+1", "sc+sz", "sc+sz+1"):
        add(f"tie_K_{dk}", 40, lambda nm, nu, row, dk=dk: tie_case(nm, nu, row, dk=dk, sc=900))
    for dk in ("sc", "sc+1"):  # (k = sc + sz is k = n: no sparse ratio; tests/test_gpu_high_ratio.py keeps n)
        add(f"tie_0_{dk}", 40, lambda nm, nu, row, dk=dk: tie_case(nm, nu, row, K=0, dk=dk, sc=150))
    add("tie_0_mid", 40, lambda nm, nu, row: tie_case(nm, nu, row, K=0, sc=900, rt=700))
    for s in ("kept", "dropped"):
        add(f"tie_sign_{s}", 768, lambda nm, nu, row, s=s: tie_case(nm, nu, row, signs=s, rt=7000, boundary=600,
                                                                   tie_units=list(range(600, 768))))
        add(f"window_sign_{s}", 40, lambda nm, nu, row, s=s: window_case(
            nm, nu, row, repeat=(30, 31, 32, 33, 34), kth="last",
            signs=(True, [True, True, True, False, True, True] if s == "kept" else [True, True, True, True, False, True]),
            extra=3))
    # the size classes
    for nu in BOUNDARY_SIZES:
        b = BOUNDARY_OF[nu]
        add(f"window_{nu}", nu, lambda nm, nu, row: window_case(nm, nu, row))
        add(f"tie_{nu}", nu, lambda nm, nu, row: tie_case(nm, nu, row))
        add(f"quota_{nu}", nu, lambda nm, nu, row, ru=(b, b, nu - 1, nu - 1): window_case(nm, nu, row, repeat=ru, kth="last",
                                                                                         extra=2))
    for nu in (32, 33):
        add(f"rank0_{nu}", nu, lambda nm, nu, row: sa_case(nm, nu, row, 0, 0.03, boundary=0))
    for nu, b in ((768, 512), (769, 512), (1536, 768), (1537, 768), (2048, 1536)):
        add(f"rank0_{nu}", nu, lambda nm, nu, row, b=b: sa_case(nm, nu, row, 0, 0.0099, boundary=b))
    # segment_pick's histogram tail: 1500 units are 47 groups, so the tail's last round of 8 is masked
    add("window_hist_tail_1500", 1500, lambda nm, nu, row: window_case(nm, nu, row, k=int(0.0099 * n_of(nu)),
                                                                       boundary=768, hist_tail=True))
    add("rank0_2049_forced", 2049, lambda nm, nu, row: _forced(sa_case(nm, nu, row, 0, 0.0099, boundary=1536)))
    return B


def _forced(c):
    c.route = "generic_forced"
    return c


BUILDERS = _builders()
PART_UNITS = 8000


def parts():
    """The case names split into plan parts of at most PART_UNITS large units (a latency-bound plan holds <= 8192), in
    the builders' order; each case is followed by its small segment, so case i of a part sits at row 2 i."""
    out, cur, units = [], [], 0
    for name, (nu, _) in BUILDERS.items():
        if cur and units + nu > PART_UNITS:
            out.append(cur)
            cur, units = [], 0
        cur.append(name)
        units += nu
    out.append(cur)
    return out


PARTS = parts()
ROW_OF = {name: (p, 2 * i) for p, names in enumerate(PARTS) for i, name in enumerate(names)}


@functools.lru_cache(maxsize=None)
def case(name):
    nu, fn = BUILDERS[name]
    c = fn(ROW_OF[name][1])
    if c.nu > M.UCAP and c.route.startswith("window"):  # more than UCAP units: the generic select, whatever the window
        c.route = "generic_forced"
        c.counts = {key: v for key, v in c.counts.items() if key in ("sa", "sc", "sz", "kth_key")}
    return c


def small_segment(row):
    return (np.random.default_rng(70 + row).standard_normal(SMALL_N) * 1e-3).astype(F32)


PIN_UNITS = 40
FILLER_UNITS = 8200


@functools.lru_cache(maxsize=None)
def gaussian(nu):
    return (np.random.default_rng(90 + nu).standard_normal(n_of(nu)) * 1e-3).astype(F32)


def part_cases(part, rmax):
    """The names of the part's cases that a plan of this rmax holds."""
    names = []
    for name in PARTS[part]:
        nm = name
        if "_rmax" in nm and not nm.endswith(f"_rmax{rmax}"):
            continue
        names.append(nm)
    return names


def plan_rows(part, rmax, batch):
    """(rows, xs, names): coalac_seg_t rows of the part's plan — every case, then its small segment, a Gaussian pin
    segment keeping rmax of its elements (the plan's largest ratio) and, in the batch plan, a Gaussian filler. A case
    that this rmax cannot hold (min_rmax, only_rmax) keeps its rows — the rows of the others must not move — as a
    Gaussian segment at ratio 0.001."""
    from tests.high_ratio_inputs import explicit_rows
    xs, ks, names = [], [], []
    for name in PARTS[part]:
        c = case(name)
        ok = c.min_rmax <= rmax and c.only_rmax in (None, rmax)
        if ok:
            xs.append(c.x)
            ks.append(c.k)
        else:
            xs.append(gaussian(c.nu))
            ks.append(max(1, c.x.size // 1000))
        names.append(name if ok else None)
        xs.append(small_segment(len(xs)))
        ks.append(SMALL_K)
        names.append(None)
    xs.append(gaussian(PIN_UNITS))
    ks.append(int(math.ceil(rmax * n_of(PIN_UNITS))))
    names.append(None)
    if batch:
        xs.append(gaussian(FILLER_UNITS))
        ks.append(int(math.ceil(0.001 * n_of(FILLER_UNITS))))
        names.append(None)
    return explicit_rows([x.size for x in xs], ks), xs, names
