// coalac.hip — MI355X (gfx950, CDNA4) model-update codec: CodecSpec v1 (per-segment exact top-k by
// |x| with lower-index tie-break, then b-bit min/max quantisation), behind the C ABI of include/coalac.h.
//
// Reference context: SonyResearch/COALA has no codec (coala/compression/__init__.py is 0 bytes); the
// hooks this replaces are coala/client/base.py:330-332 (encode) and coala/server/base.py:558-560
// (decode), and strategies.federated_averaging on the decoded uploads (aggregate).
// The spec is SURVEY.md §8(a) a3/a4; the CPU oracle restating it is oracle/codec_oracle.py.
//
// Design (DESIGN.md has the full rationale):
//   The path is HBM-bound integer/byte work: no MFMA. Encode must read the input ONCE from HBM, so the
//   exact top-k is found Floyd–Rivest style: per segment a small stratified sample brackets the k-th
//   key between two thresholds [T_lo, T_hi]; one streaming pass classifies every element as
//   A (key > T_hi: surely kept), B (T_lo <= key <= T_hi: maybe) or out, and writes A and B in index
//   order into per-unit candidate lists; a per-segment pass resolves the exact k-th key inside B;
//   a per-unit pass emits the sorted indices and codes. If a sample's bracket misses (count(A) > k or
//   count(A ∪ B) < k) the segment is re-selected exactly inside the same launch sequence (no host
//   round trip), so results are always exact.
//
//   Work unit = 4096 contiguous elements of one segment, owned by ONE wave64: ordered compaction is
//   done with wave ballots + mbcnt (records staged in the wave's LDS slice, flushed coalesced), so the
//   streaming pass has no block barriers. Segments of <= 1024 elements ("small"; COALAC_SMALL_MAX raises the
//   limit up to 4096) are encoded whole by one block in LDS.
//
//   Encode kernels, in stream order (launch_encode picks by plan class; "latency-bound" = at most
//   LATENCY_PLAN_UNITS large units, "batch" = more, "fork class" = small segments beside >= 16384 large units):
//     k_presel  batch plans: the samplers (one block per large segment: stratified sample -> [T_lo, T_hi]) and
//               the small segments (one block each) side by side
//     k_sample  latency-bound plans, the fork class and plans without small segments: the samplers alone
//     k_small   the fork class: the small segments on the plan's side stream, beside k_sample / k_scan
//     k_scan    one wave per large unit (128-thread blocks in batches): single HBM read, classify A / B,
//               candidate records in index order (u16 position + u32 value bits, 6 B each); in latency-bound
//               plans its first blocks encode the small segments (the WITH_SMALL instantiation)
//     k_ghist   one block per 32-unit group: band histogram of the group's B records
//     k_gwin    one block per group: sum the segment's group histograms -> key window of the k-th key
//               (every group block of the segment, redundantly); per-unit counts above the window + the
//               group's in-window entries (latency-bound plans: both sweep their records speculatively)
//     k_select  one block per large segment: exact k-th key + tie quota from the window lists (generic
//               multi-pass select / exact re-select on a bracket miss), per-unit output offsets (= the
//               payload's per-unit starts, wire v2), min / max -> scale, per-unit emit parameters
//     k_emit    one wave per EMIT_UPW large units (1 in latency-bound plans, one load round): kept records ->
//               ascending idx + codes
//   Decode: k_decode_lds — every output line written once, the unit's kept values placed through a per-wave
//   LDS tile; entry ranges from the payload's per-unit starts (wire v2; a host that received a v1 blob computes
//   them, coala_amd/compression/plan.py).
//   Aggregate (fused decode + FedAvg, server side): k_aggregate — two waves per unit, a per-wave LDS tile
//   holding the unkept x (base + 0), each client's kept values written in and read back in client order.
//   Dense plans (every segment keeps all its elements, ratio 1): k_dense_minmax -> k_dense_seg -> k_dense_quant
//   encode, k_dense_deq decode — the indices implied, never materialised.
//   Error feedback (client side): k_ef_accumulate (r = (x - base) + r, one stream) before an encode of
//   r, k_ef_commit / k_ef_commit_dense (r -= what the decoder will reconstruct, at the kept entries) after it.
//
// Numerics: built with -ffp-contract=off; fp32 sub/div/mul/add are separate IEEE ops, rintf is
// round-half-even — the same op sequence as the oracle, so decoded values are bit-identical.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/coalac.h"

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr uint32_t UNIT = 4096;           // elements per wave work unit
constexpr uint32_t UNIT_SHIFT = 12;
constexpr uint32_t UNIT_IT = UNIT / 256;  // float4 loads per lane per unit
constexpr uint32_t SMALL_MAX = 4096;      // segments up to this size can be encoded whole in one block (the
                                          // small-segment LDS arena; COALAC_SMALL_MAX may raise the limit to it)
constexpr uint32_t SMALL_MAX_BATCH = 1024;  // ... and are, by default, in batch plans (4096 until round 3: C2
                                            // 0.296-0.314 -> 0.280-0.285 ms per step, C3 / C4 equal or faster;
                                            // a 4096-element block select takes 14 us, the sampled path streams it)
constexpr uint32_t SMALL_MAX_LATENCY = 1024;  // ... in latency-bound plans (<= LATENCY_PLAN_UNITS units): a
                                              // block's radix select grows with n (64: 5 us, 2048: 9 us,
                                              // 4096: 14 us, alone on a CU) and the slowest small segment set
                                              // the length of k_presel; bigger segments take the sampled path
constexpr uint32_t LATENCY_PLAN_UNITS = 8192;  // ~1.3 ResNet-50 updates
constexpr uint32_t SAMPLE_MAX = 8192u;  // sampled keys per large segment
constexpr int SEL_NT = 256;               // threads of a k_select block in batches (4 waves: one per SIMD, so
                                          // a block finds room beside a streaming kernel's waves)
constexpr int GWIN_NT_LAT = 512;  // k_gwin block in latency-bound plans (256 or 512: one or two histogram bins per thread)
constexpr int GHIST_NT_LAT = 1024;  // k_ghist block in latency-bound plans (256 / 512 / 1024: 6.5 / 5.7 / 5.3 us on one update)
constexpr int SEL_NT_LAT = 512;           // ... in latency-bound plans, where nothing streams beside it (one
                                          // ResNet-50 update: k_select 11.3 -> 10.2 us; batches measured slower)
constexpr int SCAN_WPE = 5;
constexpr int SCAN_NT = 128;  // batch plans' k_scan block size (launch bounds: SCAN_WPE waves per SIMD; C3 0.584 vs 0.616 ms at 256)
constexpr int SCAN_NT_LAT = 256;  // latency-bound plans' k_scan block size (its first blocks encode the small segments)
constexpr int SCAN_NB = 1;  // load batches per k_scan unit (weights mode): 1 = all 16 float4 per lane in flight
constexpr int SCAN_WPE_LAT = 6;  // latency-bound plans' k_scan: blocks per CU (5 / 1 batch: 24.5 us, 6 / 2: 23.0, 6 / 1
                                 // spills: 31.7, 8 / 4: 24.2 on one update; batches keep SCAN_WPE / SCAN_NB)
constexpr int SCAN_WPE_LAT_1K = 7;  // ... with the default 1024-element small segments (a 16 KB arena): 7 blocks per CU, so
                                    // one ResNet-50 update's ~1,660 blocks fit one round of the chip's block slots
constexpr int SCAN_NB_LAT = 2;  // ... and load batches per unit
constexpr int SAMPLE_NT_LAT = 256;  // latency-bound plans' k_sample block size (1024 threads, 2 load batches each: 0.7 us slower)
constexpr int LOAD_AUX = 2;   // cache policy of the streaming buffer loads (k_scan, the quantise stream): non-temporal
constexpr int STORE_AUX = 2;  // cache policy of the streaming buffer stores (batch k_decode_lds, k_dense_deq): non-temporal
constexpr uint32_t STAGE_CAP = 512;       // candidate records staged in LDS per k_scan wave
constexpr int GSWEEP = 4;  // units per record-load batch of a balanced group sweep (batch plans)
constexpr uint32_t GU = 32;               // units per select group (k_ghist / k_gwin block)
constexpr uint32_t HB2 = 512;             // bins of the per-group band histograms
constexpr uint32_t GCAP = 256;            // in-window entries a group may hand to k_select
constexpr uint32_t KEY_MAX = 0x7FFFFFFFu;
constexpr uint32_t TIE_FLAG = 0x80000000u;  // in a unit's T_lo: the sampled k-th key K is a heavy tie (tie mode, k_scan)
constexpr int HIST_BINS = 2048;
constexpr uint32_t UCAP = 2048;           // units per k_select chunk (8.4 M elements)
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr int NSTAMP = 32;  // diagnostics slots per segment row (COALAC_FLAG_STAMPS)

struct SegDev {
  uint64_t in_off;
  uint64_t out_off;
  uint32_t n, k;
  uint32_t unit_begin, unit_end;  // range in the all-units table (decode)
  uint32_t lu_begin;              // first large-unit index (large segments)
  uint32_t g_begin;               // first select group (large segments)
};

struct UnitDev {
  uint64_t off;      // element offset of the unit in the flat buffer (= seg.in_off + start)
  uint64_t out_off;  // the segment's out_off
  uint32_t seg, start;
  uint32_t k;        // the segment's k
  uint16_t len;      // elements in this unit (<= UNIT)
  uint16_t last;     // 1 if this is the segment's last unit
};
static_assert(sizeof(UnitDev) == 32, "UnitDev layout");

struct Params {
  // encode / decode operands
  const float* in;
  const float* const* inptr;  // encode from per-segment pointers (coalac_encode_segptr), else null
  const float* base;
  int32_t* idx;
  void* vals;
  float* mn;
  float* scale;
  uint32_t* ustart_out;  // encode: per-unit start of the unit's kept entries (segment-relative), or null
  const int32_t* cidx;
  const void* cvals;
  const float* cmn;
  const float* cscale;
  float* out;
  // plan metadata
  const SegDev* segs;
  const UnitDev* units;   // all units (decode)
  const UnitDev* lunits;  // units of large segments (encode)
  const uint32_t* small_list;
  const uint32_t* large_list;
  const SegDev* lsegs;  // [n_large] the large segments' SegDev, in large_list order (one load round less)
  const SegDev* ssegs;  // [n_small] the small segments' SegDev, in small_list order (likewise)
  uint32_t nseg, n_small, n_large, n_units, n_lunits;
  uint32_t scan_small;  // small segments encoded by k_scan's first blocks (0 when forked to k_small)
  float levels;
  unsigned flags;
  // encode workspace: per segment
  uint32_t *tstar, *rtie, *status;
  // per large unit
  uint32_t *tlo, *thi, *cntA, *cntC, *gtC, *eqC, *eqpre, *outoff;
  uint32_t* cntZ;  // per large unit of a tie-mode segment (T_lo == 0, or flagged): its keys equal to the tie key K
                   // (0, or T_lo & KEY_MAX) — counted, not recorded
  uint32_t* tsgn;  // ... and, for K > 0, the in-unit tie rank of its first positive (bits 0-15) and first negative
                   // (bits 16-31) tie, 0xFFFF = none (a kept +K / -K tie enters mn / scale; a zero's sign does not)
  uint4* uemit;  // per large unit, from k_select: {T*, tie budget | raw-path flag << 31, mn bits, scale bits}
  uint32_t* cval;  // candidate records, ccap slots per large unit, in index order: the value bits ...
  uint16_t* cpos;  // ... and the position inside the unit (the emit reads both; every select sweep the values only)
  uint32_t ccap;  // record slots per large unit, in [STAGE_CAP, UNIT] (below UNIT a unit that finds more candidates
                  // overflows and its segment is selected and emitted from the raw data instead; coalac_plan_create's
                  // UNIT * (2 rmax + 0.05) + 256 reaches UNIT from a largest ratio of ~0.44 on, and is UNIT for every
                  // rmax >= 0.475: every element can be a record and no unit overflows)
  // parallel select (groups of GU units of one large segment)
  const uint4* groups;     // {large-segment index, first large unit, units, segment}
  const uint4* gseg;       // per group, its segment: {first large unit, units, k, first group}
  uint32_t n_groups;
  uint32_t* ghist;         // [n_groups][HB2]
  uint32_t* gcnt;          // [n_groups] in-window entries found by the group
  uint2* glist;            // [n_groups][GCAP] {value bits, unit index within the segment}
  float* gmm;              // [n_groups][2] min/max of the group's values above the window
  uint4* sstate;           // [n_large] {wlo, whi, rank inside the window, path: 0 fast / 1 generic}
  uint32_t* shhi;          // [n_large] histogram upper bound: min(T_hi, largest sampled key)

  // decode: first kept entry (segment-relative) of every unit — the payload's (wire v2)
  const uint32_t* ustart;
  // dense plans (every segment keeps all its elements): per unit the NaN-ignoring {min, max} of its values
  float* umm;
  // diagnostics: per-block phase timestamps (COALAC_FLAG_STAMPS), NSTAMP per block, 100 MHz ticks
  uint64_t* stamps;
};

// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
#define DEV __device__ __forceinline__

DEV uint32_t fkey(float x) { return __float_as_uint(x) & KEY_MAX; }

// diagnostics only: thread 0 records the 100 MHz real-time counter for phase i of large segment li
#define STAMP(P, li, i)                                                                             \
  do {                                                                                              \
    if ((P).stamps != nullptr && threadIdx.x == 0)                                                  \
      (P).stamps[(uint64_t)(li) * NSTAMP + (i)] = __builtin_amdgcn_s_memrealtime();                \
  } while (0)

// NaN-ignoring min/max (NaN only if both are NaN) = IEEE minNum/maxNum: one v_min_f32 / v_max_f32
// (hipcc quiets signalling NaNs first, so a NaN operand is always ignored). The sign of a zero result is
// canonicalised at the end (+ 0.0f), which makes the reduction order-independent.
DEV float fmin_nan(float a, float b) { return __builtin_fminf(a, b); }
DEV float fmax_nan(float a, float b) { return __builtin_fmaxf(a, b); }
DEV float qnan() { return __int_as_float(0x7FC00000); }

DEV uint32_t lane_id() { return __lane_id(); }

// lane l's value of v (v_readlane: a wave-uniform result)
DEV uint32_t rl(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }

// XCD-aware block order: workgroups are dispatched round-robin over the 8 XCDs (block b on XCD b % 8); the
// remapped index gives XCD x the x-th contiguous share of [0, gridDim.x) (a bijection for any grid size), so
// each XCD streams through one region instead of every eighth 64 KiB. NT stores of the unit pattern, 1.5 GiB:
// 5.56 -> 6.38 TB/s (tools/store_probe.hip); reads and ~100 MB buffers gain nothing.
DEV uint32_t xcd_block(uint32_t b) {
  const uint32_t nb = gridDim.x, q = nb / 8, r = nb % 8, x = b % 8, i = b / 8;
  return x * q + min(x, r) + i;
}

// number of set bits of `m` in lanes below this lane
DEV uint32_t mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Cross-lane steps by DPP (a VALU operand modifier: a few cycles) — __shfl_* lowers to ds_bpermute_b32, an LDS round
// trip per step (~100+ cycles), and a wave scan is six dependent steps. dpp<CTRL>: lane i reads lane src(i) of v
// (0 where the source lies outside its row or the row is masked off). CTRL: 0x111 + n - 1 row_shr:n, 0x128 row_ror:8,
// 0x140 row_mirror, 0x141 row_half_mirror, 0x142 row_bcast:15, 0x143 row_bcast:31, 0xB1 / 0x4E quad_perm xor 1 / xor 2.
// min(a, b) kept out of the optimiser's reach: next to min(r, x), the tie quota `x >= r ? 0 : min(c, r - x)` was folded
// into a saturating subtract whose clamp the gfx950 build then dropped — min(r, x) came out as x and a unit reserved a
// slot for a tie it did not keep (k_select, round 6: tools/dbg_encode.py, resnet18 ratio 0.1 delta). With qp = this,
// the quota is min(c, r - qp): r - qp never wraps.
DEV uint32_t umin_opaque(uint32_t a, uint32_t b) {
  uint32_t r;
  asm("v_min_u32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

template <int CTRL, int ROWM = 0xF>
DEV uint32_t dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWM, 0xF, false);
}

// inclusive prefix sum over the 64 lanes (all lanes active)
DEV uint32_t wave_incl_scan(uint32_t v) {
  v += dpp<0x111>(v);  // row_shr:1, 2, 4, 8: each 16-lane row scanned
  v += dpp<0x112>(v);
  v += dpp<0x114>(v);
  v += dpp<0x118>(v);
  v += dpp<0x142, 0xA>(v);  // row_bcast:15 into rows 1, 3
  v += dpp<0x143, 0xC>(v);  // row_bcast:31 into rows 2, 3
  return v;
}

// reduction over the 64 lanes, the result in every lane: within each row by quad / half-row / row mirrors, then the
// four rows' values by readlane
template <class OP>
DEV uint32_t wave_reduce(uint32_t v, OP op) {
  v = op(v, dpp<0xB1>(v));
  v = op(v, dpp<0x4E>(v));
  v = op(v, dpp<0x141>(v));
  v = op(v, dpp<0x140>(v));
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return op(op(a, b), op(c, d));
}

DEV float wave_min(float v) {
  return __uint_as_float(wave_reduce(__float_as_uint(v), [](uint32_t a, uint32_t b) {
    return __float_as_uint(fmin_nan(__uint_as_float(a), __uint_as_float(b)));
  }));
}

DEV float wave_max(float v) {
  return __uint_as_float(wave_reduce(__float_as_uint(v), [](uint32_t a, uint32_t b) {
    return __float_as_uint(fmax_nan(__uint_as_float(a), __uint_as_float(b)));
  }));
}

DEV uint32_t wave_min_u32(uint32_t v) {
  return wave_reduce(v, [](uint32_t a, uint32_t b) { return min(a, b); });
}

DEV uint32_t wave_max_u32(uint32_t v) {
  return wave_reduce(v, [](uint32_t a, uint32_t b) { return max(a, b); });
}

DEV uint32_t wave_sum(uint32_t v) {
  return wave_reduce(v, [](uint32_t a, uint32_t b) { return a + b; });
}

// Order one wave's own LDS accesses (a scatter, then reads of the same tile by other lanes): the LDS executes a
// wave's DS instructions in issue order, so only the compiler must not move them across this point. Unlike
// wave_fence (a wavefront-scope seq_cst fence), it emits no s_waitcnt: loads in flight stay in flight.
DEV void lds_order() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

DEV void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// stores of the select phases' per-group / per-segment results (plain global stores)
DEV void pst(const Params&, uint32_t* p, uint32_t v) { *p = v; }
DEV void pst(const Params&, float* p, float v) { *p = v; }
DEV void pst(const Params&, uint2* p, uint2 v) { *p = v; }

// Block-wide exclusive scan over NT threads. sh needs >= NT/64 words. Returns the exclusive prefix and
// the block total. Contains barriers: call from all threads.
template <int NT>
DEV uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  constexpr int NW = NT / 64;
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  uint32_t inc = wave_incl_scan(v);
  __syncthreads();
  if (lane == 63) sh[w] = inc;
  __syncthreads();
  uint32_t off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    uint32_t s = sh[i];
    if ((uint32_t)i < w) off += s;
    tot += s;
  }
  total = tot;
  return off + inc - v;
}

// Two block-wide exclusive scans sharing one pair of barriers (sh needs >= 2 * NT/64 words). Call from all threads.
template <int NT>
DEV void block_excl_scan2(uint32_t a, uint32_t b, uint32_t* sh, uint32_t& ea, uint32_t& eb, uint32_t& ta,
                          uint32_t& tb) {
  constexpr int NW = NT / 64;
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  const uint32_t ia = wave_incl_scan(a), ib = wave_incl_scan(b);
  __syncthreads();
  if (lane == 63) {
    sh[w] = ia;
    sh[NW + w] = ib;
  }
  __syncthreads();
  uint32_t oa = 0, ob = 0, sa = 0, sb = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t x = sh[i], y = sh[NW + i];
    if ((uint32_t)i < w) {
      oa += x;
      ob += y;
    }
    sa += x;
    sb += y;
  }
  ea = oa + ia - a;
  eb = ob + ib - b;
  ta = sa;
  tb = sb;
}

template <int NT>
DEV uint32_t block_sum(uint32_t v, uint32_t* sh) {
  uint32_t t;
  block_excl_scan<NT>(v, sh, t);
  return t;
}

// shf needs >= 2 * NT/64 floats
template <int NT>
DEV void block_minmax(float& mn, float& mx, float* shf) {
  constexpr int NW = NT / 64;
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  mn = wave_min(mn);
  mx = wave_max(mx);
  __syncthreads();
  if (lane == 0) {
    shf[w] = mn;
    shf[NW + w] = mx;
  }
  __syncthreads();
  float a = shf[0], b = shf[NW];
#pragma unroll
  for (int i = 1; i < NW; ++i) {
    a = fmin_nan(a, shf[i]);
    b = fmax_nan(b, shf[NW + i]);
  }
  mn = a;
  mx = b;
}

// Exact selection of the r-th largest key (1-based) among the keys in [lo, hi] that `for_each`
// enumerates (each thread enumerates its own share; the union is the key multiset). Returns T with
// count(key in (T, hi]) < r <= count(key in [T, hi]) and leaves in r the number of keys == T to take
// (r - count(key in (T, hi])). Radix narrowing with 2048-bin LDS histograms: at most 3 passes over the
// keys for a full 31-bit range. Once the bin holding the r-th key has at most RANK_MAX keys, they are
// gathered into LDS (one more enumeration) and ranked against each other instead of further radix passes
// (a small segment's keys crowd a few exponent bins: 3 passes -> 1 pass + gather + rank). sh needs >= 64
// words (broadcast slots sh[36]-sh[41]).
constexpr uint32_t RANK_MAX = 256;

template <int NT, class ForEach>
DEV uint32_t rank_select(ForEach&& for_each, uint32_t lo, uint32_t hi, uint32_t& r, uint32_t* cand, uint32_t* sh) {
  const uint32_t t = threadIdx.x, lane = lane_id();
  if (t == 0) {
    sh[39] = 0;
    sh[36] = lo;
    sh[37] = r;
  }
  __syncthreads();
  for_each([&](uint32_t key) {  // wave-aggregated append of the bin's keys
    const bool in = key >= lo && key <= hi;
    const uint64_t m = __ballot(in);
    if (m) {
      const uint32_t leader = (uint32_t)__ffsll((long long)m) - 1u;
      uint32_t base = 0;
      if (lane == leader) base = atomicAdd(&sh[39], (uint32_t)__popcll(m));
      base = (uint32_t)__builtin_amdgcn_readlane((int)base, (int)leader);
      if (in) cand[base + mbcnt(m)] = key;
    }
  });
  __syncthreads();
  const uint32_t c = sh[39];
  for (uint32_t i = t; i < c; i += NT) {
    const uint32_t ki = cand[i];
    uint32_t g = 0, e = 0;
    for (uint32_t j = 0; j < c; ++j) {  // every thread reads the same word: LDS broadcast
      const uint32_t kj = cand[j];
      g += kj > ki ? 1u : 0u;
      e += kj == ki ? 1u : 0u;
    }
    if (g < r && r <= g + e) {  // the r-th key (every tie of it writes the same two words)
      sh[36] = ki;
      sh[37] = r - g;
    }
  }
  __syncthreads();
  const uint32_t T = sh[36];
  r = sh[37];
  __syncthreads();
  return T;
}

template <int NT, int NB = HIST_BINS, class ForEach>
DEV uint32_t block_select(ForEach&& for_each, uint32_t lo, uint32_t hi, uint32_t& r, uint32_t* hist,
                          uint32_t* sh) {
  constexpr int BPT = NB / NT;  // bins per thread
  constexpr int BITS = NB == 2048 ? 11 : NB == 1024 ? 10 : NB == 512 ? 9 : 8;
  static_assert((1 << BITS) == NB, "power-of-two bins");
  const uint32_t t = threadIdx.x;
  while (lo < hi) {
    const uint32_t w = hi - lo;
    const int bl = 32 - __clz(w);
    const int shift = bl > BITS ? bl - BITS : 0;
    for (uint32_t i = t; i < NB; i += NT) hist[i] = 0;
    __syncthreads();
    const uint32_t l0 = lo, h0 = hi;
    for_each([&](uint32_t key) {
      if (key >= l0 && key <= h0) atomicAdd(&hist[(key - l0) >> shift], 1u);
    });
    __syncthreads();
    uint32_t c[BPT];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
      c[j] = hist[t * BPT + j];
      s += c[j];
    }
    uint32_t total;
    const uint32_t ex = block_excl_scan<NT>(s, sh, total);
    const uint32_t above = total - ex - s;  // keys in bins above this thread's bins
    if (t == 0) {
      sh[40] = NONE;
      sh[41] = r;
    }
    __syncthreads();
    if (above < r && r <= above + s) {
      uint32_t acc = above, cb = 0;
      int b = (int)(t * BPT);
#pragma unroll
      for (int j = BPT - 1; j >= 0; --j) {
        if (acc + c[j] >= r) {
          b = (int)(t * BPT) + j;
          cb = c[j];
          break;
        }
        acc += c[j];
      }
      sh[40] = (uint32_t)b;
      sh[41] = r - acc;
      sh[38] = cb;  // keys in the chosen bin
    }
    __syncthreads();
    const uint32_t b = sh[40];
    r = sh[41];
    const uint32_t bc = sh[38];
    __syncthreads();
    if (b == NONE) return lo;  // precondition violated (cannot happen for valid inputs)
    lo = lo + (b << shift);
    const uint32_t nhi = lo + ((1u << shift) - 1u);
    hi = nhi < hi ? nhi : hi;
    if (lo < hi && bc <= RANK_MAX && NB >= (int)RANK_MAX)
      return rank_select<NT>(for_each, lo, hi, r, hist, sh);
  }
  return lo;
}

DEV uint8_t quantize(float v, float mn, float scale, float levels) {
  if (!(scale > 0.0f)) return 0;
  const float t = (v - mn) / scale;
  const float r = rintf(t);
  if (!(r > 0.0f)) return 0;
  return (uint8_t)(r < levels ? r : levels);
}

DEV float dequantize(uint8_t q, float mn, float scale) {
  const float p = (float)q * scale;
  return mn + p;
}

// The range of CodecSpec v1 from the kept values' NaN-ignoring min a and max b: each + 0.0f (a canonical zero), mn = a,
// scale = one level's share of b - a, or 0 when they are equal. The one copy: every encoder's mn / scale is this op sequence.
DEV void codec_range(float a, float b, float levels, float& mn, float& scale) {
  a = a + 0.0f;
  b = b + 0.0f;
  mn = a;
  scale = (b == a) ? 0.0f : (b - a) / levels;
}

template <bool RAW>
DEV void store_val(const Params& P, uint64_t o, float v, float mn, float scale) {
  if (RAW)
    static_cast<float*>(P.vals)[o] = v;
  else
    static_cast<uint8_t*>(P.vals)[o] = quantize(v, mn, scale, P.levels);
}

template <bool RAW>
DEV float load_val(const Params& P, uint64_t o, float mn, float scale) {
  if (RAW) return static_cast<const float*>(P.cvals)[o];
  return dequantize(static_cast<const uint8_t*>(P.cvals)[o], mn, scale);
}

template <bool RAW>
DEV uint32_t load_code(const Params& P, uint64_t o) {
  if (RAW) return __float_as_uint(static_cast<const float*>(P.cvals)[o]);
  return static_cast<const uint8_t*>(P.cvals)[o];
}

template <bool RAW>
DEV float code_value(uint32_t q, float mn, float scale) {
  return RAW ? __uint_as_float(q) : dequantize((uint8_t)q, mn, scale);
}

template <bool DELTA>
DEV float4 load_x4(const Params& P, uint64_t off) {
  float4 v = *reinterpret_cast<const float4*>(P.in + off);
  if (DELTA) {
    const float4 b = *reinterpret_cast<const float4*>(P.base + off);
    v.x = v.x - b.x;
    v.y = v.y - b.y;
    v.z = v.z - b.z;
    v.w = v.w - b.w;
  }
  return v;
}

typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f2v __attribute__((ext_vector_type(2)));

// histogram shift of the sampled band [tlo, thi]: HIST_BINS bins of 2^shift keys cover it. k_scan
// (band histogram) and k_select (bin -> key window) must agree, so both use this.
DEV int band_shift(uint32_t tlo, uint32_t thi, int bin_bits = 11) {
  const uint32_t w = thi - tlo;
  if (w == 0) return 0;
  const int bl = 32 - __clz(w);
  return bl > bin_bits ? bl - bin_bits : 0;
}

// Buffer resource over `bytes` bytes at p (gfx9 word 3): a load at a byte offset >= bytes returns 0, a store there is
// dropped. unit_rsrc: over n fp32 elements.
DEV __amdgpu_buffer_rsrc_t bytes_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
DEV __amdgpu_buffer_rsrc_t unit_rsrc(const float* p, uint32_t n) { return bytes_rsrc(p, n * 4u); }

// non-temporal 16-byte buffer load (aux bit 1 = nt on gfx94x/gfx950) of x (or x - base) at byte offset
template <bool DELTA>
DEV float4 unit_load_x4(__amdgpu_buffer_rsrc_t rin, __amdgpu_buffer_rsrc_t rbase, uint32_t boff) {
  typedef unsigned int u4v __attribute__((ext_vector_type(4)));
  const u4v a = __builtin_amdgcn_raw_buffer_load_b128(rin, (int)boff, 0, LOAD_AUX);
  float4 v = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
  if (DELTA) {
    const u4v b = __builtin_amdgcn_raw_buffer_load_b128(rbase, (int)boff, 0, LOAD_AUX);
    v.x = v.x - __uint_as_float(b.x);
    v.y = v.y - __uint_as_float(b.y);
    v.z = v.z - __uint_as_float(b.z);
    v.w = v.w - __uint_as_float(b.w);
  }
  return v;
}

// non-temporal 16-byte buffer store (dropped when it lies past the resource's range)
template <int AUX = STORE_AUX>
DEV void unit_store_x4(__amdgpu_buffer_rsrc_t r, uint32_t boff, float4 v) {
  typedef unsigned int u4v __attribute__((ext_vector_type(4)));
  const u4v a = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
  __builtin_amdgcn_raw_buffer_store_b128(a, r, (int)boff, 0, AUX);
}

// the same 16 bytes as four dword stores: the range check drops exactly the dwords past the end
template <int AUX = STORE_AUX>
DEV void unit_store_x1x4(__amdgpu_buffer_rsrc_t r, uint32_t boff, float4 v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.x), r, (int)boff, 0, AUX);
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.y), r, (int)boff + 4, 0, AUX);
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.z), r, (int)boff + 8, 0, AUX);
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v.w), r, (int)boff + 12, 0, AUX);
}

// non-temporal (read-once) 16-byte load of x (or x - base)
template <bool DELTA>
DEV float4 load_x4_nt(const Params& P, uint64_t off) {
  const f4v a = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(P.in + off));
  float4 v = make_float4(a.x, a.y, a.z, a.w);
  if (DELTA) {
    const f4v b = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(P.base + off));
    v.x = v.x - b.x;
    v.y = v.y - b.y;
    v.z = v.z - b.z;
    v.w = v.w - b.w;
  }
  return v;
}

template <bool DELTA>
DEV float load_x1(const Params& P, uint64_t off) {
  float v = P.in[off];
  if (DELTA) v = v - P.base[off];
  return v;
}

// Input of segment s: its own pointer (coalac_encode_segptr: the model's parameter storage, no flattening
// copy) or the flat buffer at in_off. The delta base is always the flat buffer.
DEV const float* seg_in(const Params& P, uint32_t s, uint64_t in_off) {
  return P.inptr != nullptr ? P.inptr[s] : P.in + in_off;
}

template <bool DELTA>
DEV float4 load_x4p(const float* x, const float* b) {
  float4 v = *reinterpret_cast<const float4*>(x);
  if (DELTA) {
    const float4 c = *reinterpret_cast<const float4*>(b);
    v.x = v.x - c.x;
    v.y = v.y - c.y;
    v.z = v.z - c.z;
    v.w = v.w - c.w;
  }
  return v;
}

template <bool DELTA>
DEV float load_x1p(const float* x, const float* b) {
  float v = *x;
  if (DELTA) v = v - *b;
  return v;
}

DEV uint32_t hash32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// Group-histogram geometry of a segment: bins of 2^shift keys over [tlo, hhi]; keys in (hhi, thi] are
// clamped into the last bin, whose key window therefore ends at thi.
struct Band {
  uint32_t tlo, thi, hhi, last;
  int shift;
  DEV Band(uint32_t lo, uint32_t hi, uint32_t hh) : tlo(lo), thi(hi), hhi(hh) {
    shift = band_shift(lo, hh, 9);
    last = (hh - lo) >> shift;
  }
  DEV uint32_t bin(uint32_t key) const { return key > hhi ? last : (key - tlo) >> shift; }
  DEV uint32_t wlo(uint32_t b) const { return tlo + (b << shift); }
  DEV uint32_t whi(uint32_t b) const { return b == last ? thi : min(thi, wlo(b) + ((1u << shift) - 1u)); }
};

// ------------------------------------------------------------------------------------------------
// streaming classify + ordered compaction of one large unit by one wave (k_scan, exact fallback)
// Candidates (key >= tlo) are written in index order as records {position in the unit, value}: two arrays, the
// u16 positions (cpos) and the value bits (cval) — 6 bytes per record, and the select sweeps, which read values
// only, move 4 (round 3's interleaved 8-byte records: k_scan's writes were 4.4 % of its read traffic). With `stage` (k_scan) the first STAGE_CAP records go to a per-wave
// LDS buffer and leave in coalesced 512-byte stores at the end; scattered per-lane global stores were
// measured 28 % slower (tools/scan_ablate.hip). Input loads are non-temporal: the update is read once.
// The unit is loaded in NB batches of UNIT_IT/NB float4 per lane: NB = 1 for the streaming pass (all
// loads in flight at once), more for the register-lean fallback inside k_select.
// ------------------------------------------------------------------------------------------------
// CHECK: test each element against the unit's length. A full unit never needs it, nor does a partial one when
// tlo > 0 (its loads past len return 0, key 0 < tlo): k_scan picks the lean form then (wave-uniform).
// ZERO = tie mode, for a segment whose k-th key may be one heavily repeated key K: K = 0 when the bracket starts at
// key 0 (tlo == 0: a frozen or pruned tensor, an all-zero delta), or the K the sampler flagged (T_lo = K | TIE_FLAG,
// T_hi = K: its samples around the k-th rank were all K — a sign-SGD or first-Adam-step delta whose |x| are all equal,
// values clipped at a bound, a quantised tensor). Keys equal to K are COUNTED per unit (cntZ), not recorded; the
// candidates are the keys above K (in [K + 1, thi], and above). The select then takes the k-th key as K with a tie
// quota over the K-keys (index order) when the keys above K number fewer than k, and only the units whose K-keys that
// quota reaches re-read their raw data in k_emit — instead of every element becoming a candidate record, every unit
// overflowing its slots and the whole segment taking the one-block raw-data path (one ResNet-50 update of equal-|x|
// values: 9.0 ms per encode + decode on that path, tools/tie_probe.py). For K > 0 the scan also records the in-unit
// rank of the first positive and first negative K-key (tsgn): whether +K / -K is among the kept values.
template <bool DELTA, int NB, bool CHECK = true, bool ZERO = false>
DEV void scan_unit(const Params& P, uint32_t lu, const UnitDev& L, const uint32_t tlo_, const uint32_t thi,
                   uint2* stage) {
  const uint32_t tk = tlo_ & KEY_MAX;     // (ZERO: the tie key K)
  const uint32_t tlo = ZERO ? tk + 1u : tlo_;
  uint32_t cz = 0;                        // K-keys this lane saw (ZERO)
  uint32_t weq = 0, rp = NONE, rn = NONE;  // (ZERO, K > 0: K-keys of the earlier rows; first +K / -K tie rank)
  constexpr uint32_t IT = UNIT_IT / NB;
  const uint32_t lane = lane_id();
  const uint32_t len = L.len;
  const uint64_t off = L.off;
  uint32_t* RV = P.cval + (uint64_t)lu * P.ccap;
  uint16_t* RP = P.cpos + (uint64_t)lu * P.ccap;
  const uint32_t cap = P.ccap;
  uint32_t cC = 0, cA = 0;
  // buffer resources over exactly this unit: one shared lane offset for all loads (constant offsets
  // fold into the instruction), and loads past len return 0 — no separate partial-unit path
  const float* xin = P.inptr != nullptr ? P.inptr[L.seg] + L.start : P.in + off;
  const __amdgpu_buffer_rsrc_t rin = unit_rsrc(xin, len);
  const __amdgpu_buffer_rsrc_t rbase = unit_rsrc(DELTA ? P.base + off : xin, len);
  auto put = [&](uint32_t i, uint2 rec) {
    if (i >= cap) return;  // overflow: counted, not stored (the segment goes to the raw-data path)
    RV[i] = rec.y;
    RP[i] = (uint16_t)rec.x;
  };

  for (uint32_t nb = 0; nb < (uint32_t)NB; ++nb) {
    float4 v[IT];
#pragma unroll
    for (uint32_t i = 0; i < IT; ++i) v[i] = unit_load_x4<DELTA>(rin, rbase, ((nb * IT + i) * 64 + lane) * 16);
#pragma unroll
    for (uint32_t i = 0; i < IT; ++i) {
      const uint32_t e0 = ((nb * IT + i) * 64 + lane) * 4;
      const float xs[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
      bool fc[4], fa[4];
      bool any = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t key = fkey(xs[j]);
        fc[j] = (!CHECK || e0 + j < len) && key >= tlo;
        fa[j] = CHECK ? fc[j] && key > thi : key > thi;  // (thi >= tlo or ZERO: key > thi implies a candidate)
        if (ZERO) cz += ((!CHECK || e0 + j < len) && key == tk) ? 1u : 0u;
        any = any || fc[j];
      }
      if (ZERO && tk != 0u) {  // (wave-uniform) the in-unit ranks of this row's K-keys: index order is (lane, j)
        uint64_t tb[4];
        uint32_t pre = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          tb[j] = __ballot((!CHECK || e0 + j < len) && fkey(xs[j]) == tk);
          pre += mbcnt(tb[j]);
        }
        uint32_t mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if ((tb[j] >> lane) & 1ull) {
            const uint32_t rank = weq + pre + mine;
            if (__float_as_uint(xs[j]) >> 31)
              rn = min(rn, rank);
            else
              rp = min(rp, rank);
            ++mine;
          }
        }
        weq += (uint32_t)(__popcll(tb[0]) + __popcll(tb[1]) + __popcll(tb[2]) + __popcll(tb[3]));
      }
      const uint32_t c = (uint32_t)fc[0] + (uint32_t)fc[1] + (uint32_t)fc[2] + (uint32_t)fc[3];
      const uint64_t b1 = __ballot(any);
      if (b1 == 0) continue;
      if (__ballot(c >= 2) == 0) {
        // common case (~1.5 % candidates: ~4 per 256-element row): at most one candidate per lane, so its
        // position is one mbcnt instead of four, and each lane writes at most one record
        cA += (uint32_t)__popcll(__ballot(fa[0] || fa[1] || fa[2] || fa[3]));
        if (any) {
          const uint32_t pc = cC + mbcnt(b1);
          const uint32_t j = fc[0] ? 0u : fc[1] ? 1u : fc[2] ? 2u : 3u;
          const float xj = j == 0 ? xs[0] : j == 1 ? xs[1] : j == 2 ? xs[2] : xs[3];
          const uint2 rec = make_uint2(e0 + j, __float_as_uint(xj));
          if (stage != nullptr && pc < STAGE_CAP)
            stage[pc] = rec;
          else
            put(pc, rec);
        }
        cC += (uint32_t)__popcll(b1);
        continue;
      }
      uint64_t bc[4];
      uint32_t pc = cC;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bc[j] = __ballot(fc[j]);
        pc += mbcnt(bc[j]);
        cA += (uint32_t)__popcll(__ballot(fa[j]));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (fc[j]) {
          const uint2 rec = make_uint2(e0 + j, __float_as_uint(xs[j]));
          if (stage != nullptr && pc < STAGE_CAP)
            stage[pc] = rec;
          else
            put(pc, rec);
          ++pc;
        }
        cC += (uint32_t)__popcll(bc[j]);
      }
    }
  }
  if (stage != nullptr) {
    wave_fence();
    for (uint32_t i = lane; i < cC && i < STAGE_CAP; i += 64) put(i, stage[i]);
  }
  if (ZERO) {
    cz = wave_sum(cz);
    if (tk != 0u) {
      rp = wave_min_u32(rp);
      rn = wave_min_u32(rn);
    }
  }
  if (lane == 0) {
    P.cntA[lu] = cA;
    P.cntC[lu] = cC;
    if (ZERO) P.cntZ[lu] = cz;
    if (ZERO && tk != 0u) P.tsgn[lu] = min(rp, 0xFFFFu) | (min(rn, 0xFFFFu) << 16);
  }
}


// Pick the bin of a HIST_BINS histogram (LDS) holding the r-th largest key: returns the bin, leaves in
// r the rank inside that bin. sh needs >= 64 words.
template <int NT, int NB = HIST_BINS>
DEV uint32_t hist_pick(const uint32_t* hist, uint32_t& r, uint32_t* sh) {
  constexpr int BPT = NB / NT;
  const uint32_t t = threadIdx.x;
  uint32_t c[BPT];
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    c[j] = hist[t * BPT + j];
    s += c[j];
  }
  uint32_t total;
  const uint32_t ex = block_excl_scan<NT>(s, sh, total);
  const uint32_t above = total - ex - s;
  if (t == 0) {
    sh[40] = NONE;
    sh[41] = r;
  }
  __syncthreads();
  if (above < r && r <= above + s) {
    uint32_t acc = above;
    int b = (int)(t * BPT);
#pragma unroll
    for (int j = BPT - 1; j >= 0; --j) {
      if (acc + c[j] >= r) {
        b = (int)(t * BPT) + j;
        break;
      }
      acc += c[j];
    }
    sh[40] = (uint32_t)b;
    sh[41] = r - acc;
  }
  __syncthreads();
  const uint32_t b = sh[40];
  r = sh[41];
  __syncthreads();
  return b;
}

// hist_pick for two ranks at once (r1, r2; 0 = not wanted): ONE block scan of the bins instead of two.
// Returns the bins in b1 / b2 (NONE when not wanted) and the ranks inside them in q1 / q2. sh needs >= 64 words
// (slots 40-43).
template <int NT, int NB = HIST_BINS>
DEV void hist_pick2(const uint32_t* hist, uint32_t r1, uint32_t r2, uint32_t& b1, uint32_t& b2, uint32_t& q1,
                    uint32_t& q2, uint32_t* sh) {
  constexpr int BPT = NB / NT;
  const uint32_t t = threadIdx.x;
  uint32_t c[BPT];
  uint32_t s = 0;
#pragma unroll
  for (int j = 0; j < BPT; ++j) {
    c[j] = hist[t * BPT + j];
    s += c[j];
  }
  uint32_t total;
  const uint32_t ex = block_excl_scan<NT>(s, sh, total);
  const uint32_t above = total - ex - s;
  if (t == 0) {
    sh[40] = NONE;
    sh[41] = NONE;
    sh[42] = 0u;
    sh[43] = 0u;
  }
  __syncthreads();
  const uint32_t rr[2] = {r1, r2};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const uint32_t r = rr[q];
    if (r != 0 && above < r && r <= above + s) {
      uint32_t acc = above;
      int b = (int)(t * BPT);
#pragma unroll
      for (int j = BPT - 1; j >= 0; --j) {
        if (acc + c[j] >= r) {
          b = (int)(t * BPT) + j;
          break;
        }
        acc += c[j];
      }
      sh[40 + q] = (uint32_t)b;
      sh[42 + q] = r - acc;
    }
  }
  __syncthreads();
  b1 = sh[40];
  b2 = sh[41];
  q1 = sh[42];
  q2 = sh[43];
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// small segments (n <= SMALL_MAX): one 256-thread block, values in LDS, exact radix select, ordered
// compaction, min/max, codes. Runs as its own kernel (k_small) on the plan's side stream, concurrently
// with k_sample / k_scan, so its latency hides under the HBM streaming.
// ------------------------------------------------------------------------------------------------
template <bool DELTA, bool RAW, int NT = BLOCK>
DEV void small_encode(const Params& P, uint32_t si, float* vals, uint32_t* hist, uint32_t* sh) {
  const uint32_t t = threadIdx.x;
  const uint32_t s = P.small_list[si];
  const SegDev sd = P.ssegs[si];  // (the same load round as s)
  const float* xs = seg_in(P, s, sd.in_off);
  const float* bs = DELTA ? P.base + sd.in_off : xs;
  const uint32_t n = sd.n, k = sd.k;
  STAMP(P, s, 2);  // (slots 2-7: small segments; k_select uses 0, 1, 10-12 of the large segments' rows)
  if (n == 0) {
    if (t == 0) {
      P.mn[s] = 0.0f;
      P.scale[s] = 0.0f;
    }
    return;
  }
  for (uint32_t i = t * 4; i < n; i += NT * 4) {
    if (i + 3 < n) {
      const float4 v = load_x4p<DELTA>(xs + i, bs + i);
      vals[i + 0] = v.x;
      vals[i + 1] = v.y;
      vals[i + 2] = v.z;
      vals[i + 3] = v.w;
    } else {
      for (uint32_t j = i; j < n; ++j) vals[j] = load_x1p<DELTA>(xs + j, bs + j);
    }
  }
  __syncthreads();
  STAMP(P, s, 3);
  uint32_t rt = k;
  const uint32_t T = block_select<NT>(
      [&](auto&& f) {
        for (uint32_t i = t; i < n; i += NT) f(fkey(vals[i]));
      },
      0u, KEY_MAX, rt, hist, sh);
  STAMP(P, s, 4);

  // ordered ownership: thread t owns the contiguous range [b0, b1); the first rt ties are kept
  const uint32_t E = (n + NT - 1) / NT;
  const uint32_t b0 = min(n, t * E), b1 = min(n, b0 + E);
  uint32_t gt = 0, eq = 0;
  for (uint32_t i = b0; i < b1; ++i) {
    const uint32_t key = fkey(vals[i]);
    gt += key > T;
    eq += key == T;
  }
  uint32_t eqtot;
  const uint32_t eqpre = block_excl_scan<NT>(eq, sh, eqtot);
  const uint32_t quota = min(eq, rt - umin_opaque(rt, eqpre));
  uint32_t seltot;
  const uint32_t opre = block_excl_scan<NT>(gt + quota, sh, seltot);
  STAMP(P, s, 5);

  float mn = 0.0f, scale = 0.0f;
  if (!RAW) {
    float a = qnan(), b = qnan();
    uint32_t eqseen = 0;
    for (uint32_t i = b0; i < b1; ++i) {
      const float x = vals[i];
      const uint32_t key = fkey(x);
      const bool sel = key > T || (key == T && eqseen++ < quota);
      if (sel) {
        a = fmin_nan(a, x);
        b = fmax_nan(b, x);
      }
    }
    block_minmax<NT>(a, b, reinterpret_cast<float*>(sh));
    codec_range(a, b, P.levels, mn, scale);
  }
  STAMP(P, s, 6);
  if (t == 0) {
    P.mn[s] = mn;
    P.scale[s] = scale;
    if (P.ustart_out != nullptr) P.ustart_out[sd.unit_begin] = 0u;  // (n <= SMALL_MAX < UNIT: one unit)
  }
  uint64_t o = sd.out_off + opre;
  uint32_t eqseen = 0;
  for (uint32_t i = b0; i < b1; ++i) {
    const float x = vals[i];
    const uint32_t key = fkey(x);
    const bool sel = key > T || (key == T && eqseen++ < quota);
    if (sel) {
      P.idx[o] = (int32_t)i;
      store_val<RAW>(P, o, x, mn, scale);
      ++o;
    }
  }
  STAMP(P, s, 7);
}

template <bool DELTA, bool RAW>
__global__ __launch_bounds__(BLOCK) void k_small(Params P) {
  __shared__ __attribute__((aligned(16))) float vals[SMALL_MAX];
  __shared__ uint32_t hist[HIST_BINS];
  __shared__ uint32_t sh[64];
  small_encode<DELTA, RAW>(P, blockIdx.x, vals, hist, sh);
}

// ------------------------------------------------------------------------------------------------
// k_sample: per large segment, sampled thresholds [T_lo, T_hi] for every unit of the segment
// ------------------------------------------------------------------------------------------------
template <bool DELTA, int NT = BLOCK>
DEV void sample_segment(const Params& P, uint32_t li, uint32_t* hist, uint32_t* sh) {
  constexpr uint32_t RPI = NT / 4;                   // runs per load batch (4 threads per 16-element run)
  constexpr uint32_t MAXIT = SAMPLE_MAX / 16 / RPI;  // load batches per thread
  const uint32_t t = threadIdx.x;
  STAMP(P, li, 16);  // (slots 16-19: k_sample, 20-21: k_ghist, 22-24: k_gwin of the segment's last group block)
  const uint32_t s = P.large_list[li];
  const SegDev sd = P.lsegs[li];  // (the same load round as s: no dependent segment-table lookup)
  const float* xs = seg_in(P, s, sd.in_off);
  const float* bs = DELTA ? P.base + sd.in_off : xs;
  const uint32_t n = sd.n, k = sd.k;
  // R runs of 16 contiguous elements, one per stratum of n / R elements, jittered inside it.
  uint32_t R = n / 512;
  R = R < 64 ? 64 : (R > SAMPLE_MAX / 16 ? SAMPLE_MAX / 16 : R);
  R &= ~63u;
  const uint32_t m = R * 16;
  const uint32_t stride = n / R;  // >= 16 because n > small_max >= 1024
  const uint32_t room = stride - 16;
  // The sampled keys stay in registers (4 per batch per thread): all loads in flight at once, and with
  // 8 KB of LDS per block (histogram only) twice as many sample blocks fit a CU as with an LDS key copy.
  uint32_t kk[MAXIT][4];
  uint32_t okm = 0;  // bit it: this thread's batch-it run exists (R is a multiple of 64, not of RPI)
#pragma unroll
  for (uint32_t it = 0; it < MAXIT; ++it) {
    const uint32_t r0 = it * RPI + (t >> 2), q = t & 3;
    okm |= (uint32_t)(r0 < R) << it;
    const uint32_t run = r0 < R ? r0 : R - 1;
    uint32_t start = run * stride + hash32(run * 0x9E3779B9u ^ (s + 1u) * 0x85EBCA6Bu) % (room + 1u);
    start &= ~3u;
    const float4 v = load_x4p<DELTA>(xs + start + q * 4, bs + start + q * 4);
    kk[it][0] = fkey(v.x);
    kk[it][1] = fkey(v.y);
    kk[it][2] = fkey(v.z);
    kk[it][3] = fkey(v.w);
  }
  // Expected sample rank of the k-th key, widened by a margin that assumes partially correlated runs.
  const double p = (double)k / (double)n;
  const double se = p * (double)m;
  const double d = 6.0 * sqrt(se) + 8.0;
  const double rlo = ceil(se + d), rhi = floor(se - d);
  // One histogram pass over the sample's own key range; thresholds are bin EDGES taken outward (lower
  // edge for T_lo, upper edge for T_hi), which only widens the bracket.
  if (t == 0) {
    sh[44] = KEY_MAX;
    sh[45] = 0u;
  }
  for (uint32_t i = t; i < HIST_BINS; i += NT) hist[i] = 0;
  __syncthreads();
  uint32_t kmn = KEY_MAX, kmx = 0;
#pragma unroll
  for (uint32_t it = 0; it < MAXIT; ++it) {
    if ((okm >> it) & 1u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        kmn = min(kmn, kk[it][j]);
        kmx = max(kmx, kk[it][j]);
      }
    }
  }
  kmn = wave_min_u32(kmn);
  kmx = wave_max_u32(kmx);
  if (lane_id() == 0) {
    atomicMin(&sh[44], kmn);
    atomicMax(&sh[45], kmx);
  }
  __syncthreads();
  STAMP(P, li, 17);
  const uint32_t kmin = sh[44], kmax = sh[45];
  const int shift = band_shift(kmin, kmax);
#pragma unroll
  for (uint32_t it = 0; it < MAXIT; ++it) {
    if ((okm >> it) & 1u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) atomicAdd(&hist[(kk[it][j] - kmin) >> shift], 1u);
    }
  }
  __syncthreads();
  uint32_t tlo = 0u, thi = KEY_MAX;
  uint32_t blo = 0, bhi = 0, qlo = 0, qhi = 0;  // both bracket bins (and ranks inside) from one scan of the histogram
  // (a sample too small for an upper margin, rhi < 1, leaves T_hi open; the top sample's bin is still picked, for the
  // tie test below)
  hist_pick2<NT>(hist, rlo < (double)m ? (uint32_t)rlo : 0u, rhi >= 1.0 ? (uint32_t)rhi : 1u, blo, bhi, qlo, qhi, sh);
  if (rlo < (double)m) tlo = kmin + (blo << shift);
  if (rhi >= 1.0) {
    const uint64_t edge = (uint64_t)kmin + (((uint64_t)bhi + 1) << shift) - 1;
    thi = (uint32_t)min<uint64_t>(edge, kmax);
  }
  bool tie = false;
  const uint32_t mw = rlo < (double)m ? (uint32_t)rlo - (rhi >= 1.0 ? (uint32_t)rhi : 1u) : 0u;  // margin width (ranks)
  if (rlo < (double)m && (blo == bhi || hist[blo] >= mw)) {
    // The sampled keys are concentrated where the bracket lies: both bracket ranks in ONE bin, or the lower rank's bin
    // holding at least the margin's width of samples (continuous data spreads the margin's ~120 ranks over several
    // bins, each holding a few). Refine inside the bin, 11 bits per pass: while the two ranks share a sub-bin (or for
    // the lower rank alone), down to single keys. Two ranks that part: the bracket is their sub-bins' outward edges.
    // Otherwise the lower rank's key K is exact, and a K repeated in the sample (the margin's quarter, >= 8 samples)
    // is a heavy tie: tie mode (T_lo = K | TIE_FLAG; both ranks on K: T_hi = K too). A K seen fewer times is the
    // lower edge itself.
    const bool two = blo == bhi;
    uint32_t base = kmin + (blo << shift), cK = hist[blo];
    int sft = shift;
    bool split = false;
    __syncthreads();  // (every thread has read hist[blo] before the first refinement clears it)
    while (sft > 0) {
      const int ns = sft > 11 ? sft - 11 : 0;
      const uint32_t top = base + ((1u << sft) - 1u);  // (no wrap: the bin lies inside [kmin, kmax + 2^shift))
      for (uint32_t i = t; i < HIST_BINS; i += NT) hist[i] = 0;
      __syncthreads();
#pragma unroll
      for (uint32_t it = 0; it < MAXIT; ++it) {
        if ((okm >> it) & 1u) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (kk[it][j] >= base && kk[it][j] <= top) atomicAdd(&hist[(kk[it][j] - base) >> ns], 1u);
        }
      }
      __syncthreads();
      uint32_t b1, b2;
      hist_pick2<NT>(hist, qlo, two ? qhi : 0u, b1, b2, qlo, qhi, sh);
      if (two && b1 != b2) {
        tlo = base + (b1 << ns);
        if (rhi >= 1.0) thi = min<uint64_t>((uint64_t)base + (((uint64_t)b2 + 1) << ns) - 1, kmax);
        split = true;
        break;
      }
      cK = hist[b1];
      __syncthreads();
      base += b1 << ns;
      sft = ns;
    }
    if (!split) {
      if (base != 0u && (two || cK >= max(8u, mw / 4u))) {
        tie = true;
        tlo = base | TIE_FLAG;
        if (two) thi = base;
      } else {
        tlo = base;  // (base 0: the plain tlo == 0 bracket, tie mode at key 0 already)
        if (two && rhi >= 1.0) thi = base;
      }
    }
  }
  STAMP(P, li, 18);
  const uint32_t nu = sd.unit_end - sd.unit_begin;
  // the band histograms' upper bound (see below)
  const uint32_t hh = tie ? max(tlo & KEY_MAX, min(thi, kmax)) : max(tlo, min(thi, kmax));
  for (uint32_t i = t; i < nu; i += NT) {
    P.tlo[sd.lu_begin + i] = tlo;
    P.thi[sd.lu_begin + i] = thi;
  }
  // The band histograms of the parallel select span [T_lo, min(T_hi, max sampled key)] (keys above go
  // to the last bin): with T_hi = KEY_MAX a full-range histogram would be too coarse.
  if (t == 0) {
    P.shhi[li] = hh;
    P.status[s] = 0;
  }
  STAMP(P, li, 19);
}

template <bool DELTA, bool RAW, int NT>
__global__ __launch_bounds__(NT) void k_sample(Params P) {
  __shared__ uint32_t hist[HIST_BINS];
  __shared__ uint32_t sh[64];
  sample_segment<DELTA, NT>(P, blockIdx.x, hist, sh);
}

// k_presel (batch plans below the fork class): the samplers (blocks [0, n_large)) and the small segments (blocks
// after them) as one launch — both latency-bound, they run side by side ahead of k_scan, which then streams large
// units only (small segments inside a batch's k_scan held its first blocks and a 25 KB LDS arena: C2 as 2
// sub-batches streamed at ~2.3 TB/s). Latency-bound plans launch k_sample and k_scan<WITH_SMALL> instead.
template <bool DELTA, bool RAW>
__global__ __launch_bounds__(BLOCK) void k_presel(Params P) {
  __shared__ __attribute__((aligned(16))) uint8_t arena[(SMALL_MAX + HIST_BINS + 64) * 4];
  uint32_t* hist = reinterpret_cast<uint32_t*>(arena) + SMALL_MAX;
  if (blockIdx.x < P.n_large) {
    sample_segment<DELTA>(P, blockIdx.x, hist, hist + HIST_BINS);
  } else {
    small_encode<DELTA, RAW>(P, blockIdx.x - P.n_large, reinterpret_cast<float*>(arena), hist, hist + HIST_BINS);
  }
}

// k_scan: streams the large units, one wave each. (WITH_SMALL: blocks [0, scan_small) first encode the
// small segments — the latency-bound plans' instantiation; batch plans launch the one without, their small
// segments in k_presel beside the samplers or, in the fork class, in k_small on the side stream.)
// (WPE / NB: launch-bound blocks per CU and load batches; the latency-bound plans' instantiation, the one
// WITH_SMALL, takes its own — nothing streams beside it)
template <bool DELTA, bool RAW, bool WITH_SMALL, int WPE = SCAN_WPE, int NB = SCAN_NB, int NTS = BLOCK,
          uint32_t SCAP = SMALL_MAX>
__global__ __launch_bounds__(NTS, WPE) void k_scan(Params P) {
  // one LDS arena: candidate staging (NTS / 64 x STAGE_CAP records) or a small segment's values + histogram
  // (WITH_SMALL only: without it the block needs 16 KB of LDS instead of 24.8 KB)
  constexpr uint32_t NWS = NTS / 64;
  // (SCAP: the plan's small-segment limit, <= SMALL_MAX — 1024 by default for latency-bound plans, whose
  // arena then leaves room for a seventh block per CU)
  constexpr size_t SMALL_BYTES = WITH_SMALL ? (SCAP + HIST_BINS + 64) * 4 : 0;
  constexpr size_t STAGE_BYTES = NWS * STAGE_CAP * sizeof(uint2);
  __shared__ __attribute__((aligned(16))) uint8_t arena[SMALL_BYTES > STAGE_BYTES ? SMALL_BYTES : STAGE_BYTES];
  if (WITH_SMALL && blockIdx.x < P.scan_small) {
    float* vals = reinterpret_cast<float*>(arena);
    uint32_t* hist = reinterpret_cast<uint32_t*>(arena) + SCAP;
    small_encode<DELTA, RAW, NTS>(P, blockIdx.x, vals, hist, hist + HIST_BINS);
    return;
  }
  uint2* stage = reinterpret_cast<uint2*>(arena);
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t lu = ((!WITH_SMALL ? xcd_block(blockIdx.x) : blockIdx.x) - P.scan_small) * NWS + wv;
  if (lu >= P.n_lunits) return;
  const UnitDev L = P.lunits[lu];
  // delta: 4 load batches (32 float4 in flight spill)
  const uint32_t tlo = P.tlo[lu], thi = P.thi[lu];
  if (tlo == 0 || (tlo & TIE_FLAG)) {  // tie mode (wave-uniform: one bracket per segment)
    if (L.len == UNIT || tlo != 0)  // (K > 0: a partial unit's loads past len read key 0 < K + 1, never counted)
      scan_unit<DELTA, DELTA ? 4 : NB, false, true>(P, lu, L, tlo, thi, stage + wv * STAGE_CAP);
    else
      scan_unit<DELTA, DELTA ? 4 : NB, true, true>(P, lu, L, tlo, thi, stage + wv * STAGE_CAP);
  } else if (L.len == UNIT || tlo > 0)
    scan_unit<DELTA, DELTA ? 4 : NB, false>(P, lu, L, tlo, thi, stage + wv * STAGE_CAP);
  else
    scan_unit<DELTA, DELTA ? 4 : NB, true>(P, lu, L, tlo, thi, stage + wv * STAGE_CAP);
}

// ------------------------------------------------------------------------------------------------
// per-segment select (k_select: one SEL_NT-thread block per large segment)
// ------------------------------------------------------------------------------------------------
// Exclusive prefix of cnt[0..cn) into upre[0..cn] (upre[cn] = total). Barriers inside.
template <int NT>
DEV uint32_t chunk_prefix(const uint32_t* cnt, uint32_t cn, uint32_t cap, uint32_t* upre, uint32_t* sh) {
  const uint32_t t = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t c0 = 0; c0 < cn; c0 += NT) {
    const uint32_t i = c0 + t;
    const uint32_t v = i < cn ? min(cnt[i], cap) : 0u;  // stored records only
    uint32_t tot;
    const uint32_t ex = block_excl_scan<NT>(v, sh, tot);
    if (i < cn) upre[i] = carry + ex;
    carry += tot;
  }
  if (t == 0) upre[cn] = carry;
  __syncthreads();
  return carry;
}


// The records of a unit past its first two rows (n > 128: plans above ratio ~0.02), TAIL_ROWS rows of 64 per load
// round instead of one dependent round per row (C3 at ratio 0.1: a ~450-record unit took 6 rounds).
constexpr uint32_t TAIL_ROWS = 4;
// (k_emit batches its record rows the same way only in plans above HIGH_RATIO: at ratio 0.01 almost every unit's records
// fit the preloaded first row, and the batched loop measured 1.5 % slower on C3 — 0.600 vs 0.592 ms per step; C3 at
// ratio 0.1: 0.922 vs 0.982 ms with it, profiles/r05_ab.txt)
constexpr double HIGH_RATIO = 0.02;
template <class F>
DEV void tail_rows(const uint32_t* R, uint32_t n, uint32_t u, F&& f, uint32_t from = 128) {
  constexpr uint32_t TR = TAIL_ROWS;
  const uint32_t lane = lane_id();
  for (uint32_t i0 = from; i0 < n; i0 += 64 * TR) {
    uint32_t x[TR];
#pragma unroll
    for (uint32_t b = 0; b < TR; ++b)
      if (i0 + b * 64 < n) x[b] = R[min(i0 + b * 64 + lane, n - 1)];  // (wave-uniform guard)
#pragma unroll
    for (uint32_t b = 0; b < TR; ++b)
      if (i0 + b * 64 < n) f(__uint_as_float(x[b]), i0 + b * 64 + lane < n, u);
  }
}

// Wave w owns the units whose first record index (upre[u]) lies in [w*total/NW, (w+1)*total/NW):
// contiguous unit ranges balanced by record count, so segment order = (wave, unit, lane) order. A wave
// reads one unit at a time from its contiguous region (coalesced, trivial addressing, the unit is
// wave-uniform so per-unit counts are ballot popcounts), G units per batch with 2 records per lane per
// unit in flight. f(x, valid, u) is called by ALL lanes (ballots allowed); fend(u) after each unit.
// RM: record rows per unit in the batch's load round (2; 8 in batch plans above HIGH_RATIO, where a unit holds ~450
// records: all of them in that one round instead of 1 + 2 rounds per unit — C3 at ratio 0.1: 0.908-0.920 vs
// 0.925-0.927 ms; the sweeps there are bound by the HBM traffic the other sub-batch's streams leave them)
template <int NW, int G, int RM = 2, class F, class FE>
DEV void unit_sweep(const uint32_t* cand, uint32_t stride, uint32_t lu0, const uint32_t* upre, uint32_t cn,
                    uint32_t total, F&& f, FE&& fend) {
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  const uint32_t J0 = (uint32_t)((uint64_t)total * w / NW), J1 = (uint32_t)((uint64_t)total * (w + 1) / NW);
  auto lower = [&](uint32_t key) {  // first u in [0, cn] with upre[u] >= key
    uint32_t lo = 0, hi = cn;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (upre[mid] < key)
        lo = mid + 1;
      else
        hi = mid;
    }
    return lo;
  };
  const uint32_t U0 = w == 0 ? 0u : lower(J0);
  const uint32_t U1 = w == NW - 1 ? cn : lower(J1);
  for (uint32_t u = U0; u < U1; u += G) {
    uint32_t x[G][RM], nn[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint32_t uu = min(u + g, U1 - 1);
      const uint32_t n = upre[uu + 1] - upre[uu];
      const uint32_t last = n ? n - 1 : 0u;  // region slot 0 always exists; read it when n == 0
      const uint32_t* R = cand + (uint64_t)(lu0 + uu) * stride;
      nn[g] = n;
#pragma unroll
      for (int r = 0; r < RM; ++r)
        if (r < 2 || 64u * r < n) x[g][r] = R[min(lane + 64u * r, last)];  // (rows past 2: wave-uniform guard)
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (u + g < U1) {
        const uint32_t uu = u + g, n = nn[g];
        f(__uint_as_float(x[g][0]), lane < n, uu);
#pragma unroll
        for (int r = 1; r < RM; ++r)
          if (n > 64u * r) f(__uint_as_float(x[g][r]), lane + 64u * r < n, uu);
        if (n > 64u * RM) tail_rows(cand + (uint64_t)(lu0 + uu) * stride, n, uu, f, 64u * RM);
        fend(uu);
      }
    }
  }
}

// The same prefix from counts already in registers (thread i < cn holds unit i's count, cn <= NT): the
// loads were issued with the caller's other loads of the same round.
template <int NT>
DEV uint32_t reg_prefix(uint32_t c, uint32_t cn, uint32_t* upre, uint32_t* sh) {
  const uint32_t t = threadIdx.x;
  uint32_t tot;
  const uint32_t ex = block_excl_scan<NT>(t < cn ? c : 0u, sh, tot);
  if (t < cn) upre[t] = ex;
  if (t == 0) upre[cn] = tot;
  __syncthreads();
  return tot;
}

// A group's records swept by the block's waves balanced by record count (unit_sweep): the counts and a block
// prefix come first, then the record loads — batch plans, where the select kernels run beside the other
// sub-batch's streaming waves (the speculative sweep below measured slower there: C3 0.617-0.636 vs 0.600-0.604 ms)
template <int NT, int G = GSWEEP, int RM = 2>
struct BalancedSweep {
  uint32_t* upre;
  uint32_t total, cn;
  DEV void load(const Params& P, uint32_t lu0, uint32_t units, uint32_t* upre_, uint32_t* sh) {
    upre = upre_;
    cn = units;
    const uint32_t c = threadIdx.x < units ? min(P.cntC[lu0 + threadIdx.x], P.ccap) : 0u;
    total = reg_prefix<NT>(c, units, upre, sh);  // barriers inside
  }
  template <class F, class FE>
  DEV void run(const Params& P, uint32_t lu0, F&& f, FE&& fend) const {
    unit_sweep<NT / 64, G, RM>(P.cval, P.ccap, lu0, upre, cn, total, f, fend);
  }
};

// A group's records swept by a block WITHOUT waiting for the units' counts first: wave w owns the UPW
// consecutive units [w * UPW, (w + 1) * UPW) of the group (index order = wave order) and loads their counts
// and the first two 64-record rows of every unit in ONE round, speculatively (slots past a unit's count hold
// stale words, never used; ccap >= 128). unit_sweep instead balances the waves by record count, which needs
// the counts and a block prefix before the first record load — one more dependent round on the select chain.
template <uint32_t UPW>
struct SpecSweep {
  uint32_t x0[UPW], x1[UPW], n;  // lane g < UPW: unit g's stored-record count
  uint32_t u0, cn;
  DEV void load(const Params& P, uint32_t lu0, uint32_t units, uint32_t*, uint32_t*) {
    const uint32_t lane = lane_id();
    u0 = (threadIdx.x >> 6) * UPW;
    cn = units;
    const uint32_t uc = min(u0 + min(lane, UPW - 1), units - 1);
    const uint32_t nr = P.cntC[lu0 + uc];
#pragma unroll
    for (uint32_t g = 0; g < UPW; ++g) {
      const uint32_t* R = P.cval + (uint64_t)(lu0 + min(u0 + g, units - 1)) * P.ccap;
      x0[g] = R[lane];
      x1[g] = R[lane + 64];
    }
    n = (lane < UPW && u0 + lane < units) ? min(nr, P.ccap) : 0u;
  }
  // f(x, valid, u) for every lane (ballots allowed), fend(u) after each unit; u = unit index in the group
  template <class F, class FE>
  DEV void run(const Params& P, uint32_t lu0, F&& f, FE&& fend) const {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t g = 0; g < UPW; ++g) {
      const uint32_t u = u0 + g;
      if (u < cn) {
        const uint32_t nn = (uint32_t)__builtin_amdgcn_readlane((int)n, (int)g);
        f(__uint_as_float(x0[g]), lane < nn, u);
        if (nn > 64) f(__uint_as_float(x1[g]), lane + 64 < nn, u);
        if (nn > 128) tail_rows(P.cval + (uint64_t)(lu0 + u) * P.ccap, nn, u, f);
        fend(u);
      }
    }
  }
};

// LDS scratch of the segment select (k_select, and the SELECT role of the one-launch encode, whose LDS
// must stay <= 32 KB so five streaming blocks still fit a CU): 28.3 KB
constexpr uint32_t WLIST = 1024;  // in-window entries the fast path can hold
constexpr uint32_t SELECT_SPEC = 64u;  // k_select: speculatively gathered slots per group window list (one update: 64 -> 0.0811 ms per
                                       // step, 16 -> 0.0830, 8 -> 0.0838: longer lists otherwise cost a dependent round)
constexpr int SEL_HB = 1024;      // bins of the select's radix histograms
struct SelSmem {
  uint32_t hist[SEL_HB];
  uint32_t upre[UCAP + 1];
  uint32_t ge[UCAP];   // per unit of the chunk: count above T* (bits 0-15) | count equal T* (bits 16-31)
  uint2 lst[WLIST];    // in-window entries {value bits, unit}, all waves concatenated = index order
  uint32_t wcnt[SEL_NT_LAT / 64];
  uint32_t sh[64];
  float shf[2 * (SEL_NT_LAT / 64)];
};
static_assert(sizeof(SelSmem) <= 29 * 1024, "select LDS budget");

// Generic path: radix select over all candidates (1-3 coalesced sweeps) + a counts sweep; handles any
// number of ties and segments of any size (units in chunks of UCAP).
template <int NT>
DEV void select_generic(const Params& P, uint32_t lb, uint32_t nu, uint32_t tlo, uint32_t thi, uint32_t r,
                        SelSmem& S, uint32_t& T_out, uint32_t& rt_out, uint32_t& fp, uint32_t& fn, float& gmn,
                        float& gmx) {
  constexpr int NW = NT / 64;
  const uint32_t t = threadIdx.x, lane = lane_id(), wv = t >> 6;
  uint32_t rt = r;
  auto forC = [&](auto&& f) {
    for (uint32_t c0 = 0; c0 < nu; c0 += UCAP) {
      const uint32_t cn = min(UCAP, nu - c0);
      const uint32_t total = chunk_prefix<NT>(P.cntC + lb + c0, cn, P.ccap, S.upre, S.sh);
      unit_sweep<NW, 4>(
          P.cval, P.ccap, lb + c0, S.upre, cn, total,
          [&](float x, bool valid, uint32_t) {
            if (valid) f(fkey(x));
          },
          [&](uint32_t) {});
      __syncthreads();
    }
  };
  const uint32_t T = rt == 0 ? thi : block_select<NT, SEL_HB>(forC, tlo, thi, rt, S.hist, S.sh);

  // counts sweep: per-unit gt/eq, segment-wide tie rank of the first positive / negative tie, min/max
  // of the values with key > T (all of them are kept).
  float lmn = qnan(), lmx = qnan();
  uint32_t carry_eq = 0;
  if (t == 0) {
    S.sh[42] = NONE;
    S.sh[43] = NONE;
  }
  for (uint32_t c0 = 0; c0 < nu; c0 += UCAP) {
    const uint32_t cn = min(UCAP, nu - c0);
    for (uint32_t i = t; i < cn; i += NT) S.ge[i] = 0;
    const uint32_t total = chunk_prefix<NT>(P.cntC + lb + c0, cn, P.ccap, S.upre, S.sh);
    uint32_t weq = 0, wfp = NONE, wfn = NONE, ug = 0, ue = 0;  // wave-uniform
    unit_sweep<NW, 4>(
        P.cval, P.ccap, lb + c0, S.upre, cn, total,
        [&](float x, bool valid, uint32_t) {
          const uint32_t key = fkey(x);
          const bool g = valid && key > T;
          const bool e = valid && key == T;
          ug += (uint32_t)__popcll(__ballot(g));
          const float xg = g ? x : qnan();
          lmn = fmin_nan(lmn, xg);
          lmx = fmax_nan(lmx, xg);
          const uint64_t eb = __ballot(e);
          if (eb) {
            const bool neg = (__float_as_uint(x) >> 31) != 0;
            const uint64_t pm = __ballot(e && !neg), nm = __ballot(e && neg);
            if (wfp == NONE && pm) wfp = weq + (uint32_t)__popcll(eb & ((1ull << (__ffsll((long long)pm) - 1)) - 1ull));
            if (wfn == NONE && nm) wfn = weq + (uint32_t)__popcll(eb & ((1ull << (__ffsll((long long)nm) - 1)) - 1ull));
            weq += (uint32_t)__popcll(eb);
            ue += (uint32_t)__popcll(eb);
          }
        },
        [&](uint32_t u) {
          if (lane == 0) S.ge[u] = ug | (ue << 16);
          ug = ue = 0;
        });
    if (lane == 0) S.wcnt[wv] = weq;
    __syncthreads();
    uint32_t wpre = carry_eq, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const uint32_t c = S.wcnt[i];
      if ((uint32_t)i < wv) wpre += c;
      tot += c;
    }
    if (lane == 0 && wfp != NONE) atomicMin(&S.sh[42], wpre + wfp);
    if (lane == 0 && wfn != NONE) atomicMin(&S.sh[43], wpre + wfn);
    carry_eq += tot;
    __syncthreads();
    for (uint32_t i = t; i < cn; i += NT) {
      P.gtC[lb + c0 + i] = S.ge[i] & 0xFFFFu;
      P.eqC[lb + c0 + i] = S.ge[i] >> 16;
    }
    __syncthreads();
  }
  T_out = T;
  rt_out = rt;
  fp = S.sh[42];
  fn = S.sh[43];
  gmn = lmn;
  gmx = lmx;
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// parallel select, fast path: groups of GU units of one large segment, one 256-thread block each
// ------------------------------------------------------------------------------------------------
// k_ghist: the group's HB2-bin histogram of the band keys [tlo, thi] -> ghist[group]. (A fused variant in
// which the segment's last-arriving group block ran segment_pick needed an agent-scope release fence in
// every block — an L2 writeback on gfx950 — and was ~100x slower; kernel boundaries are cheaper.)
template <int NT, bool SPEC, bool HR = false>
using GroupSweep = std::conditional_t<SPEC, SpecSweep<(GU + NT / 64 - 1) / (NT / 64)>,
                                      std::conditional_t<HR, BalancedSweep<NT, 2, 8>, BalancedSweep<NT>>>;

template <int NT, bool SPEC, bool HR>
DEV void group_hist(const Params& P, uint32_t gi, uint32_t* hist, uint32_t* upre, uint32_t* sh) {
  const uint4 G = P.groups[gi];  // x: large-segment index, y: first large unit, z: units, w: segment
  const uint32_t t = threadIdx.x;
  STAMP(P, G.x, 20);
  // one load round for everything that depends on G only: the band, and every unit's count and first
  // records (the histogram needs no index order, so no count prefix before the record loads)
  const uint32_t tlo = P.tlo[G.y] & KEY_MAX, thi = P.thi[G.y], hh = P.shhi[G.x];  // (tie mode K: band [K, K], empty)
  GroupSweep<NT, SPEC, HR> sw;
  for (uint32_t i = t; i < HB2; i += NT) hist[i] = 0;
  sw.load(P, G.y, G.z, upre, sh);
  __syncthreads();
  const Band band(tlo, thi, hh);
  sw.run(
      P, G.y,
      [&](float x, bool valid, uint32_t) {
        const uint32_t key = fkey(x);
        if (valid && key >= tlo && key <= thi) atomicAdd(&hist[band.bin(key)], 1u);
      },
      [&](uint32_t) {});
  __syncthreads();
  for (uint32_t i = t; i < HB2; i += NT) pst(P, P.ghist + (uint64_t)gi * HB2 + i, hist[i]);
  STAMP(P, G.x, 21);
}

// NT: 256 threads in batches, GHIST_NT_LAT in latency-bound plans (nothing streams beside the block); SPEC: the
// speculative group sweep (latency-bound plans)
template <int NT, bool SPEC, bool HR = false>  // HR: batch plans above HIGH_RATIO (8 record rows per unit per round)
__global__ __launch_bounds__(NT) void k_ghist(Params P) {
  __shared__ uint32_t hist[HB2];
  __shared__ uint32_t upre[GU + 1];
  __shared__ uint32_t sh[64];
  group_hist<NT, SPEC, HR>(P, blockIdx.x, hist, upre, sh);
}

// segment_pick: per large segment — validate the sampled bracket, sum the group histograms, pick the bin of
// the k-th key: {window lo, window hi, rank inside the window, 0}; {.., 1} routes the segment to the
// generic single-block path (bracket miss, nothing to take from B, huge segment, test flags). Every group
// block of the segment computes it (identically) at the start of k_gwin — cheaper than a launch of its
// own between k_ghist and k_gwin. Returned to every thread.
template <int NT = BLOCK>
DEV uint4 segment_pick(const Params& P, const SegDev& sd, const Band& band, bool tieseg, uint32_t* hist, uint32_t* sh) {
  const uint32_t t = threadIdx.x;
  const uint32_t lb = sd.lu_begin, nu = sd.unit_end - sd.unit_begin, k = sd.k;
  const uint32_t g0 = sd.g_begin, ng = (nu + GU - 1) / GU;
  // one load round: the group histograms (this thread's bins t and t + NT, up to 24 groups' loads in
  // flight) and the per-unit counts (up to 3 per thread) together
  static_assert(HB2 == 2 * NT || HB2 == NT, "one or two histogram bins per thread");
  constexpr bool TWO = HB2 == 2 * NT;
  constexpr uint32_t GB = 24, CB = 3;
  const bool zseg = tieseg;  // the scan counted this segment's keys equal to its tie key (cntZ; tie mode)
  uint32_t h0 = 0, h1 = 0, sa = 0, sc = 0, ov = 0, sz = 0;
  {
    uint32_t v0[GB], v1[GB], ca[CB], cc[CB], cz[CB];
#pragma unroll
    for (uint32_t j = 0; j < GB; ++j) {
      const uint64_t row = (uint64_t)(g0 + min(j, ng - 1)) * HB2;
      v0[j] = P.ghist[row + t];
      v1[j] = TWO ? P.ghist[row + NT + t] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < CB; ++j) {
      const uint32_t i = min(t + j * NT, nu - 1);
      cc[j] = P.cntC[lb + i];
      ca[j] = P.cntA[lb + i];
      cz[j] = P.cntZ[lb + i];  // (unconditional; used for a zero-bracket segment only)
    }
#pragma unroll
    for (uint32_t j = 0; j < GB; ++j) {
      h0 += j < ng ? v0[j] : 0u;
      h1 += j < ng ? v1[j] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < CB; ++j) {
      if (t + j * NT < nu) {
        sa += ca[j];
        sc += cc[j];
        sz += zseg ? cz[j] : 0u;
        ov += cc[j] > P.ccap ? 1u : 0u;
      }
    }
  }
  for (uint32_t g = GB; g < ng; g += 8) {  // segments of more than GB groups
    uint32_t v0[8], v1[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      const uint64_t row = (uint64_t)(g0 + min(g + j, ng - 1)) * HB2;
      v0[j] = P.ghist[row + t];
      v1[j] = TWO ? P.ghist[row + NT + t] : 0u;
    }
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
      h0 += g + j < ng ? v0[j] : 0u;
      h1 += g + j < ng ? v1[j] : 0u;
    }
  }
  for (uint32_t i = t + CB * NT; i < nu; i += NT) {
    const uint32_t c = P.cntC[lb + i];
    sa += P.cntA[lb + i];
    sc += c;
    sz += zseg ? P.cntZ[lb + i] : 0u;
    ov += c > P.ccap ? 1u : 0u;
  }
  hist[t] = h0;
  if (TWO) hist[NT + t] = h1;
  sa = block_sum<NT>(sa, sh);  // barriers inside (also publish hist)
  sc = block_sum<NT>(sc, sh);
  ov = block_sum<NT>(ov, sh);
  if (zseg) sz = block_sum<NT>(sz, sh);
  // (a unit that overflowed its record slots sends the segment to the raw-data path in segment_select)
  const bool forced = (P.flags & (COALAC_FLAG_FORCE_EXACT | COALAC_FLAG_GENERIC_SELECT)) || nu > UCAP || ov != 0;
  // the k-th key is the tie key K: every recorded key (all above K) is kept, and the first k - sc K-keys by index. The
  // window [1, 0] is empty: k_gwin counts every record as above it (per-unit kept counts) and takes their min / max
  if (!forced && zseg && sc < k && k - sc <= sz) return make_uint4(1u, 0u, k - sc, 2u);
  const bool generic = forced || !(sa < k && k <= sc);
  if (generic) return make_uint4(0u, 0u, 0u, 1u);
  __syncthreads();
  uint32_t r = k - sa;
  const uint32_t b = hist_pick<NT, HB2>(hist, r, sh);
  if (b == NONE) return make_uint4(0u, 0u, 0u, 1u);
  return make_uint4(band.wlo(b), band.whi(b), r, 0u);
}

// k_gwin: per group — per-unit counts of keys above the window (-> gtC), the group's in-window entries
// in index order (-> glist, count -> gcnt), min/max of the values above the window (-> gmm)
template <int NW = WAVES>
struct GwinSmemT {
  uint32_t upre[GU + 1];
  uint2 slots[NW][GCAP];
  uint32_t wcnt[NW];
  float shf[2 * NW];
};
using GwinSmem = GwinSmemT<WAVES>;

template <int NT, bool DELTA, bool RAW>
DEV void segment_select(const Params& P, uint32_t li, SelSmem& S);

// (sw: the group's counts and first records, loaded by the caller with its other loads)
template <int NT, class SW>
DEV void group_window(const Params& P, uint32_t gi, const uint4 G, const uint4 st, uint32_t lu_begin, const SW& sw,
                      GwinSmemT<NT / 64>& W_, uint32_t* sh) {
  constexpr int NW = NT / 64;
  auto& slots = W_.slots;
  uint32_t* wcnt = W_.wcnt;
  float* shf = W_.shf;
  const uint32_t t = threadIdx.x, lane = lane_id(), wv = t >> 6;
  const uint32_t wlo = st.x, whi = st.y;
  const uint32_t useg0 = G.y - lu_begin;  // unit index (within the segment) of the group's first unit
  uint32_t wc = 0, ug = 0;
  float lmn = qnan(), lmx = qnan();
  sw.run(
      P, G.y,
      [&](float x, bool valid, uint32_t u) {
        const uint32_t key = fkey(x);
        const bool g = valid && key > whi;
        const bool in = valid && key >= wlo && key <= whi;
        ug += (uint32_t)__popcll(__ballot(g));
        const float xg = g ? x : qnan();
        lmn = fmin_nan(lmn, xg);
        lmx = fmax_nan(lmx, xg);
        const uint64_t im = __ballot(in);
        if (im) {
          const uint32_t pos = wc + mbcnt(im);
          if (in && pos < GCAP) slots[wv][pos] = make_uint2(__float_as_uint(x), useg0 + u);
          wc += (uint32_t)__popcll(im);
        }
      },
      [&](uint32_t u) {
        if (lane == 0) {
          pst(P, P.gtC + G.y + u, ug);
          pst(P, P.eqC + G.y + u, 0u);
        }
        ug = 0;
      });
  if (lane == 0) wcnt[wv] = wc;
  __syncthreads();
  uint32_t wpre = 0, W = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const uint32_t c = wcnt[i];
    if (i < (int)wv) wpre += c;
    W += c;
  }
  for (uint32_t q = lane; q < wc && q < GCAP; q += 64)
    if (wpre + q < GCAP) pst(P, P.glist + (uint64_t)gi * GCAP + wpre + q, slots[wv][q]);
  block_minmax<NT>(lmn, lmx, shf);
  if (t == 0) {
    pst(P, P.gcnt + gi, W);
    pst(P, P.gmm + 2 * gi, lmn);
    pst(P, P.gmm + 2 * gi + 1, lmx);
  }
}

template <int NT, bool SPEC, bool HR>
DEV void group_pick_window(const Params& P, uint32_t gi, GwinSmemT<NT / 64>& W, uint32_t* hist, uint32_t* sh) {
  // round 1: the group and its segment's geometry (gseg: {first large unit, units, k, first group}, so nothing
  // waits for a segment-table lookup); round 2: the band, the group's unit counts and first records
  // (SpecSweep), the segment's group histograms and unit counts — everything the block reads, in one round
  const uint4 G = P.groups[gi];
  const uint4 GS = P.gseg[gi];
  STAMP(P, G.x, 22);
  SegDev sd{};
  sd.lu_begin = GS.x;
  sd.unit_end = GS.y;
  sd.k = GS.z;
  sd.g_begin = GS.w;
  const uint32_t tlo = P.tlo[G.y], thi = P.thi[G.y], hh = P.shhi[G.x];
  GroupSweep<NT, SPEC, HR> sw;
  sw.load(P, G.y, G.z, W.upre, sh);
  const uint4 st = segment_pick<NT>(P, sd, Band(tlo & KEY_MAX, thi, hh), tlo == 0 || (tlo & TIE_FLAG), hist, sh);
  STAMP(P, G.x, 23);
  if (st.w == 0 || st.w == 2) group_window<NT>(P, gi, G, st, GS.x, sw, W, sh);
  if (threadIdx.x == 0 && G.y == GS.x) {  // the segment's first group
    uint2* ss = reinterpret_cast<uint2*>(P.sstate + G.x);
    pst(P, ss, make_uint2(st.x, st.y));
    pst(P, ss + 1, make_uint2(st.z, st.w));
  }
  STAMP(P, G.x, 24);
}

// NT: 256 threads in batches, GWIN_NT_LAT in latency-bound plans (nothing streams beside the block)
template <int NT, bool SPEC, bool HR = false>  // HR: as k_ghist
__global__ __launch_bounds__(NT) void k_gwin(Params P) {
  __shared__ GwinSmemT<NT / 64> W;
  __shared__ uint32_t hist[HB2];
  __shared__ uint32_t sh[64];
  group_pick_window<NT, SPEC, HR>(P, blockIdx.x, W, hist, sh);
}

// ------------------------------------------------------------------------------------------------
// raw-data path of a segment (bracket miss, COALAC_FLAG_FORCE_EXACT, or a unit with more candidates than
// its ccap record slots): T* from the raw keys (segment_select), per-unit counts from the raw data here,
// and the emit re-reads the raw data (emit_raw_unit). No candidate record is used.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t RAW_NB = 2u;  // load rounds per unit of a raw-data pass (round 5: 4 rounds of 4 float4 per lane)
// One wave's pass over a unit's raw data (row by row, index order): per element whether key > T and
// whether key == T, handed to f(row, j, x, gt, tie) for every lane (ballots allowed inside f).
template <bool DELTA, class F>
DEV void raw_unit_rows(const Params& P, const UnitDev& L, F&& f) {
  const uint32_t lane = lane_id();
  const float* xin = P.inptr != nullptr ? P.inptr[L.seg] + L.start : P.in + L.off;
  const __amdgpu_buffer_rsrc_t rin = unit_rsrc(xin, L.len);
  const __amdgpu_buffer_rsrc_t rbase = unit_rsrc(DELTA ? P.base + L.off : xin, L.len);
  for (uint32_t nb = 0; nb < RAW_NB; ++nb) {  // UNIT_IT / RAW_NB float4 per lane in flight
    constexpr uint32_t IT = UNIT_IT / RAW_NB;
    float4 v[IT];
#pragma unroll
    for (uint32_t i = 0; i < IT; ++i) v[i] = unit_load_x4<DELTA>(rin, rbase, ((nb * IT + i) * 64 + lane) * 16);
#pragma unroll
    for (uint32_t i = 0; i < IT; ++i) f(nb * IT + i, v[i]);
  }
}

// Per-unit counts above / equal to T of the raw segment -> gtC / eqC; min / max of the values above T; the
// segment-wide tie rank of the first positive and first negative tie (index order). Waves own contiguous
// unit ranges in order. Block-level: call from all threads.
template <int NT, bool DELTA>
DEV void raw_counts(const Params& P, uint32_t lb, uint32_t nu, uint32_t T, uint32_t* sh, uint32_t* wcnt,
                    uint32_t& fp, uint32_t& fn, float& gmn, float& gmx, uint32_t* ge) {
  constexpr int NW = NT / 64;
  const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
  const uint32_t u0 = (uint32_t)((uint64_t)nu * wv / NW), u1 = (uint32_t)((uint64_t)nu * (wv + 1) / NW);
  uint32_t weq = 0, wfp = NONE, wfn = NONE;
  float lmn = qnan(), lmx = qnan();
  for (uint32_t u = u0; u < u1; ++u) {
    const UnitDev L = P.lunits[lb + u];
    uint32_t ug = 0, ue = 0;
    raw_unit_rows<DELTA>(P, L, [&](uint32_t row, float4 v) {
      const float xs[4] = {v.x, v.y, v.z, v.w};
      const uint32_t e0 = (row * 64 + lane) * 4;
      uint32_t pre = 0, mine = 0;
      uint64_t tb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t key = fkey(xs[j]);
        const bool ok = e0 + j < L.len;
        const bool g = ok && key > T, e = ok && key == T;
        ug += (uint32_t)__popcll(__ballot(g));
        tb[j] = __ballot(e);
        pre += mbcnt(tb[j]);
        const float xg = g ? xs[j] : qnan();
        lmn = fmin_nan(lmn, xg);
        lmx = fmax_nan(lmx, xg);
      }
      // index order inside a row is (lane, j): a tie's rank = ties of lower lanes + earlier ties of its lane
      uint32_t rp = NONE, rn = NONE;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool e = ((tb[j] >> lane) & 1ull) != 0;
        if (e) {
          const bool neg = (__float_as_uint(xs[j]) >> 31) != 0;
          const uint32_t rank = weq + pre + mine;
          if (neg)
            rn = min(rn, rank);
          else
            rp = min(rp, rank);
          ++mine;
        }
      }
      wfp = min(wfp, wave_min_u32(rp));
      wfn = min(wfn, wave_min_u32(rn));
      const uint32_t rowt = (uint32_t)(__popcll(tb[0]) + __popcll(tb[1]) + __popcll(tb[2]) + __popcll(tb[3]));
      weq += rowt;
      ue += rowt;
    });
    if (lane == 0) {
      pst(P, P.gtC + lb + u, ug);
      pst(P, P.eqC + lb + u, ue);
      if (u < UCAP) ge[u] = ug | (ue << 16);  // (select_finish reads LDS: other threads own the unit there)
    }
  }
  // wave prefixes of the tie counts -> segment-wide ranks of the first positive / negative tie
  if (lane == 0) wcnt[wv] = weq;
  if (threadIdx.x == 0) {
    sh[42] = NONE;
    sh[43] = NONE;
  }
  __syncthreads();
  uint32_t wpre = 0;
  for (int i = 0; i < (int)wv; ++i) wpre += wcnt[i];
  if (lane == 0 && wfp != NONE) atomicMin(&sh[42], wpre + wfp);
  if (lane == 0 && wfn != NONE) atomicMin(&sh[43], wpre + wfn);
  __syncthreads();
  fp = sh[42];
  fn = sh[43];
  gmn = lmn;
  gmx = lmx;
  __syncthreads();
}

template <int NT>
DEV void window_resolve(SelSmem& S, uint32_t W, uint4 st, float lmn0, float lmx0, uint32_t& T_out, uint32_t& rt_out,
                        uint32_t& fp, uint32_t& fn, float& gmn, float& gmx);

// Fast-path resolution in k_select: gather the groups' in-window lists (group order = index order),
// find the exact key inside the window, apply the window entries to the per-unit counts. Returns false
// if a group's list overflowed (the caller then runs the generic path from scratch).
template <int NT>
DEV bool select_from_groups(const Params& P, const SegDev& sd, uint32_t lb, uint32_t nu, uint4 st, SelSmem& S,
                            uint32_t& T_out, uint32_t& rt_out, uint32_t& fp, uint32_t& fn, float& gmn, float& gmx) {
  const uint32_t t = threadIdx.x;
  const uint32_t g0 = sd.g_begin, ng = (nu + GU - 1) / GU;  // ng <= UCAP / GU = 64 <= NT
  // one load round: the groups' list lengths, min / max above the window, the first per-unit counts, and —
  // speculatively, before their lengths are known — the first SPEC slots of every group's in-window list (the
  // typical window share of a group fits; a longer list's remainder is loaded after the scan)
  constexpr uint32_t SPEC = SELECT_SPEC, SPT = (UCAP / GU) * SPEC / NT;
  static_assert((UCAP / GU) * SPEC % NT == 0, "speculative gather geometry");
  uint2 sv[SPT];
#pragma unroll
  for (uint32_t j = 0; j < SPT; ++j) {
    const uint32_t i = t + j * NT, g = i / SPEC;
    sv[j] = g < ng ? P.glist[(uint64_t)(g0 + g) * GCAP + i % SPEC] : make_uint2(0u, 0u);
  }
  const uint32_t c = t < ng ? P.gcnt[g0 + t] : 0u;
  const float gmn0 = t < ng ? P.gmm[2 * (g0 + t)] : qnan(), gmx0 = t < ng ? P.gmm[2 * (g0 + t) + 1] : qnan();
  constexpr uint32_t CB = 3;
  uint32_t gtc[CB];
#pragma unroll
  for (uint32_t j = 0; j < CB; ++j) gtc[j] = P.gtC[lb + min(t + j * NT, nu - 1)];
  uint32_t W;
  const uint32_t gpre = block_excl_scan<NT>(c, S.sh, W);
  const uint32_t over = block_sum<NT>(c > GCAP ? 1u : 0u, S.sh);
  if (over || W > WLIST) return false;
  // each group's entries go to its offset in the segment's list (group order = index order)
  if (t < ng) S.upre[t] = gpre;
  if (t == 0) S.upre[ng] = W;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < SPT; ++j) {
    const uint32_t i = t + j * NT, g = i / SPEC, slot = i % SPEC;
    if (g < ng && S.upre[g] + slot < S.upre[g + 1]) S.lst[S.upre[g] + slot] = sv[j];
  }
  for (uint32_t g = 0; g < ng; ++g) {  // (wave-uniform) lists longer than SPEC: the rest
    const uint32_t a = S.upre[g], n = S.upre[g + 1] - a;
    for (uint32_t slot = SPEC + t; slot < n; slot += NT) S.lst[a + slot] = P.glist[(uint64_t)(g0 + g) * GCAP + slot];
  }
#pragma unroll
  for (uint32_t j = 0; j < CB; ++j)
    if (t + j * NT < nu) S.ge[t + j * NT] = gtc[j];
  for (uint32_t i = t + CB * NT; i < nu; i += NT) S.ge[i] = P.gtC[lb + i];
  __syncthreads();
  window_resolve<NT>(S, W, st, gmn0, gmx0, T_out, rt_out, fp, fn, gmn, gmx);
  return true;
}

// The exact k-th key inside the window [st.x, st.y] from the segment's in-window list S.lst[0, W) (index order), rank
// st.z inside the window; the entries above it and its ties applied to the per-unit counts in S.ge (above | equal << 16);
// the segment-wide tie ranks of the first positive / negative tie; min / max of the kept window entries folded into
// this thread's lmn / lmx (the values above the window). Block-level.
template <int NT>
DEV void window_resolve(SelSmem& S, uint32_t W, uint4 st, float lmn0, float lmx0, uint32_t& T_out, uint32_t& rt_out,
                        uint32_t& fp, uint32_t& fn, float& gmn, float& gmx) {
  const uint32_t t = threadIdx.x;
  uint32_t rt = st.z;
  const uint32_t T = block_select<NT, SEL_HB>(
      [&](auto&& f) {
        for (uint32_t i = t; i < W; i += NT) f(S.lst[i].x & KEY_MAX);
      },
      st.x, st.y, rt, S.hist, S.sh);
  constexpr uint32_t EPT = WLIST / NT;
  const uint32_t q0 = min(W, t * EPT), q1 = min(W, q0 + EPT);
  float lmn = qnan(), lmx = qnan();
  uint32_t leq = 0, lfp = NONE, lfn = NONE;
  for (uint32_t q = q0; q < q1; ++q) {
    const uint32_t vb = S.lst[q].x;
    const uint32_t key = vb & KEY_MAX;
    if (key > T) {
      atomicAdd(&S.ge[S.lst[q].y], 1u);
      lmn = fmin_nan(lmn, __uint_as_float(vb));
      lmx = fmax_nan(lmx, __uint_as_float(vb));
    } else if (key == T) {
      atomicAdd(&S.ge[S.lst[q].y], 1u << 16);
      const bool neg = (vb >> 31) != 0;
      lfp = min(lfp, neg ? NONE : leq);
      lfn = min(lfn, neg ? leq : NONE);
      ++leq;
    }
  }
  lmn = fmin_nan(lmn, lmn0);  // (select_from_groups: thread t < ng holds group t's)
  lmx = fmax_nan(lmx, lmx0);
  uint32_t teq;
  const uint32_t ex = block_excl_scan<NT>(leq, S.sh, teq);
  if (t == 0) {
    S.sh[42] = NONE;
    S.sh[43] = NONE;
  }
  __syncthreads();
  if (lfp != NONE) atomicMin(&S.sh[42], ex + lfp);
  if (lfn != NONE) atomicMin(&S.sh[43], ex + lfn);
  __syncthreads();
  T_out = T;  // per-unit counts stay in S.ge for the caller's in-order scan
  rt_out = rt;
  fp = S.sh[42];
  fn = S.sh[43];
  gmn = lmn;
  gmx = lmx;
  __syncthreads();
}

// Zero-tie ranks (tie mode, the k-th key is the segment's tie key K > 0): the segment-wide ranks of the first +K and
// -K ties, from the units' tie prefixes (S.ge >> 16 = the unit's K-keys) and in-unit ranks (tsgn). Block-level.
template <int NT>
DEV void zero_tie_ranks(const Params& P, uint32_t lb, uint32_t nu, SelSmem& S, uint32_t& fp_rank, uint32_t& fn_rank) {
  const uint32_t t = threadIdx.x;
  uint32_t lp = NONE, ln = NONE, carry = 0;
  for (uint32_t c0 = 0; c0 < nu; c0 += NT) {
    const uint32_t i = c0 + t;
    const uint32_t z = i < nu ? S.ge[i] >> 16 : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl_scan<NT>(z, S.sh, tot) + carry;
    carry += tot;
    if (i < nu) {
      const uint32_t sg = P.tsgn[lb + i], fp = sg & 0xFFFFu, fn = sg >> 16;
      if (fp != 0xFFFFu) lp = min(lp, ex + fp);
      if (fn != 0xFFFFu) ln = min(ln, ex + fn);
    }
  }
  if (t == 0) {
    S.sh[42] = NONE;
    S.sh[43] = NONE;
  }
  __syncthreads();
  if (lp != NONE) atomicMin(&S.sh[42], lp);
  if (ln != NONE) atomicMin(&S.sh[43], ln);
  __syncthreads();
  fp_rank = S.sh[42];
  fn_rank = S.sh[43];
  __syncthreads();
}

// The select of a segment that the window path cannot resolve: the generic multi-pass select over the records, or —
// on a bracket miss, a unit that overflowed its record slots, or COALAC_FLAG_FORCE_EXACT — the raw-data path (exact
// k-th key of the whole segment from its input, per-unit counts from the raw data, status 1: k_emit re-reads the input).
// Per-unit counts land in gtC / eqC. Block-level.
template <int NT, bool DELTA>
DEV void select_fallback(const Params& P, uint32_t s, const SegDev& sd, SelSmem& S, uint32_t& T, uint32_t& rt,
                         uint32_t& fp_rank, uint32_t& fn_rank, float& gmn, float& gmx, uint32_t& raw_path) {
  constexpr int NW = NT / 64;
  const uint32_t t = threadIdx.x, wv = t >> 6;
  const float* xs = seg_in(P, s, sd.in_off);
  const float* bs = DELTA ? P.base + sd.in_off : xs;
  const uint32_t lb = sd.lu_begin, nu = sd.unit_end - sd.unit_begin, k = sd.k;
  uint32_t sa = 0, sc = 0;
  for (uint32_t i = t; i < nu; i += NT) {
    sa += P.cntA[lb + i];
    sc += P.cntC[lb + i];
  }
  sa = block_sum<NT>(sa, S.sh);
  sc = block_sum<NT>(sc, S.sh);
  uint32_t mc = 0;  // most candidates any unit found (> ccap: records were dropped)
  for (uint32_t i = t; i < nu; i += NT) mc = max(mc, P.cntC[lb + i]);
  mc = wave_max_u32(mc);
  if (lane_id() == 0) S.wcnt[wv] = mc;
  __syncthreads();
  for (int i = 0; i < NW; ++i) mc = max(mc, S.wcnt[i]);
  __syncthreads();
  const uint32_t tlo = P.tlo[lb] & KEY_MAX, thi = P.thi[lb];  // (tie mode K: records are the keys above K)
  raw_path = 0u;
  if ((P.flags & COALAC_FLAG_FORCE_EXACT) || !(sa <= k && k <= sc) || mc > P.ccap) {
    // raw-data path (rare): the exact k-th key of the whole segment, per-unit counts from the raw data;
    // k_emit re-reads the raw data for this segment (status 1)
    const uint32_t n = sd.n;
    uint32_t rk = k;
    T = block_select<NT, SEL_HB>(
        [&](auto&& f) {
          for (uint32_t i = t; i < n; i += NT) f(fkey(load_x1p<DELTA>(xs + i, bs + i)));
        },
        0u, KEY_MAX, rk, S.hist, S.sh);
    rt = rk;
    raw_counts<NT, DELTA>(P, lb, nu, T, S.sh, S.wcnt, fp_rank, fn_rank, gmn, gmx, S.ge);
    raw_path = 1u;
    if (t == 0) pst(P, P.status + s, 1u);
  } else {
    // rank of the k-th key among candidates with key <= thi (0: none of them)
    select_generic<NT>(P, lb, nu, tlo, thi, k - sa, S, T, rt, fp_rank, fn_rank, gmn, gmx);
  }
}

// The end of every segment select: mn / scale from the kept values' min / max (+ the kept ties' ±T), the segment's
// T*, tie budget, mn, scale, and the in-order scan over its units — global tie prefix, output offsets (= the wire-v2
// starts), each unit's emit parameters (k_emit loads them with the unit's own words, in one round): {T*, tie budget |
// raw-data emit << 31, mn, scale} — raw-data emit for every unit of a raw-path segment, and for the units of a
// zero-tie segment whose K-keys the quota reaches. done: the per-unit counts are in S.ge (above | equal << 16), else
// in gtC / eqC. Block-level.
template <int NT, bool RAW>
DEV void select_finish(const Params& P, uint32_t s, const SegDev& sd, SelSmem& S, bool done, bool zero_tie,
                       uint32_t raw_path, uint32_t T, uint32_t rt, uint32_t fp_rank, uint32_t fn_rank, float gmn,
                       float gmx) {
  const uint32_t t = threadIdx.x;
  const uint32_t lb = sd.lu_begin, nu = sd.unit_end - sd.unit_begin;
  float mn = 0.0f, scale = 0.0f;
  if (!RAW) {
    const float tv = __uint_as_float(T);
    if (t == 0 && fp_rank < rt) {
      gmn = fmin_nan(gmn, tv);
      gmx = fmax_nan(gmx, tv);
    }
    if (t == 0 && fn_rank < rt) {
      gmn = fmin_nan(gmn, -tv);
      gmx = fmax_nan(gmx, -tv);
    }
    block_minmax<NT>(gmn, gmx, S.shf);
    codec_range(gmn, gmx, P.levels, mn, scale);
  }
  if (t == 0) {
    pst(P, P.tstar + s, T);
    pst(P, P.rtie + s, rt);
    pst(P, P.mn + s, mn);
    pst(P, P.scale + s, scale);
  }
  // thread t takes unit c0 + t of each NT-unit chunk (coalesced loads and stores): ONE paired block scan of the tie and
  // above-T* counts per chunk — the quotas of the units before u sum to min(rt, ties before u), so u's output offset is
  // its above-T* prefix + that. The counts are in LDS (S.ge) whenever nu <= UCAP (every path leaves them there); a
  // segment of more units (the generic path, chunk by chunk) reads gtC / eqC with L1-bypassing loads — this block
  // wrote them, and a plain load may hit a line this CU's L1 cached before (cdna_hip_programming.md §6 G16)
  const bool lds = done || nu <= UCAP;
  uint32_t carry_e = 0, carry_g = 0;
  for (uint32_t c0 = 0; c0 < nu; c0 += NT) {  // (block_excl_scan2 opens with a barrier: S.sh free again)
    const uint32_t i = c0 + t;
    const bool valid = i < nu;
    uint32_t e = 0, g = 0;
    if (valid) {
      if (lds) {
        const uint32_t v = S.ge[i];
        e = v >> 16;
        g = v & 0xFFFFu;
      } else {
        e = __builtin_nontemporal_load(P.eqC + lb + i);
        g = __builtin_nontemporal_load(P.gtC + lb + i);
      }
    }
    uint32_t ex, gx, te, tg;
    block_excl_scan2<NT>(e, g, S.sh, ex, gx, te, tg);
    ex += carry_e;
    gx += carry_g;
    carry_e += te;
    carry_g += tg;
    const uint32_t qp = umin_opaque(rt, ex);  // ties kept before unit i (see umin_opaque)
    const uint32_t quota = min(e, rt - qp);
    const uint32_t so = gx + qp;
    if (valid) {
      pst(P, P.eqpre + lb + i, ex);
      pst(P, P.outoff + lb + i, so);
      if (P.ustart_out != nullptr) pst(P, P.ustart_out + sd.unit_begin + i, so);  // wire v2: the unit's start
      const uint32_t rawu = raw_path | (zero_tie && quota > 0 ? 1u : 0u);
      P.uemit[lb + i] = make_uint4(T, rt | (rawu << 31), __float_as_uint(mn), __float_as_uint(scale));
    }
  }
}

template <int NT, bool DELTA, bool RAW>
DEV void segment_select(const Params& P, uint32_t li, SelSmem& S) {
  const uint32_t t = threadIdx.x;
  const uint32_t s = P.large_list[li];
  const SegDev sd = P.lsegs[li];  // (same load round as s and the select state)
  const uint4 st = P.sstate[li];
  const uint32_t lb = sd.lu_begin, nu = sd.unit_end - sd.unit_begin;
  STAMP(P, li, 0);
  uint32_t T = 0, rt = 0, fp_rank = NONE, fn_rank = NONE;
  float gmn = qnan(), gmx = qnan();
  const bool zero_tie = st.w == 2;  // the k-th key is the segment's tie key K (segment_pick; tie mode)
  bool done;
  if (zero_tie) {
    // every record kept (k_gwin's per-unit counts above the empty window), the first rt K-keys by index. K = 0: a
    // zero's sign does not matter to mn / scale (canonicalised + 0.0f below), so one "positive tie" stands for them;
    // K > 0: the segment-wide ranks of the first +K and -K ties (zero_tie_ranks)
    const uint32_t g0 = sd.g_begin, ng = (nu + GU - 1) / GU;  // ng <= UCAP / GU <= NT
    const uint32_t tk = P.tlo[lb] & KEY_MAX;
    gmn = t < ng ? P.gmm[2 * (g0 + t)] : qnan();
    gmx = t < ng ? P.gmm[2 * (g0 + t) + 1] : qnan();
    for (uint32_t i = t; i < nu; i += NT) S.ge[i] = P.gtC[lb + i] | (P.cntZ[lb + i] << 16);
    __syncthreads();
    T = tk;
    rt = st.z;
    fp_rank = rt > 0 ? 0u : NONE;
    if (tk != 0u) zero_tie_ranks<NT>(P, lb, nu, S, fp_rank, fn_rank);  // (block-uniform)
    done = true;
  } else {
    done = st.w == 0 && select_from_groups<NT>(P, sd, lb, nu, st, S, T, rt, fp_rank, fn_rank, gmn, gmx);
  }
  uint32_t raw_path = 0;
  STAMP(P, li, 1);
  if (!done) select_fallback<NT, DELTA>(P, s, sd, S, T, rt, fp_rank, fn_rank, gmn, gmx, raw_path);
  STAMP(P, li, 10);
  select_finish<NT, RAW>(P, s, sd, S, done, zero_tie, raw_path, T, rt, fp_rank, fn_rank, gmn, gmx);
  STAMP(P, li, 12);
}

template <bool DELTA, bool RAW, int NT = SEL_NT>
__global__ __launch_bounds__(NT) void k_select(Params P) {
  __shared__ SelSmem S;
  segment_select<NT, DELTA, RAW>(P, blockIdx.x, S);
}

// ------------------------------------------------------------------------------------------------
// k_emit: a block takes a tile of WAVES * UPW consecutive large units and its waves interleave them (wave w takes
// units w, w + WAVES, ...: emit_units' stride) — each unit's candidate list is already in index order: keep
// key > T and the ties whose segment-wide tie rank is < rt, compact with ballots, write idx + code. No LDS. A unit
// holds ~1.5 % of its 4096 elements as candidates (about one record per lane), so one unit per wave was a chain of
// dependent loads (count -> unit/segment metadata -> records) per 64 records: here lane g loads the metadata of the
// wave's g-th unit (two dependent rounds for all its units at once) and every unit's first 64 records are in flight
// before the first one is classified.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t EMIT_UPW = 4u;  // large units per k_emit wave in batches (round 6, with the interleaved tile: 4 vs 8
                                   // C3 0.586-0.595 vs 0.608-0.639 ms, C2 0.271 vs 0.275-0.278, C3_signs 1.427-1.436 vs
                                   // 1.471-1.543, C4 2.205 vs 2.155-2.202; 2 units: C3 0.624; profiles/r06_ab_emit_upw.txt)
// ... in latency-bound plans (<= LATENCY_PLAN_UNITS units): a wave's units are handled one after the other,
// so fewer per wave shortens the launch (one ResNet-50 update: 8 per wave 13.1 us, 2 per wave 6.0, 1 per
// wave 5.1)
constexpr uint32_t EMIT_UPW_LAT = 1u;

// the raw-data emit of one large unit (its segment took the raw-data path): re-read the unit, keep key > T
// and the ties whose segment-wide rank (eqp + ties before them) is < rt, in index order
template <bool DELTA, bool RAW>
DEV void emit_raw_unit(const Params& P, const UnitDev& L, uint32_t T, uint32_t rt, uint32_t eqp, uint64_t obase,
                       float mn, float scale) {
  const uint32_t lane = lane_id();
  uint32_t eqc = 0, outc = 0;
  raw_unit_rows<DELTA>(P, L, [&](uint32_t row, float4 v) {
    const float xs[4] = {v.x, v.y, v.z, v.w};
    const uint32_t e0 = (row * 64 + lane) * 4;
    bool gt[4], tie[4], sel[4];
    uint32_t tpre = 0, spre = 0, ntie = 0, nsel = 0;
    uint64_t tb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t key = fkey(xs[j]);
      const bool ok = e0 + j < L.len;
      gt[j] = ok && key > T;
      tie[j] = ok && key == T;
      tb[j] = __ballot(tie[j]);
      tpre += mbcnt(tb[j]);
      ntie += (uint32_t)__popcll(tb[j]);
    }
    uint32_t mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // rank of a tie: ties of lower lanes, then earlier ties of this lane
      sel[j] = gt[j] || (tie[j] && eqp + eqc + tpre + mine < rt);
      mine += tie[j] ? 1u : 0u;
    }
    uint64_t sb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sb[j] = __ballot(sel[j]);
      spre += mbcnt(sb[j]);
      nsel += (uint32_t)__popcll(sb[j]);
    }
    uint32_t k = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (sel[j]) {
        const uint64_t o = obase + outc + spre + k;
        P.idx[o] = (int32_t)(L.start + e0 + j);
        store_val<RAW>(P, o, xs[j], mn, scale);
        ++k;
      }
    }
    eqc += ntie;
    outc += nsel;
  });
}

// one wave emits the large units lu0 + g * stride, g < UPW, below lu1. Batches: a block takes a tile of WAVES * UPW
// consecutive units and its waves interleave them (stride WAVES), so the units that take the raw-data emit — a tie-mode
// segment's first ones, consecutive — are shared by the block's waves instead of filling one wave with 8 raw passes in
// series, while a wave's metadata loads stay within a few lines. (Striding by the whole grid spread them further but
// scattered every wave's metadata loads over 8 lines per array: C2 +2-10 %, C3 +1-6 % by box, profiles/r06_ab.txt.)
template <bool DELTA, bool RAW, uint32_t UPW, uint32_t TR>
DEV void emit_units(const Params& P, uint32_t lu0, uint32_t lu1, uint32_t stride) {
  const uint32_t lane = lane_id();
  auto unit = [&](uint32_t g) { return lu0 + g * stride; };
  const uint32_t ng = lu0 < lu1 ? min(UPW, (lu1 - lu0 + stride - 1) / stride) : 0u;  // this wave's units
  // lane g < UPW holds unit g's count, offsets and its segment's T*, tie budget, mn, scale (lanes past the wave's
  // units repeat its last one; never used)
  const uint32_t lug = unit(min(lane, ng - 1));
  uint32_t nCg, startg, eqpg, oog, Tg, rtg, stg;
  uint64_t sog;
  float mng, scg;
  uint2 rec0[UPW];  // {position, value bits}: every unit's first 64 records
  if constexpr (UPW == 1) {
    // latency-bound plans — ONE load round: the unit's count, record, offsets and its segment's emit parameters
    // (k_select copies them to every unit), and, before the count is known, the unit's first 64 (128) record
    // slots (ccap >= 128: slots past the count hold stale words, never used)
    const uint32_t nCr = P.cntC[lug];
    startg = P.lunits[lug].start;
    sog = P.lunits[lug].out_off;
    eqpg = P.eqpre[lug];
    oog = P.outoff[lug];
    const uint4 ue = P.uemit[lug];
    const uint64_t r0 = (uint64_t)lu0 * P.ccap;
    rec0[0] = make_uint2(P.cpos[r0 + lane], P.cval[r0 + lane]);
    nCg = min(nCr, P.ccap);  // stored records (a raw-path unit may have dropped some)
    Tg = ue.x;
    rtg = ue.y & 0x7FFFFFFFu;
    stg = ue.y >> 31;  // raw-data emit (a raw-path segment, or a zero-tie unit whose zeros the quota reaches)
    mng = RAW ? 0.0f : __uint_as_float(ue.z);
    scg = RAW ? 0.0f : __uint_as_float(ue.w);
  } else {
    // batches: round 1 — the unit's count, offsets and emit parameters; round 2 — every unit's first rows of
    // records (clamped to the count: the one-round form measured slower beside the other sub-batch's streaming)
    nCg = min(P.cntC[lug], P.ccap);
    startg = P.lunits[lug].start;
    sog = P.lunits[lug].out_off;
    eqpg = P.eqpre[lug];
    oog = P.outoff[lug];
    const uint4 ue = P.uemit[lug];
    Tg = ue.x;
    rtg = ue.y & 0x7FFFFFFFu;
    stg = ue.y >> 31;  // raw-data emit
    mng = RAW ? 0.0f : __uint_as_float(ue.z);
    scg = RAW ? 0.0f : __uint_as_float(ue.w);
#pragma unroll
    for (uint32_t g = 0; g < UPW; ++g) {
      const uint32_t lu = unit(min(g, ng - 1)), nC = rl(nCg, g);
      const uint32_t last = nC ? nC - 1 : 0u;
      const uint64_t r0 = (uint64_t)lu * P.ccap;  // unconditional (clamped) loads
      rec0[g] = make_uint2(P.cpos[r0 + min(lane, last)], P.cval[r0 + min(lane, last)]);
    }
  }
#pragma unroll
  for (uint32_t g = 0; g < UPW; ++g) {
    const uint32_t nC = rl(nCg, g);
    if (g < ng && rl(stg, g) != 0) {
      const uint64_t so = ((uint64_t)rl((uint32_t)(sog >> 32), g) << 32) | rl((uint32_t)sog, g);
      emit_raw_unit<DELTA, RAW>(P, P.lunits[unit(g)], rl(Tg, g), rl(rtg, g), rl(eqpg, g), so + rl(oog, g),
                                __uint_as_float(rl(__float_as_uint(mng), g)), __uint_as_float(rl(__float_as_uint(scg), g)));
    } else if (g < ng && nC != 0) {
      const uint32_t lu = unit(g);
      const uint32_t T = rl(Tg, g), rt = rl(rtg, g), eqp = rl(eqpg, g);
      const float mn = __uint_as_float(rl(__float_as_uint(mng), g));
      const float scale = __uint_as_float(rl(__float_as_uint(scg), g));
      const uint64_t so = ((uint64_t)rl((uint32_t)(sog >> 32), g) << 32) | rl((uint32_t)sog, g);
      const uint64_t obase = so + rl(oog, g);
      const uint32_t start = rl(startg, g);
      const uint64_t r0 = (uint64_t)lu * P.ccap;
      uint32_t eqc = 0, outc = 0;
      auto row = [&](uint32_t i0, uint2 rec) {
        const uint32_t i = i0 + lane;
        const bool valid = i < nC;
        const float x = __uint_as_float(rec.y);
        const uint32_t key = fkey(x);
        const bool e = valid && key == T;
        const uint64_t eb = __ballot(e);
        const uint32_t rank = eqp + eqc + mbcnt(eb);
        eqc += (uint32_t)__popcll(eb);
        const bool sel = valid && (key > T || (e && rank < rt));
        const uint64_t sb = __ballot(sel);
        if (sel) {
          const uint64_t o = obase + outc + mbcnt(sb);
          P.idx[o] = (int32_t)(start + rec.x);
          store_val<RAW>(P, o, x, mn, scale);
        }
        outc += (uint32_t)__popcll(sb);
      };
      row(0, rec0[g]);
      // rows past the first (preloaded) one: TR rows per load round (see tail_rows)
      for (uint32_t i0 = 64; i0 < nC; i0 += 64 * TR) {
        uint2 rb[TR];
#pragma unroll
        for (uint32_t b = 0; b < TR; ++b) {
          const uint32_t ic = min(i0 + b * 64 + lane, nC - 1);
          if (i0 + b * 64 < nC) rb[b] = make_uint2(P.cpos[r0 + ic], P.cval[r0 + ic]);  // (wave-uniform)
        }
#pragma unroll
        for (uint32_t b = 0; b < TR; ++b)
          if (i0 + b * 64 < nC) row(i0 + b * 64, rb[b]);
      }
    }
  }
}

template <bool DELTA, bool RAW, uint32_t UPW, uint32_t TR>  // TR: record rows per load round past the first
__global__ __launch_bounds__(BLOCK) void k_emit(Params P) {
  const uint32_t wv = threadIdx.x >> 6;
  const uint32_t t0 = blockIdx.x * WAVES * UPW;  // the block's tile of WAVES * UPW consecutive units
  if (t0 + wv >= P.n_lunits) return;
  const bool st = blockIdx.x < P.nseg;  // diagnostics rows: block index (slots 13-14)
  if (st) STAMP(P, blockIdx.x, 13);
  emit_units<DELTA, RAW, UPW, TR>(P, t0 + wv, min(t0 + WAVES * UPW, P.n_lunits), WAVES);
  if (st) STAMP(P, blockIdx.x, 14);
}

// ------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------
// k_decode_lds: every output line written ONCE (non-temporal float4 stores for batches). WPU waves per unit, each
// owning RPW = 16 / WPU of its 16 rows, in passes of QROWS rows through a per-wave LDS tile: the pass's kept
// values are scattered into the zeroed tile (one ds_write per 64 entries), its rows read back (ds_read_b128, + the
// base in delta mode, whose next pass's rows load while the current one goes through LDS) and stored, and the same
// slots zeroed again. The unit's entry range [lo, hi) comes from the per-unit starts: the payload's own (wire v2,
// written by the encoder) or k_bounds'. Round 2 merged the kept values in registers instead (a wave-uniform walk
// over every entry, ~10 VALU each: as much issue time per unit as its stores); round 3 measured one unit per wave in
// two 8-row passes fastest for batches (C3 0.672 -> 0.622 ms per step, profiles/r03_decode_ab.txt). Entries outside
// the wave's rows (an untrusted list) never match a pass and are dropped.
constexpr int DECODE_LDS_WPE = 5;
constexpr int DECODE_LDS_WPE_BASE = 4;  // delta mode: two passes of base rows in registers (5 per SIMD spilled)
constexpr uint32_t DECODE_QROWS = 8u;  // batches, weights mode: rows per tile pass (8: half a unit, 8 KiB of LDS per wave; 4 rows: C3
                                       // 0.671-0.674 ms per step, 8 rows: 0.621-0.623, profiles/r03_decode_ab.txt)
constexpr uint32_t DECODE_QROWS_BASE = 4u;  // delta mode: rows per tile pass
constexpr int DECODE_NT = 256;  // k_decode_lds block size (its per-wave LDS tile is QROWS KiB)
constexpr uint32_t DECODE_WPU_LAT = 2u;  // latency-bound plans: waves per unit (one update: every wave one 8-row pass)
constexpr int DECODE_SAUX_LAT = 0;  // latency-bound plans: store cache policy (a ~100 MB output: plain stores)

// NCH: 64-entry chunks of the unit's kept entries held in registers across the passes (1 at ratios up to ~1.5 %;
// plans of higher ratios take 8 — up to 512 entries, ratio ~12 % — so the entry lists are loaded once per unit,
// not once per pass and again for the zeroing); chunks past NCH are loaded per pass as before
template <bool RAW, bool HASBASE, uint32_t WPU, uint32_t QROWS, int SAUX, bool XCD, uint32_t NCH = 1>
__global__ __launch_bounds__(DECODE_NT, HASBASE ? DECODE_LDS_WPE_BASE : DECODE_LDS_WPE) void k_decode_lds(Params P) {
  constexpr uint32_t DW = DECODE_NT / 64, RPW = UNIT_IT / WPU, NPASS = RPW / QROWS;
  constexpr uint32_t QSH = QROWS == 2u ? 9u : QROWS == 4u ? 10u : QROWS == 8u ? 11u : 12u, QM = (1u << QSH) - 1u;
  static_assert((QROWS << 8) == (1u << QSH) && RPW % QROWS == 0 && NPASS >= 1, "tile pass geometry");
  __shared__ float4 qtile[DW][QROWS * 64];
  const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
  const uint32_t wid = (XCD ? xcd_block(blockIdx.x) : blockIdx.x) * DW + wv;
  const uint32_t u = wid / WPU, pass0 = (wid % WPU) * NPASS;  // this wave's unit and first pass (QROWS rows each)
  if (u >= P.n_units) return;
  float4* tile = qtile[wv];
  float* tf = reinterpret_cast<float*>(tile);
#pragma unroll
  for (uint32_t it = 0; it < QROWS; ++it) tile[it * 64 + lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  // round 1: the unit and its entry range (the next unit's start is the end of this one's: a non-last unit is
  // followed by its segment's next unit; the index is clamped for the plan's final unit, which is a last unit)
  const UnitDev U = P.units[u];
  uint32_t lo = P.ustart[u];
  uint32_t hi = P.ustart[min(u + 1, P.n_units - 1)];
  const float mn = RAW ? 0.0f : P.cmn[U.seg], sc = RAW ? 0.0f : P.cscale[U.seg];
  // clamp: the bounds may come from an untrusted payload (k >= 1 for every unit); a valid unit holds at most len
  // kept entries (distinct positions), which also bounds the entry loops below for any corrupt range
  lo = min(lo, U.k);
  hi = max(lo, min(min(U.last ? U.k : hi, U.k), lo + U.len));
  const uint32_t cnt = hi - lo;
  // round 2: the first NCH x 64 entries (+ the base rows of the first pass)
  uint32_t qc[NCH], posc[NCH];
#pragma unroll
  for (uint32_t c = 0; c < NCH; ++c) {
    const uint64_t e1 = U.out_off + min(lo + c * 64 + lane, U.k - 1);
    qc[c] = load_code<RAW>(P, e1);
    posc[c] = (uint32_t)P.cidx[e1] - U.start;
  }
  const uint32_t len = U.len;
  const __amdgpu_buffer_rsrc_t rout = unit_rsrc(P.out + U.off, len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(HASBASE ? P.base + U.off : P.out + U.off, len);
  float4 bq[QROWS], bn[QROWS];
  if (HASBASE) {
#pragma unroll
    for (uint32_t it = 0; it < QROWS; ++it) bn[it] = unit_load_x4<false>(rb, rb, ((pass0 * QROWS + it) * 64 + lane) * 16);
  }
  float valc[NCH];
#pragma unroll
  for (uint32_t c = 0; c < NCH; ++c) valc[c] = code_value<RAW>(qc[c], mn, sc);
  lds_order();
#pragma unroll
  for (uint32_t qi = 0; qi < NPASS; ++qi) {
    const uint32_t qq = pass0 + qi;
    if (HASBASE) {
#pragma unroll
      for (uint32_t it = 0; it < QROWS; ++it) bq[it] = bn[it];
      if (qi + 1 < NPASS) {
#pragma unroll
        for (uint32_t it = 0; it < QROWS; ++it)
          bn[it] = unit_load_x4<false>(rb, rb, (((qq + 1) * QROWS + it) * 64 + lane) * 16);
      }
    }
    // scatter: the first NCH x 64 entries are in registers; more are loaded chunk by chunk
#pragma unroll
    for (uint32_t c = 0; c < NCH; ++c)
      if (c * 64 + lane < cnt && (posc[c] >> QSH) == qq) tf[posc[c] & QM] = valc[c];
    for (uint32_t e0 = lo + NCH * 64; e0 < hi; e0 += 64) {
      const uint64_t e = U.out_off + min(e0 + lane, hi - 1);
      const uint32_t p2 = (uint32_t)P.cidx[e] - U.start;
      if (e0 + lane < hi && (p2 >> QSH) == qq) tf[p2 & QM] = code_value<RAW>(load_code<RAW>(P, e), mn, sc);
    }
    lds_order();
    float4 o[QROWS];
#pragma unroll
    for (uint32_t it = 0; it < QROWS; ++it) {
      const float4 d = tile[it * 64 + lane];
      o[it] = HASBASE ? make_float4(bq[it].x + d.x, bq[it].y + d.y, bq[it].z + d.z, bq[it].w + d.w) : d;
    }
    lds_order();
    if (qi + 1 < NPASS) {  // zero what was written (the same slots), for the next pass
#pragma unroll
      for (uint32_t c = 0; c < NCH; ++c)
        if (c * 64 + lane < cnt && (posc[c] >> QSH) == qq) tf[posc[c] & QM] = 0.0f;
      for (uint32_t e0 = lo + NCH * 64; e0 < hi; e0 += 64) {
        const uint64_t e = U.out_off + min(e0 + lane, hi - 1);
        const uint32_t p2 = (uint32_t)P.cidx[e] - U.start;
        if (e0 + lane < hi && (p2 >> QSH) == qq) tf[p2 & QM] = 0.0f;
      }
    }
    if ((len & 3u) == 0) {  // wave-uniform: one float4 buffer store per slot
#pragma unroll
      for (uint32_t it = 0; it < QROWS; ++it) unit_store_x4<SAUX>(rout, ((qq * QROWS + it) * 64 + lane) * 16, o[it]);
    } else {  // a segment's last unit with n % 4 != 0: dword stores (range-checked per dword)
#pragma unroll
      for (uint32_t it = 0; it < QROWS; ++it) unit_store_x1x4<SAUX>(rout, ((qq * QROWS + it) * 64 + lane) * 16, o[it]);
    }
    lds_order();
  }
}

// ------------------------------------------------------------------------------------------------
// aggregate: fused server-side decode + FedAvg of C client updates of one layout
// ------------------------------------------------------------------------------------------------
constexpr int AGG_WPE = 1;  // k_aggregate launch-bounds blocks per CU (register budget)
constexpr uint32_t AGG_SPLIT = 2u;  // waves per 4096-element unit in k_aggregate (each owns UNIT_IT / AGG_SPLIT rows)
constexpr uint32_t AGG_DEPTH = 16u;  // clients whose entries k_aggregate loads together (16 ResNet-50 clients: 4 -> 73.5 us, 8 -> 70.9 us, 16 -> 69.1 us)

struct AggArgs {
  const uint32_t* ustart;  // [n_units] the clients' per-unit starts (wire v2)
  const float* weights;    // [clients] fp32 weights (float(w_i), as torch converts a Python scalar)
  uint32_t clients, T, U0; // clients, segments per client, units per client
  uint64_t Kc;             // kept entries per client (out_off stride between clients)
  float total, inv_total;  // sum of weights; 1.0f / total (fp32 division)
  const uint8_t* avg_mask; // [T] 1: segment averaged, 0: client 0's value passed through; null: all averaged
};

// the end of an averaged element, one copy for k_aggregate and k_aggregate_dense: acc / total (DIV), acc * (1.0f / total)
// (RECIP, inv_total = the fp32 quotient 1.0f / total) or acc (SUM)
template <int MODE>
DEV float4 agg_final(float4 a, float total, float inv_total) {
  if (MODE == COALAC_AGG_DIV) return make_float4(a.x / total, a.y / total, a.z / total, a.w / total);
  if (MODE == COALAC_AGG_SUM) return a;
  return make_float4(a.x * inv_total, a.y * inv_total, a.z * inv_total, a.w * inv_total);
}

// k_aggregate: one wave per 4096-element unit of the (client-0) layout. For client i in order (segments
// the avg mask leaves out — the buffers of aggregation_content "parameters" — take client 0's x_0 as is,
// as strategies.weighted_sum_only_params / federated_averaging_only_params leave models[0]'s buffers,
// coala/server/strategies.py:32-54, 93-124):
//   x_i = base + d_i   (d_i = decoded value where client i kept the element, +0.0f elsewhere: exactly
//                       what coalac_decode with a base writes; without a base x_i = d_i)
//   acc = x_0 * w_0, then acc = acc + (x_i * w_i)        (torch: params *= w0; params += s_i * w_i)
//   out = acc / total (mode DIV, torch CPU division) or acc * (1.0f / total) (mode RECIP, torch GPU
//   division by a host scalar)                       — coala/server/strategies.py:6-29, 57-90
//   or out = acc (mode SUM: weighted_sum, strategies.py:57-90, whose result the distributed server hands
//   to reduce_models, coala/distributed/distributed.py:42-57)
// x_i goes through a per-wave LDS tile holding base + 0.0f (= base, checked per wave; zero without a base):
// at the client's kept positions base + d_i is written, every lane reads its rows back with ds_read_b128
// (x_i itself: one multiply and one add per element and client), then the base value is put back.
// Latency: every client's range / mn / scale / weight is fetched lane-parallel in one round (lane j =
// client j of a 64-client chunk); the first 64 kept entries of AGG_DEPTH clients are then loaded in one
// batch and accumulated in client order (a unit where some client keeps more than 64 entries takes the
// unbatched path, one client at a time).
// Where a client's range and entries come from is the body's SRC:
//   AGG_STRIDED  one batched plan: the clients are identical copies of one layout, so client c's unit / segment /
//                entry offsets are u + c*U0, seg + c*T, out_off + c*Kc (host-validated)       — k_aggregate
//   AGG_ENTRIES  a one-layout plan and per-client pointers: client c's idx / vals / mn / scale / ustart arrays are
//                where its upload landed. Lane j fetches client j's pointers in a round of their own before the
//                starts' (they need only the client number); the entries' pointers are read across lanes
//   AGG_COMPACT  as ENTRIES, the entries being the (12 + B)-bit fields of the client's wire v3 stream: the field's
//                word and the next (clamped inside the stream), funnel-shifted where they are used; at bits 32 the
//                fp32 value of entry j is vals[j]                                       — k_aggregate_uploads
enum { AGG_STRIDED = 0, AGG_ENTRIES = 1, AGG_COMPACT = 2 };

struct AggUploads {  // device arrays of `clients` device pointers each (null where the kind does not read them)
  const int32_t* const* idx;
  const uint32_t* const* packed;
  const void* const* vals;
  const float* const* mn;
  const float* const* scale;
  const uint32_t* const* ustart;
  uint64_t nwords;  // COMPACT: words of every client's stream
  uint32_t w;       // COMPACT: field bits, 12 + B
};
struct AggNoUploads {};

// a lane's client: where its starts, mn, scale, entries (idx or the stream) and values are
template <int SRC>
struct AggClient {
  const uint32_t* ustart;
  const float *mn, *scale;
  const void *ent, *vals;
};
template <>
struct AggClient<AGG_STRIDED> {};

template <int SRC, bool RAW, bool HASBASE, int MODE, class Uploads>
DEV void aggregate_unit(const Params& P, const AggArgs& A, const Uploads& S) {
  // AGG_SPLIT waves per unit, each owning RI of its UNIT_IT rows: a smaller LDS tile and half the registers
  // per wave, so twice the waves are resident
  constexpr uint32_t RI = UNIT_IT / AGG_SPLIT, HE = UNIT / AGG_SPLIT;  // rows / elements per wave
  __shared__ float4 tiles[WAVES][HE / 4];
  const uint32_t lane = lane_id(), wv = threadIdx.x >> 6;
  const uint32_t wid = blockIdx.x * WAVES + wv;
  const uint32_t u = __builtin_amdgcn_readfirstlane(wid / AGG_SPLIT), h = __builtin_amdgcn_readfirstlane(wid % AGG_SPLIT);
  if (u >= A.U0) return;
  // round 0 (per-client pointers only): lane j's client of the chunk at c0, its pointers
  AggClient<SRC> C;
  auto client_of = [&](uint32_t c0) {
    if constexpr (SRC != AGG_STRIDED) {
      const uint32_t cl = c0 + min(lane, min(64u, A.clients - c0) - 1);
      C.ustart = S.ustart[cl];
      C.mn = RAW ? nullptr : S.mn[cl];
      C.scale = RAW ? nullptr : S.scale[cl];
      C.ent = SRC == AGG_COMPACT ? static_cast<const void*>(S.packed[cl]) : static_cast<const void*>(S.idx[cl]);
      C.vals = SRC == AGG_COMPACT && !RAW ? nullptr : S.vals[cl];
    }
  };
  // the starts of lane j's client in this unit
  auto starts_of = [&](uint32_t c0, uint32_t& s0, uint32_t& s1) {
    if constexpr (SRC == AGG_STRIDED) {
      const uint32_t ucl = u + (c0 + min(lane, min(64u, A.clients - c0) - 1)) * A.U0;
      s0 = A.ustart[ucl];
      s1 = A.ustart[min(ucl + 1, P.n_units - 1)];
    } else {
      s0 = C.ustart[u];
      s1 = C.ustart[min(u + 1, P.n_units - 1)];
    }
  };
  client_of(0);
  // round 1: the unit (scalar loads), and the first 64 clients' starts in it (lane j: client j; they need
  // only u), pinned above the first use of either
  const UnitDev U = P.units[u];
  uint32_t us0, us1;
  starts_of(0, us0, us1);
  asm volatile("" : "+v"(us0), "+v"(us1)::"memory");
  const uint32_t len = U.len, kseg = U.k;
  const uint32_t e_lo = h * HE;  // first element (within the unit) of this wave's rows
  if (e_lo >= len) return;
  const uint32_t hlen = min(len - e_lo, HE);
  float4* tile = tiles[wv];
  float* tf = reinterpret_cast<float*>(tile);
  const float* bs = HASBASE ? P.base + U.off + e_lo : nullptr;
  // the body twice: full 2048-element rows (every load and store a float4, no length test, so no control-flow
  // merge drains the loads in flight) and a unit's partial last rows
  auto body = [&](auto full_tag) {
    constexpr bool FULL = decltype(full_tag)::value;
    const uint32_t hl = FULL ? HE : hlen;
    auto load_base = [&](uint32_t it) -> float4 {
      const uint32_t e = (it * 64 + lane) * 4;
      if (FULL) return *reinterpret_cast<const float4*>(bs + e);
      return make_float4(e + 0 < hl ? bs[e + 0] : 0.0f, e + 1 < hl ? bs[e + 1] : 0.0f,
                         e + 2 < hl ? bs[e + 2] : 0.0f, e + 3 < hl ? bs[e + 3] : 0.0f);
    };
    // ---- round 2, every request of it issued before any is used: the avg flag, the clients' mn / scale /
    // weight, the base rows and the first AGG_DEPTH clients' entries (all unconditional: a select after a
    // load, never a branch around it)
    struct Meta {
      uint32_t lo, hi;
      float mn, sc, w;
    };
    // lane j: client c0 + j (clamped to the last client of the chunk)
    auto meta_of = [&](uint32_t c0, uint32_t s0, uint32_t s1) -> Meta {
      const uint32_t cl = c0 + min(lane, min(64u, A.clients - c0) - 1);
      Meta m;
      m.lo = min(s0, kseg);
      m.hi = max(m.lo, min(min(U.last ? kseg : s1, kseg), m.lo + len));
      if constexpr (SRC == AGG_STRIDED) {
        const uint32_t sl = U.seg + cl * A.T;
        m.mn = RAW ? 0.0f : P.cmn[sl];
        m.sc = RAW ? 0.0f : P.cscale[sl];
      } else {
        m.mn = RAW ? 0.0f : C.mn[U.seg];
        m.sc = RAW ? 0.0f : C.scale[U.seg];
      }
      m.w = A.weights[cl];
      return m;
    };
    auto meta = [&](uint32_t c0) -> Meta {
      uint32_t s0, s1;
      client_of(c0);
      starts_of(c0, s0, s1);
      return meta_of(c0, s0, s1);
    };
    // lane jj's pointer, wave-uniform
    auto lanep = [](const void* p, uint32_t jj) -> const void* {
      const uint64_t b = reinterpret_cast<uint64_t>(p);
      const uint32_t l = __builtin_amdgcn_readlane((uint32_t)b, jj), hw = __builtin_amdgcn_readlane((uint32_t)(b >> 32), jj);
      return reinterpret_cast<const void*>((uint64_t)hw << 32 | l);
    };
    // COMPACT: entry e of the unit's segment in a stream, its field's word, the next word inside the stream and
    // the field's first bit in the word
    auto field_at = [&](uint32_t e, uint64_t& wd, uint64_t& wd1, uint32_t& sh) {
      if constexpr (SRC == AGG_COMPACT) {
        const uint64_t bit = (U.out_off + e) * S.w;
        wd = bit >> 5;  // (wd < nwords: out_off + e < total_k and the stream holds total_k fields)
        wd1 = min(wd + 1, S.nwords - 1);
        sh = (uint32_t)bit & 31u;
      }
    };
    // ... and the entry from the two words: v_alignbit_b32 takes the 32 bits from bit sh of b:a (a itself at
    // sh == 0). A field that ends inside a takes none of b's bits below the mask; one that straddles has its
    // second word inside the stream (total_k fields fit nwords words)
    auto field_entry = [&](uint32_t a, uint32_t b, uint32_t sh, uint32_t raw, uint32_t& idx, uint32_t& q) {
      if constexpr (SRC == AGG_COMPACT) {
        const uint32_t v = __builtin_amdgcn_alignbit(b, a, sh) & ((1u << S.w) - 1u);
        idx = U.start | (v & 0xFFFu);
        q = RAW ? raw : v >> 12;
      }
    };
    // entries of client c0 + j: the raw loaded words only (any arithmetic on them here would make the wave
    // wait for the loads right away, in-order vmcnt). COMPACT: the field's two words (x, q), at bits 32 the value (r)
    auto fetch = [&](const Meta& M, uint32_t c0, uint32_t j, uint32_t& idx, uint32_t& q, uint32_t& r) {
      const uint32_t jj = min(j, min(64u, A.clients - c0) - 1);
      r = 0;
      const uint32_t lo = __builtin_amdgcn_readlane(M.lo, jj), hi = __builtin_amdgcn_readlane(M.hi, jj);
      const uint64_t oo = U.out_off + (SRC == AGG_STRIDED ? (uint64_t)(c0 + jj) * A.Kc : 0);
      const uint32_t e = min(lo + lane, hi > lo ? hi - 1 : lo);  // kseg >= 1: entry lo always exists
      if constexpr (SRC == AGG_STRIDED) {
        idx = (uint32_t)P.cidx[oo + min(e, kseg - 1)];
        q = load_code<RAW>(P, oo + min(e, kseg - 1));
      } else if constexpr (SRC == AGG_ENTRIES) {
        const uint64_t o = oo + min(e, kseg - 1);
        idx = (uint32_t) static_cast<const int32_t*>(lanep(C.ent, jj))[o];
        const void* vp = lanep(C.vals, jj);
        q = RAW ? __float_as_uint(static_cast<const float*>(vp)[o]) : static_cast<const uint8_t*>(vp)[o];
      } else {
        const uint32_t* pk = static_cast<const uint32_t*>(lanep(C.ent, jj));
        uint64_t wd, wd1;
        uint32_t sh;
        field_at(min(e, kseg - 1), wd, wd1, sh);
        idx = pk[wd];
        q = pk[wd1];
        if (RAW) r = __float_as_uint(static_cast<const float*>(lanep(C.vals, jj))[oo + min(e, kseg - 1)]);
      }
    };
    // the fetched entry as its index and code (COMPACT: extracted here, where the words are first used)
    auto entry_of = [&](const Meta& M, uint32_t c0, uint32_t j, uint32_t x, uint32_t y, uint32_t r, uint32_t& idx,
                        uint32_t& q) {
      if constexpr (SRC == AGG_COMPACT) {
        const uint32_t jj = min(j, min(64u, A.clients - c0) - 1);
        const uint32_t lo = __builtin_amdgcn_readlane(M.lo, jj), hi = __builtin_amdgcn_readlane(M.hi, jj);
        const uint32_t e = min(min(lo + lane, hi > lo ? hi - 1 : lo), kseg - 1);
        field_entry(x, y, ((uint32_t)U.out_off + e) * S.w & 31u, r, idx, q);
      } else {
        idx = x;
        q = y;
      }
    };
    // entry e (< kseg) of client c0 + j, loaded and used at once (the generic path)
    auto entry_at = [&](uint32_t c0, uint32_t j, uint32_t e, uint32_t& idx, uint32_t& q) {
      if constexpr (SRC == AGG_STRIDED) {
        const uint64_t oo = U.out_off + (uint64_t)(c0 + j) * A.Kc;
        idx = (uint32_t)P.cidx[oo + e];
        q = load_code<RAW>(P, oo + e);
      } else if constexpr (SRC == AGG_ENTRIES) {
        const uint64_t o = U.out_off + e;
        idx = (uint32_t) static_cast<const int32_t*>(lanep(C.ent, j))[o];
        const void* vp = lanep(C.vals, j);
        q = RAW ? __float_as_uint(static_cast<const float*>(vp)[o]) : static_cast<const uint8_t*>(vp)[o];
      } else {
        const uint32_t* pk = static_cast<const uint32_t*>(lanep(C.ent, j));
        uint64_t wd, wd1;
        uint32_t sh, raw = 0;
        field_at(e, wd, wd1, sh);
        if (RAW) raw = __float_as_uint(static_cast<const float*>(lanep(C.vals, j))[U.out_off + e]);
        field_entry(pk[wd], pk[wd1], sh, raw, idx, q);
      }
    };
    float4 bv[RI];
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) bv[it] = HASBASE ? load_base(it) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    lds_order();  // the requests below stay in this body (common to both, the compiler would hoist them above
                  // the length test, whose branch then drains them)
    const uint8_t* amp = A.avg_mask != nullptr ? A.avg_mask + U.seg : reinterpret_cast<const uint8_t*>(A.weights);
    uint32_t am = *amp;
    Meta M = meta_of(0, us0, us1);
    uint32_t pa[AGG_DEPTH], qa[AGG_DEPTH], ra[AGG_DEPTH];  // (ra: COMPACT at bits 32 only)
#pragma unroll
    for (uint32_t t = 0; t < AGG_DEPTH; ++t) fetch(M, 0, t, pa[t], qa[t], ra[t]);
    // pinned: no request above moves below this point (the compiler sinks loads toward their first use,
    // which would put the entries' round behind the base's)
    asm volatile("" : "+v"(M.lo), "+v"(M.hi), "+v"(M.mn), "+v"(M.sc), "+v"(M.w), "+v"(am)::"memory");
    const bool avg = A.avg_mask == nullptr || am != 0;
    const uint32_t nclients = avg ? A.clients : 1u;
    if (!avg) M.w = 1.0f;  // (x_0 * 1.0f == x_0)
    // The tile holds x_i where client i kept nothing: base + 0.0f (HASBASE) or +0.0f. The fast path writes
    // tile + d_i at a client's kept positions, which is base + d_i only where base + 0.0f == base: a wave
    // whose rows hold a -0.0f or a NaN base ("odd") takes the generic path, which adds the base read from
    // global memory
    bool odd = false;
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) {
      const float v[4] = {bv[it].x, bv[it].y, bv[it].z, bv[it].w};
      if (HASBASE) {
#pragma unroll
        for (int c = 0; c < 4; ++c) odd |= __float_as_uint(v[c]) == 0x80000000u || v[c] != v[c];
      }
      const f2v l = f2v{v[0], v[1]} + f2v{0.0f, 0.0f}, h2 = f2v{v[2], v[3]} + f2v{0.0f, 0.0f};
      tile[it * 64 + lane] = HASBASE ? make_float4(l.x, l.y, h2.x, h2.y) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    odd = HASBASE && __ballot(odd) != 0;
    // acc starts at -0.0f, the exact additive identity (-0 + t == t for every t, signed zeros included): the
    // first client's acc + x_0 * w_0 is torch's x_0 * w_0 bit for bit, and no client is special
    float4 acc[RI];
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) acc[it] = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
    // acc = acc + x * w: IEEE fp32 ops in this order, on float2 pairs (v_pk_mul_f32 / v_pk_add_f32), x read
    // from the tile
    auto accumulate = [&](float w) {
      const f2v w2 = {w, w};
#pragma unroll
      for (uint32_t it = 0; it < RI; ++it) {
        const float4 x = tile[it * 64 + lane];
        const f2v tl = f2v{x.x, x.y} * w2, th = f2v{x.z, x.w} * w2;
        const f2v sl2 = f2v{acc[it].x, acc[it].y} + tl, sh2 = f2v{acc[it].z, acc[it].w} + th;
        acc[it] = make_float4(sl2.x, sl2.y, sh2.x, sh2.y);
      }
    };
    auto lanef = [](float v, uint32_t j) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), j)); };
    const uint32_t pbase = U.start + e_lo;
    for (uint32_t c0 = 0; c0 < nclients; c0 += 64) {
      if (c0 > 0) {
        M = meta(c0);
#pragma unroll
        for (uint32_t t = 0; t < AGG_DEPTH; ++t) fetch(M, c0, t, pa[t], qa[t], ra[t]);
      }
      const uint32_t cn = min(64u, nclients - c0);
      // generic path (an odd wave, or any client with more than 64 kept entries in this unit, ratio >~ 1.5 %):
      // every client in turn, its entries loaded chunk by chunk, x_i = base + d_i with the base from global
      // memory, put back as base + 0.0f after the rows are read
      if (odd || __ballot(lane < cn && M.hi - M.lo > 64) != 0) {
        for (uint32_t j = 0; j < cn; ++j) {
          const uint32_t lo = __builtin_amdgcn_readlane(M.lo, j), hi = __builtin_amdgcn_readlane(M.hi, j);
          const float mn = lanef(M.mn, j), sc = lanef(M.sc, j);
          for (uint32_t e = lo + lane; e < hi; e += 64) {
            uint32_t ix, q;
            entry_at(c0, j, e, ix, q);
            const uint32_t p2 = ix - pbase;
            const float v2 = code_value<RAW>(q, mn, sc);
            if (p2 < hl) tf[p2] = HASBASE ? bs[p2] + v2 : v2;
          }
          lds_order();
          accumulate(lanef(M.w, j));
          lds_order();
          for (uint32_t e = lo + lane; e < hi; e += 64) {
            uint32_t ix, q;
            entry_at(c0, j, e, ix, q);
            const uint32_t p2 = ix - pbase;
            if (p2 < hl) tf[p2] = HASBASE ? bs[p2] + 0.0f : 0.0f;
          }
          lds_order();
        }
        continue;
      }
      // fast path, in client order: x = tile + d written at the client's positions, the rows read and
      // accumulated, the tile's value put back. The tile value under the next client's entries is read right
      // after this client's put-back, so the wave never waits on it
      for (uint32_t j0 = 0; j0 < cn; j0 += AGG_DEPTH) {
        if (j0 > 0) {
#pragma unroll
          for (uint32_t t = 0; t < AGG_DEPTH; ++t) fetch(M, c0, j0 + t, pa[t], qa[t], ra[t]);
        }
        uint32_t ix, q, ixn = 0, qn = 0;
        entry_of(M, c0, j0, pa[0], qa[0], ra[0], ix, q);
        float tb = HASBASE ? tf[min(ix - pbase, HE - 1)] : 0.0f;
#pragma unroll
        for (uint32_t t = 0; t < AGG_DEPTH; ++t) {
          const uint32_t j = j0 + t;
          if (j >= cn) continue;
          if constexpr (SRC != AGG_COMPACT)
            entry_of(M, c0, j, pa[t], qa[t], ra[t], ix, q);  // (the loaded words themselves)
          else if (t > 0)
            ix = ixn, q = qn;  // (extracted once, for the tile value read under it)
          const uint32_t pos = ix - pbase;  // wraps (>= hl) outside this wave's rows
          const uint32_t ne = __builtin_amdgcn_readlane(M.hi, j) - __builtin_amdgcn_readlane(M.lo, j);
          const bool mine = lane < ne && pos < hl;
          const float d = code_value<RAW>(q, lanef(M.mn, j), lanef(M.sc, j));
          if (mine) tf[pos] = HASBASE ? tb + d : d;
          lds_order();
          accumulate(lanef(M.w, j));
          lds_order();
          if (mine) tf[pos] = tb;
          if (t + 1 < AGG_DEPTH) entry_of(M, c0, j + 1, pa[t + 1], qa[t + 1], ra[t + 1], ixn, qn);
          if (HASBASE && t + 1 < AGG_DEPTH) tb = tf[min(ixn - pbase, HE - 1)];
          lds_order();
        }
      }
    }
    float* out = P.out + U.off + e_lo;
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) {
      const float4 o = avg ? agg_final<MODE>(acc[it], A.total, A.inv_total) : acc[it];
      const uint32_t e = (it * 64 + lane) * 4;
      if (FULL) {
        *reinterpret_cast<float4*>(out + e) = o;
      } else {
        if (e + 0 < hl) out[e + 0] = o.x;
        if (e + 1 < hl) out[e + 1] = o.y;
        if (e + 2 < hl) out[e + 2] = o.z;
        if (e + 3 < hl) out[e + 3] = o.w;
      }
    }
  };
  if (hlen == HE)
    body(std::true_type{});
  else
    body(std::false_type{});
}

template <bool RAW, bool HASBASE, int MODE>
__global__ __launch_bounds__(BLOCK, AGG_WPE) void k_aggregate(Params P, AggArgs A) {
  aggregate_unit<AGG_STRIDED, RAW, HASBASE, MODE>(P, A, AggNoUploads{});
}

// k_aggregate's body over a one-layout plan, every client's arrays where its upload landed (A.U0 = the plan's units;
// A.ustart, A.T and A.Kc are not read). SRC: AGG_ENTRIES or AGG_COMPACT
template <int SRC, bool RAW, bool HASBASE, int MODE>
__global__ __launch_bounds__(BLOCK, AGG_WPE) void k_aggregate_uploads(Params P, AggArgs A, AggUploads S) {
  aggregate_unit<SRC, RAW, HASBASE, MODE>(P, A, S);
}

// ------------------------------------------------------------------------------------------------
// dense codec: a plan whose every segment keeps all n elements (ratio 1 — the download direction's default,
// coala/server/base.py:196,397 — or segments too small to drop anything). The index list is implied (0..n-1
// per segment) and never materialised; a caller that passes idx / ustart buffers still gets them written.
//   encode: k_dense_minmax (per unit, NaN-ignoring min / max) -> k_dense_seg (per segment: mn, scale) ->
//           k_dense_quant (per unit: read 4 B, write the 1-B code)         — HBM 4 B + 1 B per element
//           (the min / max pass reads the update once more; an update that fits the 256 MB Infinity Cache
//           is re-read from it)
//   decode: k_dense_deq (per unit: read the 1-B code, write 4 B; + base in delta mode)
// One wave per 4096-element unit, 16 float4 per lane, XCD-aware unit order in batches.
// ------------------------------------------------------------------------------------------------
// cache policies: the min / max pass reads with the default policy (an update that fits the Infinity Cache is still
// there for the quantise pass, which reads non-temporally); the dense decode stores non-temporally (one update's
// download 0.073 vs 0.088 ms per step with plain stores; a reciprocal-multiply quantise measured no faster: these
// streams are memory-bound, profiles/r05_ab.txt)
constexpr int DENSE_MM_AUX = 0;
constexpr int DENSE_Q_AUX = 2;  // the quantise stream's loads (non-temporal)
template <bool DELTA, int AUX>  // (AUX: the loads' cache policy)
DEV void dense_unit_load(const Params& P, const UnitDev& U, float4 (&v)[UNIT_IT]) {
  typedef unsigned int u4v __attribute__((ext_vector_type(4)));
  const uint32_t lane = lane_id();
  const float* xin = P.inptr != nullptr ? P.inptr[U.seg] + U.start : P.in + U.off;
  const __amdgpu_buffer_rsrc_t rin = unit_rsrc(xin, U.len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(DELTA ? P.base + U.off : xin, U.len);
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    const int boff = (int)((it * 64 + lane) * 16);
    const u4v a = __builtin_amdgcn_raw_buffer_load_b128(rin, boff, 0, AUX);
    v[it] = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
    if (DELTA) {
      const u4v b = __builtin_amdgcn_raw_buffer_load_b128(rb, boff, 0, AUX);
      v[it] = make_float4(v[it].x - __uint_as_float(b.x), v[it].y - __uint_as_float(b.y), v[it].z - __uint_as_float(b.z),
                          v[it].w - __uint_as_float(b.w));
    }
  }
}

// The dense quantise of one value (k_dense_quant, k_dense_block_quant). RCP: (x - mn) / scale as q = RN(a * y),
// y = RN(1 / scale), then q + RN(a - q * scale) * y by two FMAs — the correctly rounded quotient (Markstein) when
// neither the residual nor the quotient leaves the normal range, which scale in [2^-90, 2^90] ensures wherever the code
// is not 0 (t >= 0.5 needs a >= 2^-91); below that both round to code 0. The caller picks RCP for such a scale (a
// wave-uniform branch) and the IEEE division of `quantize` otherwise (scale 0, NaN, inf or extreme).
DEV bool dense_rcp_scale(float scale) { return scale >= 0x1p-90f && scale <= 0x1p90f; }
template <bool RCP>
DEV uint32_t dense_code(float x, float mn, float scale, float y, float levels) {
  if (!RCP) return quantize(x, mn, scale, levels);
  const float a = x - mn;
  const float q = a * y;
  const float t = __builtin_fmaf(__builtin_fmaf(-q, scale, a), y, q);
  const float rt = rintf(t);
  if (!(rt > 0.0f)) return 0u;
  return (uint32_t)(uint8_t)(rt < levels ? rt : levels);
}

// ... and that choice, made once per wave: f(qz) runs with qz(x) = dense_code<RCP> of the range, RCP a compile-time
// value inside f (two copies of f's straight-line loop behind one wave-uniform branch)
template <class F>
DEV void with_rcp(float mn, float scale, float levels, F&& f) {
  auto run = [&](auto rcp_tag) {
    constexpr bool RCP = decltype(rcp_tag)::value;
    const float y = RCP ? 1.0f / scale : 0.0f;
    f([&](float x) -> uint32_t { return dense_code<RCP>(x, mn, scale, y, levels); });
  };
  if (dense_rcp_scale(scale))  // (scale 0, NaN, inf or extreme: the division)
    run(std::true_type{});
  else
    run(std::false_type{});
}

// Stochastic (unbiased) rounding of the dense quantisers, the one copy of its contract, host and
// device: element c (its flat position, the segment's in_off + its index) of a call with the 64-bit `seed` draws 24
// uniform bits from three rounds of the lowbias32 mixer — two over the seed and the high word of c (sr_key: the same
// for every element of a unit that crosses no 2^32 boundary), one over the low word — and its code is floor(t) or
// floor(t) + 1, the latter with probability t - floor(t) (exact in fp32; an integer t is kept).
#define HOSTDEV __host__ __device__ __forceinline__
HOSTDEV uint32_t sr_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
HOSTDEV uint32_t sr_key(uint64_t seed, uint32_t c_hi) {
  return sr_mix(sr_mix(c_hi ^ (uint32_t)(seed >> 32) ^ 0x9E3779B9u) ^ (uint32_t)seed);
}
HOSTDEV uint32_t sr_u24_keyed(uint32_t key, uint32_t c_lo) { return sr_mix(c_lo ^ key) >> 8; }
HOSTDEV uint32_t sr_u24(uint64_t seed, uint64_t c) { return sr_u24_keyed(sr_key(seed, (uint32_t)(c >> 32)), (uint32_t)c); }
// t: the IEEE quotient (v - mn) / scale (the caller gives 0 where !(scale > 0)); u24: sr_u24's draw
HOSTDEV uint32_t sr_code(float t, uint32_t u24, float levels) {
  if (!(t > 0.0f)) return 0u;  // (NaN, v == mn)
  if (t >= levels) return (uint32_t)levels;
  const float f = floorf(t);
  return (uint32_t)f + (((float)u24 * 0x1p-24f < t - f) ? 1u : 0u);
}

// with_rcp for a caller that rounds the quotient itself: f(tq) runs with tq(x) = the IEEE quotient (x - mn) / scale,
// bit for bit, or 0 where !(scale > 0). The product form stands for the division only where tools/rcp_div_check.c
// found them equal — scale in [2^-90, 2^90] and x - mn >= 2^-100 (or 0: both forms give 0); below that round-to-nearest
// cannot tell them apart (both codes are 0) but a stochastic code can, so `proven` (dense_unit_proven, wave-uniform)
// sends a unit that holds such a value to the division.
template <class F>
DEV void with_rcp_quotient(float mn, float scale, bool proven, F&& f) {
  auto run = [&](auto rcp_tag) {
    constexpr bool RCP = decltype(rcp_tag)::value;
    const float y = RCP ? 1.0f / scale : 0.0f;
    const bool pos = scale > 0.0f;
    f([&](float x) -> float {
      const float a = x - mn;
      if (!RCP) return pos ? a / scale : 0.0f;
      const float q = a * y;
      return __builtin_fmaf(__builtin_fmaf(-q, scale, a), y, q);
    });
  };
  if (dense_rcp_scale(scale) && proven)
    run(std::true_type{});
  else
    run(std::false_type{});
}

// no value of the loaded unit has 0 < x - mn < 2^-100 (the bit pattern of x - mn, minus one, is below that of 2^-100
// minus one exactly there: a negative or NaN difference has the high bits set); the same answer in every lane. The
// positions past the unit's end hold 0.0f: they can only send the unit to the division, which is always right.
DEV bool dense_unit_proven(const float4 (&v)[UNIT_IT], float mn) {
  uint32_t m = 0xFFFFFFFFu;
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t b = __float_as_uint(xs[j] - mn) - 1u;
      m = b < m ? b : m;
    }
  }
  return __ballot(m < __float_as_uint(0x1p-100f) - 1u) == 0;
}

// A unit's stochastic-rounding key: sr_key of the high word of its first element's position c0 = in_off + start, from
// the scalar unit when the unit's last element shares that word (wave-uniform), else `carry` tells each lane whether
// its element's low word has wrapped (c_lo < c0's) and it takes the next word's key.
struct SrUnit {
  uint32_t lo, key, key1;
  bool split;
};
DEV SrUnit sr_unit(uint64_t seed, uint64_t c0, uint32_t len) {
  SrUnit s;
  s.lo = (uint32_t)c0;
  const uint32_t hi = (uint32_t)(c0 >> 32);
  s.split = (uint32_t)((c0 + len - 1u) >> 32) != hi;
  s.key = sr_key(seed, hi);
  s.key1 = s.split ? sr_key(seed, hi + 1u) : s.key;
  return s;
}
DEV uint32_t sr_draw(const SrUnit& s, uint32_t e) {
  const uint32_t c = s.lo + e;
  return sr_u24_keyed(s.split && c < s.lo ? s.key1 : s.key, c);
}

// the NaN-ignoring min / max of a loaded unit over the whole wave (every lane gets both)
DEV void dense_unit_minmax(const float4 (&v)[UNIT_IT], uint32_t len, uint32_t lane, float& a, float& b) {
  a = qnan(), b = qnan();
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    const uint32_t e0 = (it * 64 + lane) * 4;
    const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x = (len == UNIT || e0 + j < len) ? xs[j] : qnan();  // (loads past len read 0)
      a = fmin_nan(a, x);
      b = fmax_nan(b, x);
    }
  }
  a = wave_min(a);
  b = wave_max(b);
}

// ... and of NR of its rows from row r0 on: a block of G = 256 NR elements below the unit. Rows past
// the unit's end give NaN / NaN (no such block exists: its range is neither written nor read).
template <uint32_t NR>
DEV void dense_rows_minmax(const float4 (&v)[UNIT_IT], uint32_t r0, uint32_t len, uint32_t lane, float& a, float& b) {
  a = qnan(), b = qnan();
#pragma unroll
  for (uint32_t it = r0; it < r0 + NR; ++it) {
    const uint32_t e0 = (it * 64 + lane) * 4;
    const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x = (len == UNIT || e0 + j < len) ? xs[j] : qnan();  // (loads past len read 0)
      a = fmin_nan(a, x);
      b = fmax_nan(b, x);
    }
  }
  a = wave_min(a);
  b = wave_max(b);
}

// The index of a unit's first G-element block in the range arrays: gb[s] blocks precede segment s
// (the plan's table for G), UNIT / G of them every whole unit before this one. From the plan, never from a payload.
template <uint32_t G>
DEV uint64_t dense_block_index(const uint64_t* __restrict__ gb, const UnitDev& U) {
  return gb[U.seg] + (uint64_t)(U.start >> UNIT_SHIFT) * (UNIT / G);
}

// A dense unit's codes sit at the positions themselves (k == n: entry e is element e): its first entry in vals, and
// whether its codes can move as whole dwords — they start 4-byte aligned (16-byte for raw floats) and end on a dword.
// The one copy: every kernel that reads or writes a unit's codes takes the same branch.
DEV uint64_t dense_unit_entry(const UnitDev& U) { return U.out_off + U.start; }
DEV bool dense_unit_vec(const UnitDev& U) {
  const uint64_t o = dense_unit_entry(U);
  return (o & 3u) == 0 && (U.len & 3u) == 0;
}

// Four codes of a unit at byte offset boff of the resource over its `len` codes (bytes_rsrc): one dword where the
// unit's codes are whole dwords (vec), else four range-checked bytes — a load past len gives 0, a store there is dropped.
DEV uint32_t dense_codes_row(__amdgpu_buffer_rsrc_t r, bool vec, uint32_t boff) {
  if (vec) return __builtin_amdgcn_raw_buffer_load_b32(r, (int)boff, 0, 0);
  return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, (int)boff, 0, 0) |
         ((uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, (int)boff + 1, 0, 0) << 8) |
         ((uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, (int)boff + 2, 0, 0) << 16) |
         ((uint32_t)__builtin_amdgcn_raw_buffer_load_b8(r, (int)boff + 3, 0, 0) << 24);
}

DEV void dense_codes_store_row(__amdgpu_buffer_rsrc_t r, bool vec, uint32_t boff, const uint32_t (&c)[4]) {
  if (vec) {
    __builtin_amdgcn_raw_buffer_store_b32(c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24), r, (int)boff, 0, 0);
  } else {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)c[j], r, (int)(boff + j), 0, 0);
  }
}

// The end of every dense decoder, one row (lane l's float4 of row `row`) at a time: base + x, and the store — 16 bytes
// where the unit's length is a multiple of four, else four dwords, the range check dropping those past the end.
DEV float4 dense_add_base(float4 b, float4 x) { return make_float4(b.x + x.x, b.y + x.y, b.z + x.z, b.w + x.w); }
template <int AUX = STORE_AUX>
DEV void dense_store_row(__amdgpu_buffer_rsrc_t rout, uint32_t len, uint32_t row, uint32_t lane, float4 x) {
  if ((len & 3u) == 0)
    unit_store_x4<AUX>(rout, (row * 64 + lane) * 16, x);
  else
    unit_store_x1x4<AUX>(rout, (row * 64 + lane) * 16, x);
}

template <bool DELTA, bool XCD>
__global__ __launch_bounds__(BLOCK) void k_dense_minmax(Params P) {
  const uint32_t u = (XCD ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  float4 v[UNIT_IT];
  dense_unit_load<DELTA, DENSE_MM_AUX>(P, U, v);
  const uint32_t lane = lane_id();
  float a, b;
  dense_unit_minmax(v, U.len, lane, a, b);
  if (lane == 0) {
    P.umm[2 * u] = a;
    P.umm[2 * u + 1] = b;
  }
}

// one block per segment: its units' partial min / max -> mn, scale (CodecSpec v1: each + 0.0f; scale 0 when
// they are equal); raw values (bits 32): mn = scale = 0
template <bool RAW>
__global__ __launch_bounds__(BLOCK) void k_dense_seg(Params P) {
  __shared__ float shf[2 * WAVES];
  const uint32_t s = blockIdx.x;
  const SegDev sd = P.segs[s];
  float a = qnan(), b = qnan();
  if (!RAW)
    for (uint32_t u = sd.unit_begin + threadIdx.x; u < sd.unit_end; u += BLOCK) {
      a = fmin_nan(a, P.umm[2 * u]);
      b = fmax_nan(b, P.umm[2 * u + 1]);
    }
  block_minmax<BLOCK>(a, b, shf);
  if (threadIdx.x == 0) {
    float mn = 0.0f, scale = 0.0f;
    if (!RAW && sd.n != 0) codec_range(a, b, P.levels, mn, scale);
    P.mn[s] = mn;
    P.scale[s] = scale;
  }
}

// SEGRED: every wave reduces its segment's per-unit min / max itself (k_dense_seg folded in: the unit's loads are in
// flight meanwhile, the ~50 KB of pairs are L2-resident, and one launch boundary goes); the segment's first unit
// writes its mn / scale. Used when every segment has a unit (an empty segment has no wave to write its zeros).
// SR: stochastic rounding with the call's `seed`: the same loads, range and stores, each code from
// sr_code of the IEEE quotient and the element's own draw (the integer hash is issued behind the unit's loads).
template <bool DELTA, bool RAW, bool XCD, bool SEGRED, bool SR>
DEV void dense_quant_unit(const Params& P, uint64_t seed) {
  const uint32_t u = (XCD ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id();
  // SEGRED: the first SEGRED_PAIRS x 64 units' min / max pairs are loaded ahead of the unit's own loads (straight-line
  // code: the reduce waits for them alone, the unit's loads still in flight); a longer segment's remainder afterwards
  constexpr uint32_t SEGRED_PAIRS = 8;
  SegDev sd{};
  float2 m[SEGRED_PAIRS];
  const float2* umm2 = reinterpret_cast<const float2*>(P.umm);
  if (SEGRED) {
    sd = P.segs[U.seg];
    if (!RAW) {
#pragma unroll
      for (uint32_t j = 0; j < SEGRED_PAIRS; ++j) {
        const uint32_t w = sd.unit_begin + j * 64 + lane;
        m[j] = w < sd.unit_end ? umm2[w] : make_float2(qnan(), qnan());
      }
    }
  }
  float4 v[UNIT_IT];
  dense_unit_load<DELTA, DENSE_Q_AUX>(P, U, v);
  float mn = 0.0f, scale = 0.0f;
  if (SEGRED) {
    if (!RAW) {  // (same NaN-ignoring min / max and + 0.0f as k_dense_seg: order-independent, bit-identical)
      float a = qnan(), b = qnan();
#pragma unroll
      for (uint32_t j = 0; j < SEGRED_PAIRS; ++j) {
        a = fmin_nan(a, m[j].x);
        b = fmax_nan(b, m[j].y);
      }
      for (uint32_t w = sd.unit_begin + SEGRED_PAIRS * 64 + lane; w < sd.unit_end; w += 64) {
        const float2 t = umm2[w];
        a = fmin_nan(a, t.x);
        b = fmax_nan(b, t.y);
      }
      codec_range(wave_min(a), wave_max(b), P.levels, mn, scale);
    }
    if (u == sd.unit_begin && lane == 0) {
      P.mn[U.seg] = mn;
      P.scale[U.seg] = scale;
    }
  } else if (!RAW) {
    mn = P.mn[U.seg];
    scale = P.scale[U.seg];
  }
  const uint64_t o = dense_unit_entry(U);
  const bool vec = dense_unit_vec(U);
  if (RAW) {
    const __amdgpu_buffer_rsrc_t r = unit_rsrc(static_cast<float*>(P.vals) + o, U.len);
#pragma unroll
    for (uint32_t it = 0; it < UNIT_IT; ++it) {
      if (vec)
        unit_store_x4<0>(r, (it * 64 + lane) * 16, v[it]);
      else
        unit_store_x1x4<0>(r, (it * 64 + lane) * 16, v[it]);
    }
  } else {
    const __amdgpu_buffer_rsrc_t r = bytes_rsrc(static_cast<uint8_t*>(P.vals) + o, U.len);
    // dense_code's reciprocal form: the IEEE division sequence it replaces cost 3.5 us of the download step
    // (profiles/r06_ab_dense_segred.txt)
    if constexpr (SR) {
      const SrUnit sr = sr_unit(seed, U.off, U.len);
      with_rcp_quotient(mn, scale, dense_rcp_scale(scale) && dense_unit_proven(v, mn), [&](auto tq) {
#pragma unroll
        for (uint32_t it = 0; it < UNIT_IT; ++it) {
          const uint32_t e0 = (it * 64 + lane) * 4;
          const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
          uint32_t c[4];
#pragma unroll
          for (uint32_t j = 0; j < 4; ++j) c[j] = sr_code(tq(xs[j]), sr_draw(sr, e0 + j), P.levels);
          dense_codes_store_row(r, vec, e0, c);
        }
      });
    } else {
      with_rcp(mn, scale, P.levels, [&](auto qz) {
#pragma unroll
        for (uint32_t it = 0; it < UNIT_IT; ++it) {
          const uint32_t c[4] = {qz(v[it].x), qz(v[it].y), qz(v[it].z), qz(v[it].w)};
          dense_codes_store_row(r, vec, (it * 64 + lane) * 4, c);
        }
      });
    }
  }
  if (P.idx != nullptr) {  // a caller that asked for the (implied) indices
    for (uint32_t e = lane; e < U.len; e += 64) P.idx[o + e] = (int32_t)(U.start + e);
  }
  if (P.ustart_out != nullptr && lane == 0) P.ustart_out[u] = U.start;
}

template <bool DELTA, bool RAW, bool XCD, bool SEGRED>
__global__ __launch_bounds__(BLOCK) void k_dense_quant(Params P) {
  dense_quant_unit<DELTA, RAW, XCD, SEGRED, false>(P, 0);
}

template <bool DELTA, bool XCD, bool SEGRED>
__global__ __launch_bounds__(BLOCK) void k_dense_quant_sr(Params P, uint64_t seed) {
  dense_quant_unit<DELTA, false, XCD, SEGRED, true>(P, seed);
}

// the decoded values of four uint8 codes in one dword (dense_codes_row)
DEV float4 dense_codes_values(uint32_t w, float mn, float scale) {
  return make_float4(dequantize((uint8_t)(w & 0xFFu), mn, scale), dequantize((uint8_t)((w >> 8) & 0xFFu), mn, scale),
                     dequantize((uint8_t)((w >> 16) & 0xFFu), mn, scale), dequantize((uint8_t)(w >> 24), mn, scale));
}

// the decoded values of a dense plan's unit (its codes sit at the positions themselves): lane l's float4 of row it
// in d[it]; positions past the unit's end hold mn (code 0) or 0.0f (raw) and are never stored
template <bool RAW>
DEV void dense_unit_values(const Params& P, const UnitDev& U, float mn, float scale, uint32_t lane, float4 (&d)[UNIT_IT]) {
  const uint64_t o = dense_unit_entry(U);
  const bool vec = dense_unit_vec(U);
  if (RAW) {
    const float* src = static_cast<const float*>(P.cvals) + o;
    const __amdgpu_buffer_rsrc_t r = unit_rsrc(src, U.len);
#pragma unroll
    for (uint32_t it = 0; it < UNIT_IT; ++it) {
      if (vec) {
        d[it] = unit_load_x4<false>(r, r, (it * 64 + lane) * 16);
      } else {
        const uint32_t b = (it * 64 + lane) * 16;
        d[it] = make_float4(__uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)b, 0, 0)),
                            __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)b + 4, 0, 0)),
                            __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)b + 8, 0, 0)),
                            __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)b + 12, 0, 0)));
      }
    }
  } else {
    const __amdgpu_buffer_rsrc_t r = bytes_rsrc(static_cast<const uint8_t*>(P.cvals) + o, U.len);
    uint32_t w[UNIT_IT];
#pragma unroll
    for (uint32_t it = 0; it < UNIT_IT; ++it) w[it] = dense_codes_row(r, vec, (it * 64 + lane) * 4);
#pragma unroll
    for (uint32_t it = 0; it < UNIT_IT; ++it) d[it] = dense_codes_values(w[it], mn, scale);
  }
}

template <bool RAW, bool HASBASE, bool XCD>
__global__ __launch_bounds__(BLOCK) void k_dense_deq(Params P) {
  const uint32_t u = (XCD ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id();
  const float mn = RAW ? 0.0f : P.cmn[U.seg], scale = RAW ? 0.0f : P.cscale[U.seg];
  float4 d[UNIT_IT];
  dense_unit_values<RAW>(P, U, mn, scale, lane, d);
  const __amdgpu_buffer_rsrc_t rout = unit_rsrc(P.out + U.off, U.len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(HASBASE ? P.base + U.off : P.out + U.off, U.len);
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    float4 x = d[it];
    if (HASBASE) x = dense_add_base(unit_load_x4<false>(rb, rb, (it * 64 + lane) * 16), x);
    dense_store_row(rout, U.len, it, lane, x);
  }
}

// ------------------------------------------------------------------------------------------------
// error feedback (client side): the residual memory of a top-k upload, DESIGN.md §11
//   k_ef_accumulate  r = (x - base) + r over every unit of the plan (fp32 subtract, then fp32 add): the encoder then
//                    runs on r as a plain input
//   k_ef_commit      r[pos] = r[pos] - xhat at every kept entry (xhat: code_value, the decoder's own arithmetic), +0.0f
//                    where that is not finite; positions not kept still hold the accumulated value, which IS the residual
// ------------------------------------------------------------------------------------------------
constexpr uint32_t EF_ROWS = 4u;   // rows (float4 per lane) of each operand in flight per k_ef_accumulate wave: 12 b128
                                   // loads per lane with a base, and few enough registers for 8 waves per SIMD
constexpr int EF_STORE_AUX = 0;    // cache policy of the residual's stores (0 plain, 2 non-temporal): the encode reads
                                   // them next (A/B in DESIGN.md §11)

template <bool HASBASE>
__global__ __launch_bounds__(BLOCK) void k_ef_accumulate(Params P) {
  static_assert(UNIT_IT % EF_ROWS == 0, "accumulate batch geometry");
  const uint32_t u = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id(), len = U.len;
  const float* x = P.inptr != nullptr ? P.inptr[U.seg] + U.start : P.in + U.off;
  // range-checked operands: a load past the unit's end gives 0, a store past it is dropped (the padding between
  // segments is never written)
  const __amdgpu_buffer_rsrc_t rx = unit_rsrc(x, len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(HASBASE ? P.base + U.off : x, len);
  const __amdgpu_buffer_rsrc_t rr = unit_rsrc(P.out + U.off, len);
  const uint32_t rows = (len + 255u) >> 8;  // rows that hold elements (wave-uniform)
  for (uint32_t i0 = 0; i0 < rows; i0 += EF_ROWS) {
    float4 d[EF_ROWS], r[EF_ROWS];
#pragma unroll
    for (uint32_t it = 0; it < EF_ROWS; ++it) {
      const uint32_t b = ((i0 + it) * 64 + lane) * 16;
      d[it] = unit_load_x4<HASBASE>(rx, rb, b);
      r[it] = unit_load_x4<false>(rr, rr, b);
    }
#pragma unroll
    for (uint32_t it = 0; it < EF_ROWS; ++it) {
      const float4 a = make_float4(d[it].x + r[it].x, d[it].y + r[it].y, d[it].z + r[it].z, d[it].w + r[it].w);
      dense_store_row<EF_STORE_AUX>(rr, len, i0 + it, lane, a);
    }
  }
}

// a - xhat, or +0.0f when that is NaN or +-Inf (a diverged element must not stay in the memory)
DEV float ef_residual(float a, float xhat) {
  const float v = a - xhat;
  return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u ? 0.0f : v;
}

// one wave per unit; the unit's entry range from the per-unit starts, clamped as k_decode_lds clamps it; a lane takes
// one entry at a time (two rounds of 64 in flight). An entry whose position lies outside the unit (never from this
// library's encoder) is dropped.
template <bool RAW>
__global__ __launch_bounds__(BLOCK) void k_ef_commit(Params P) {
  const uint32_t u = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const uint32_t lane = lane_id();
  const UnitDev U = P.units[u];
  uint32_t lo = P.ustart[u];
  uint32_t hi = P.ustart[min(u + 1, P.n_units - 1)];
  const float mn = RAW ? 0.0f : P.cmn[U.seg], sc = RAW ? 0.0f : P.cscale[U.seg];
  lo = min(lo, U.k);
  hi = max(lo, min(min(U.last ? U.k : hi, U.k), lo + U.len));
  float* r = P.out + U.off;
  for (uint32_t e0 = lo; e0 < hi; e0 += 128) {
    uint32_t pos[2], q[2];
    float a[2];
    bool ok[2];
#pragma unroll
    for (uint32_t c = 0; c < 2; ++c) {
      const uint32_t ei = e0 + c * 64 + lane;
      const uint64_t e = U.out_off + min(ei, hi - 1);
      pos[c] = (uint32_t)P.cidx[e] - U.start;
      q[c] = load_code<RAW>(P, e);
      ok[c] = ei < hi && pos[c] < U.len;
    }
#pragma unroll
    for (uint32_t c = 0; c < 2; ++c)
      if (ok[c]) a[c] = r[pos[c]];
#pragma unroll
    for (uint32_t c = 0; c < 2; ++c)
      if (ok[c]) r[pos[c]] = ef_residual(a[c], code_value<RAW>(q[c], mn, sc));
  }
}

// a dense plan: every position is a kept entry, taken positionally
template <bool RAW>
__global__ __launch_bounds__(BLOCK) void k_ef_commit_dense(Params P) {
  const uint32_t u = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id();
  const float mn = RAW ? 0.0f : P.cmn[U.seg], scale = RAW ? 0.0f : P.cscale[U.seg];
  float4 d[UNIT_IT];
  dense_unit_values<RAW>(P, U, mn, scale, lane, d);
  const __amdgpu_buffer_rsrc_t rr = unit_rsrc(P.out + U.off, U.len);
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    const float4 a = unit_load_x4<false>(rr, rr, (it * 64 + lane) * 16);
    const float4 v = make_float4(ef_residual(a.x, d[it].x), ef_residual(a.y, d[it].y), ef_residual(a.z, d[it].z),
                                 ef_residual(a.w, d[it].w));
    dense_store_row<EF_STORE_AUX>(rr, U.len, it, lane, v);
  }
}

// ------------------------------------------------------------------------------------------------
// compact payload (wire v3): entry j of the plan's idx / vals arrays as one (12 + B)-bit field
//   field_j = (idx[j] & 0xFFF) | (code_j << 12)      B = bits (<= 8), or 0 at bits 32 (the fp32 values stay apart)
// in a little-endian bit stream of uint32 words: field j occupies bits [j w, (j + 1) w), bit t of the stream is bit
// t % 32 of word t / 32. The upper index bits are the entry's unit number, which the per-unit starts carry already.
//   k_pack    a flat stream over the positions [0, total_k): a lane owns 32 consecutive entries = w whole words
//   k_unpack  one wave per unit of the plan's table, its entry range from the starts (clamped as k_decode_lds clamps)
// ------------------------------------------------------------------------------------------------
constexpr uint32_t PACK_E = 32;  // entries per k_pack lane: 32 fields of w bits are exactly w words

// N fields of W bits each as the N W / 32 whole words of a little-endian bit stream (k_pack, k_pack_dense). Fully
// unrolled: nb and wi are compile-time values, f[] and word[] stay in registers.
template <uint32_t W, uint32_t N>
DEV void pack_fields(const uint32_t (&f)[N], uint32_t (&word)[W * N / 32u]) {
  static_assert(W * N % 32u == 0, "whole words");
  uint64_t acc = 0;
  uint32_t nb = 0, wi = 0;
#pragma unroll
  for (uint32_t i = 0; i < N; ++i) {
    acc |= (uint64_t)f[i] << nb;
    nb += W;
    if (nb >= 32u) {
      word[wi++] = (uint32_t)acc;
      acc >>= 32;
      nb -= 32u;
    }
  }
}

// B: code bits (0 = none: a raw plan's values are not read). idx and vals are 16-byte aligned (checked by the entry
// point), so a full lane reads its 32 indices as eight b128 loads and its 32 codes as two.
template <uint32_t B>
__global__ __launch_bounds__(BLOCK) void k_pack(const int32_t* __restrict__ idx, const uint8_t* __restrict__ vals,
                                                uint32_t* __restrict__ out, uint64_t K) {
  constexpr uint32_t W = 12u + B;
  const uint64_t t = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const uint64_t j0 = t * PACK_E;
  if (j0 >= K) return;
  const uint32_t cnt = (uint32_t)min((uint64_t)PACK_E, K - j0);
  uint32_t f[PACK_E];
  if (cnt == PACK_E) {
    const int4* pi = reinterpret_cast<const int4*>(idx + j0);
#pragma unroll
    for (uint32_t i = 0; i < PACK_E / 4; ++i) {
      const int4 v = pi[i];
      f[4 * i + 0] = (uint32_t)v.x & 0xFFFu;
      f[4 * i + 1] = (uint32_t)v.y & 0xFFFu;
      f[4 * i + 2] = (uint32_t)v.z & 0xFFFu;
      f[4 * i + 3] = (uint32_t)v.w & 0xFFFu;
    }
    if (B != 0) {
      const uint4* pv = reinterpret_cast<const uint4*>(vals + j0);
#pragma unroll
      for (uint32_t i = 0; i < PACK_E / 16; ++i) {
        const uint4 v = pv[i];
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t c = 0; c < 16; ++c) f[16 * i + c] |= ((q[c >> 2] >> ((c & 3u) * 8u)) & ((1u << B) - 1u)) << 12;
      }
    }
  } else {  // the stream's last lane: entries past total_k are zero fields (the tail word's padding)
#pragma unroll
    for (uint32_t i = 0; i < PACK_E; ++i) {
      f[i] = 0u;
      if (i < cnt) {
        f[i] = (uint32_t)idx[j0 + i] & 0xFFFu;
        if (B != 0) f[i] |= ((uint32_t)vals[j0 + i] & ((1u << B) - 1u)) << 12;
      }
    }
  }
  uint32_t word[W];
  pack_fields<W, PACK_E>(f, word);
  const uint32_t nw = (cnt * W + 31u) >> 5;  // words this lane owns (W for a full lane); every one written once
  uint32_t* o = out + t * W;
#pragma unroll
  for (uint32_t i = 0; i < W; ++i)
    if (i < nw) o[i] = word[i];
}

// one wave per unit, one lane per entry: the field's one or two words (the second only when the field straddles a
// word and the word lies inside the stream's nwords), then idx = unit start | low 12 bits, vals = code. Whatever the
// starts say, lo <= e < hi <= k: only positions out_off + [0, k) of the unit's own segment are written.
template <bool RAW>
__global__ __launch_bounds__(BLOCK) void k_unpack(Params P, const uint32_t* __restrict__ packed, uint64_t nwords,
                                                  uint32_t w) {
  const uint32_t u = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const uint32_t lane = lane_id();
  const UnitDev U = P.units[u];
  uint32_t lo = P.ustart[u];
  uint32_t hi = P.ustart[min(u + 1, P.n_units - 1)];
  lo = min(lo, U.k);
  hi = max(lo, min(min(U.last ? U.k : hi, U.k), lo + U.len));
  const uint32_t mask = (1u << w) - 1u;
  uint8_t* vals = static_cast<uint8_t*>(P.vals);
  for (uint32_t e = lo + lane; e < hi; e += 64) {
    const uint64_t j = U.out_off + e;
    const uint64_t bit = j * w;
    const uint64_t wd = bit >> 5;
    const uint32_t sh = (uint32_t)bit & 31u;
    uint32_t v = packed[wd] >> sh;  // (wd < nwords: j < total_k and the stream holds total_k fields)
    if (sh + w > 32u && wd + 1 < nwords) v |= packed[wd + 1] << (32u - sh);
    v &= mask;
    P.idx[j] = (int32_t)(U.start | (v & 0xFFFu));
    if (!RAW) vals[j] = (uint8_t)(v >> 12);
  }
}

// ------------------------------------------------------------------------------------------------
// bit-packed dense codes (wire v4): a dense plan's uint8 codes as B-bit fields, B = bits (1..8)
//   segment s (plan row order) owns W_s = ceil(n_s B / 32) words at word offset pw_s = sum of W_t, t < s; entry e of
//   the segment (its code at vals[out_off_s + e]) occupies bits [e B, (e + 1) B) of that sub-stream, little-endian
//   (bit t is bit t % 32 of word t / 32), the last word's padding bits zero.
// A segment's sub-stream starts on a word, so does every 4096-element unit of it: unit u_s at word pw_s + 128 B u_s.
// One wave per unit owns whole words: plain stores, no atomics.
//   k_pack_dense     a lane takes 32-entry groups (two per unit): 32 codes -> B words
//   k_unpack_dense   the inverse: B words -> 32 codes, written inside vals[out_off_s + [0, n_s)) only
//   k_dense_deq_stream  k_dense_deq reading the stream itself: a lane's four elements of a row are 4 B bits; the
//                       range of an element its segment's (wire v4) or its unit's (wire v5, below)
// Shared pieces, one copy each: the unit's words (dense_unit_word_off: every kernel here, k_dense_block_quant,
// k_aggregate_dense; dense_unit_words_rsrc: the three kernels here), the unit's codes (dense_unit_entry / dense_unit_vec / dense_codes_row /
// dense_codes_store_row: the dense section's), a row of the stream (dense_row_words / dense_row_values:
// k_dense_deq_stream, k_aggregate_dense), the field accumulator (pack_fields: k_pack's).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t DPACK_E = 32;                      // entries per group: B whole words
constexpr uint32_t DPACK_G = UNIT / DPACK_E / 64;     // groups per lane per unit (2)

// where the unit's words start inside the stream and how many it owns (the segment's last unit: up to the segment's
// last word)
template <uint32_t B>
DEV uint64_t dense_unit_word_off(const uint64_t* pw, const UnitDev& U, uint32_t& nwords) {
  nwords = ((uint32_t)U.len * B + 31u) >> 5;
  return pw[U.seg] + (uint64_t)(UNIT / 32u * B) * (U.start >> UNIT_SHIFT);
}

// the resource over the unit's words: a load past them returns 0, a store there is dropped — never another segment's
// word or past the stream (they lie inside the segment's W_s). The one copy of the stream's addressing, with
// dense_row_words / dense_row_values below.
template <uint32_t B>
DEV __amdgpu_buffer_rsrc_t dense_unit_words_rsrc(const uint32_t* packed, const uint64_t* pw, const UnitDev& U) {
  uint32_t nwords;
  const uint64_t woff = dense_unit_word_off<B>(pw, U, nwords);
  return bytes_rsrc(packed + woff, nwords * 4u);
}

template <uint32_t B>
__global__ __launch_bounds__(BLOCK) void k_pack_dense(Params P, const uint64_t* __restrict__ pw,
                                                      const uint8_t* __restrict__ vals, uint32_t* __restrict__ packed) {
  const uint32_t u = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id();
  const bool vec = dense_unit_vec(U);
  // range-checked to the unit's codes: a group's tail past len reads 0, which is the padding
  const __amdgpu_buffer_rsrc_t rin = bytes_rsrc(vals + dense_unit_entry(U), U.len);
  const __amdgpu_buffer_rsrc_t rout = dense_unit_words_rsrc<B>(packed, pw, U);
  uint32_t q[DPACK_G][DPACK_E / 4];  // four codes per dword
#pragma unroll
  for (uint32_t g = 0; g < DPACK_G; ++g) {
    const uint32_t b0 = (g * 64 + lane) * DPACK_E;
    // The wave-uniform branch stands outside the loop on purpose: one loop over dense_codes_row(rin, vec, ...) compiles
    // to a branch per dword (about 100 instructions more per kernel, checked in the gfx950 assembly), not one per group.
    if (vec) {
#pragma unroll
      for (uint32_t i = 0; i < DPACK_E / 4; ++i) q[g][i] = dense_codes_row(rin, true, b0 + 4 * i);
    } else {
#pragma unroll
      for (uint32_t i = 0; i < DPACK_E / 4; ++i) q[g][i] = dense_codes_row(rin, false, b0 + 4 * i);
    }
  }
#pragma unroll
  for (uint32_t g = 0; g < DPACK_G; ++g) {
    uint32_t c[DPACK_E], word[B];
#pragma unroll
    for (uint32_t i = 0; i < DPACK_E; ++i) c[i] = (q[g][i >> 2] >> ((i & 3u) * 8u)) & ((1u << B) - 1u);
    pack_fields<B, DPACK_E>(c, word);
    const uint32_t w0 = (g * 64 + lane) * B;  // words past the unit's own are dropped by the range check
#pragma unroll
    for (uint32_t i = 0; i < B; ++i) __builtin_amdgcn_raw_buffer_store_b32(word[i], rout, (int)((w0 + i) * 4u), 0, 0);
  }
}

template <uint32_t B>
__global__ __launch_bounds__(BLOCK) void k_unpack_dense(Params P, const uint64_t* __restrict__ pw,
                                                        const uint32_t* __restrict__ packed, uint8_t* __restrict__ vals) {
  const uint32_t u = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id();
  const bool vec = dense_unit_vec(U);
  const __amdgpu_buffer_rsrc_t rin = dense_unit_words_rsrc<B>(packed, pw, U);
  // range-checked to the unit's codes: a store past len is dropped (only vals[out_off + [0, n)) is written)
  const __amdgpu_buffer_rsrc_t rout = bytes_rsrc(vals + dense_unit_entry(U), U.len);
  uint32_t w[DPACK_G][B + 1];
#pragma unroll
  for (uint32_t g = 0; g < DPACK_G; ++g) {
    const uint32_t w0 = (g * 64 + lane) * B;
#pragma unroll
    for (uint32_t i = 0; i < B; ++i) w[g][i] = __builtin_amdgcn_raw_buffer_load_b32(rin, (int)((w0 + i) * 4u), 0, 0);
    w[g][B] = 0u;
  }
#pragma unroll
  for (uint32_t g = 0; g < DPACK_G; ++g) {
    const uint32_t b0 = (g * 64 + lane) * DPACK_E;
#pragma unroll
    for (uint32_t d = 0; d < DPACK_E / 4; ++d) {
      uint32_t c[4];
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {  // (compile-time word and shift of entry 4 d + j)
        const uint32_t bit = (4 * d + j) * B, wd = bit >> 5, sh = bit & 31u;
        uint32_t v = w[g][wd] >> sh;
        if (sh + B > 32u) v |= w[g][wd + 1] << (32u - sh);
        c[j] = v & ((1u << B) - 1u);
      }
      dense_codes_store_row(rout, vec, b0 + 4 * d, c);
    }
  }
}

// A row of the stream: lane l's four elements of row `row` are the 4 B bits at bit (row * 64 + l) * 4 B of the unit's
// words — one word, or two when the field straddles (never for B = 1, 2, 4, 8); a field at the unit's end reads 0 past
// its words (dense_unit_words_rsrc). Shared by k_dense_deq_stream and k_aggregate_dense.
template <uint32_t B>
DEV void dense_row_words(__amdgpu_buffer_rsrc_t rin, uint32_t row, uint32_t lane, uint32_t& lo, uint32_t& hi) {
  constexpr bool STRADDLE = (32u % (4u * B)) != 0u;
  const uint32_t wd = ((row * 64 + lane) * 4u * B) >> 5;
  lo = __builtin_amdgcn_raw_buffer_load_b32(rin, (int)(wd * 4u), 0, 0);
  hi = STRADDLE ? __builtin_amdgcn_raw_buffer_load_b32(rin, (int)(wd * 4u + 4u), 0, 0) : 0u;
}

template <uint32_t B>
DEV float4 dense_row_values(uint32_t lo, uint32_t hi, uint32_t row, uint32_t lane, float mn, float scale) {
  const uint32_t sh = ((row * 64 + lane) * 4u * B) & 31u;
  const uint32_t f = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
  constexpr uint32_t M = (1u << B) - 1u;
  return make_float4(dequantize((uint8_t)(f & M), mn, scale), dequantize((uint8_t)((f >> B) & M), mn, scale),
                     dequantize((uint8_t)((f >> (2 * B)) & M), mn, scale),
                     dequantize((uint8_t)((f >> (3 * B)) & M), mn, scale));
}

// Which range (mn, scale) decodes an element of a stream: its unit's own (PERUNIT: wire v5, block-wise) or its
// segment's (wire v4). The one copy of the rule, for k_dense_deq_stream and k_aggregate_dense.
template <bool PERUNIT>
DEV uint32_t dense_range_index(uint32_t u, const UnitDev& U) {
  return PERUNIT ? u : U.seg;
}

// k_dense_deq with its values read from the dense stream, the ranges at rmn / rscale [dense_range_index]: wire v4's
// decode (PERUNIT false: one range per segment) and wire v5's (true: one per unit) are this one kernel. Same
// dequantize, base + x and stores as k_dense_deq.
template <uint32_t B, bool PERUNIT, bool HASBASE, bool XCD>
__global__ __launch_bounds__(BLOCK) void k_dense_deq_stream(Params P, const uint64_t* __restrict__ pw,
                                                            const uint32_t* __restrict__ packed,
                                                            const float* __restrict__ rmn,
                                                            const float* __restrict__ rscale) {
  const uint32_t u = (XCD ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id(), ri = dense_range_index<PERUNIT>(u, U);
  const float mn = rmn[ri], scale = rscale[ri];
  const __amdgpu_buffer_rsrc_t rin = dense_unit_words_rsrc<B>(packed, pw, U);
  uint32_t lo[UNIT_IT], hi[UNIT_IT];
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) dense_row_words<B>(rin, it, lane, lo[it], hi[it]);
  const __amdgpu_buffer_rsrc_t rout = unit_rsrc(P.out + U.off, U.len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(HASBASE ? P.base + U.off : P.out + U.off, U.len);
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    float4 x = dense_row_values<B>(lo[it], hi[it], it, lane, mn, scale);
    if (HASBASE) x = dense_add_base(unit_load_x4<false>(rb, rb, (it * 64 + lane) * 16), x);
    dense_store_row(rout, U.len, it, lane, x);
  }
}

// k_dense_deq_stream for G-element blocks below the unit: a row takes the range of its block, at
// dense_block_index (gb: the plan's block table for G) — UNIT / G wave-uniform pairs per unit, those of blocks past the
// unit's end not read. A kernel of its own: the 4096 kernel above keeps its registers.
template <uint32_t B, bool HASBASE, bool XCD, uint32_t G>
__global__ __launch_bounds__(BLOCK) void k_dense_deq_stream_g(Params P, const uint64_t* __restrict__ pw,
                                                              const uint64_t* __restrict__ gb,
                                                              const uint32_t* __restrict__ packed,
                                                              const float* __restrict__ rmn,
                                                              const float* __restrict__ rscale) {
  static_assert(G == 256u || G == 1024u, "blocks below the unit: 256 or 1024 elements");
  constexpr uint32_t NBU = UNIT / G, RB = G / 256u;  // blocks per unit, rows per block
  // (the unit as a scalar, as k_aggregate_dense's: the unit's record and its ranges are then scalar loads)
  const uint32_t u =
      __builtin_amdgcn_readfirstlane((XCD ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6));
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id();
  const uint64_t g0 = dense_block_index<G>(gb, U);
  float mn[NBU], scale[NBU];
#pragma unroll
  for (uint32_t j = 0; j < NBU; ++j) {
    const bool there = j * G < U.len;  // (wave-uniform; a block past the end: its rows are never stored)
    mn[j] = there ? rmn[g0 + j] : 0.0f;
    scale[j] = there ? rscale[g0 + j] : 0.0f;
  }
  const __amdgpu_buffer_rsrc_t rin = dense_unit_words_rsrc<B>(packed, pw, U);
  uint32_t lo[UNIT_IT], hi[UNIT_IT];
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) dense_row_words<B>(rin, it, lane, lo[it], hi[it]);
  const __amdgpu_buffer_rsrc_t rout = unit_rsrc(P.out + U.off, U.len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(HASBASE ? P.base + U.off : P.out + U.off, U.len);
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    float4 x = dense_row_values<B>(lo[it], hi[it], it, lane, mn[it / RB], scale[it / RB]);
    if (HASBASE) x = dense_add_base(unit_load_x4<false>(rb, rb, (it * 64 + lane) * 16), x);
    dense_store_row(rout, U.len, it, lane, x);
  }
}

// ------------------------------------------------------------------------------------------------
// block-wise dense quantisation (wire v5): every 4096-element unit of a dense plan is quantised over its
// OWN range — CodecSpec v1 applied to the unit as if it were a segment with k = n — and the codes leave as wire v4's
// B-bit stream, in one pass: no min / max pre-pass, no segment reduce, no byte-per-element intermediate.
//   k_dense_block_quant  one wave per unit: load (16 float4 per lane), the wave's NaN-ignoring min / max -> bmn[u],
//                        bscale[u], quantise (dense_code: k_dense_quant's arithmetic), emit the unit's words
//   the decode is k_dense_deq_stream<PERUNIT> with (mn, scale) = (bmn[u], bscale[u])
// Emission: lane l's four codes of row it are one 4 B-bit field, field f = it * 64 + l at bit 4 B f of the unit's
// sub-stream. The wave writes its 1024 fields to its own 4 KB of LDS, then lane l builds the words l, l + 64, ... of
// the unit (128 B of them) from the fields that overlap each — 8 / B fields where 4 B divides 32, at most 1 +
// ceil(31 / 4 B) otherwise — and stores every word whole, consecutive lanes consecutive dwords. The stores are range-
// checked to the unit's ceil(len B / 32) words, which lie inside its segment's [pw_s, pw_s + W_s).
// ------------------------------------------------------------------------------------------------
// The fused error feedback's unit: v = (x - base) + r, k_ef_accumulate's arithmetic (fp32 subtract, then
// fp32 add), EF_ROWS rows of each operand in flight as there. The operands are range-checked to the unit: a load past
// its end gives 0. x and base are read once (non-temporal, as the quantise stream's); r is read with the default policy.
constexpr int BLOCK_EF_STORE_AUX = 0;  // cache policy of the new residual's stores (0 plain, 2 non-temporal; A/B in
                                       // DESIGN.md §19)
template <bool HASBASE>
DEV void ef_unit_load(const Params& P, const UnitDev& U, float4 (&v)[UNIT_IT]) {
  static_assert(UNIT_IT % EF_ROWS == 0, "accumulate batch geometry");
  typedef unsigned int u4v __attribute__((ext_vector_type(4)));
  const uint32_t lane = lane_id();
  const float* xin = P.inptr != nullptr ? P.inptr[U.seg] + U.start : P.in + U.off;
  const __amdgpu_buffer_rsrc_t rx = unit_rsrc(xin, U.len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(HASBASE ? P.base + U.off : xin, U.len);
  const __amdgpu_buffer_rsrc_t rr = unit_rsrc(P.out + U.off, U.len);
#pragma unroll
  for (uint32_t i0 = 0; i0 < UNIT_IT; i0 += EF_ROWS) {
    u4v x[EF_ROWS], b[EF_ROWS], r[EF_ROWS];
#pragma unroll
    for (uint32_t it = 0; it < EF_ROWS; ++it) {
      const int boff = (int)(((i0 + it) * 64 + lane) * 16);
      x[it] = __builtin_amdgcn_raw_buffer_load_b128(rx, boff, 0, DENSE_Q_AUX);
      if (HASBASE) b[it] = __builtin_amdgcn_raw_buffer_load_b128(rb, boff, 0, DENSE_Q_AUX);
      r[it] = __builtin_amdgcn_raw_buffer_load_b128(rr, boff, 0, 0);
    }
#pragma unroll
    for (uint32_t it = 0; it < EF_ROWS; ++it) {
      float4 d = make_float4(__uint_as_float(x[it].x), __uint_as_float(x[it].y), __uint_as_float(x[it].z),
                             __uint_as_float(x[it].w));
      if (HASBASE)
        d = make_float4(d.x - __uint_as_float(b[it].x), d.y - __uint_as_float(b[it].y), d.z - __uint_as_float(b[it].z),
                        d.w - __uint_as_float(b[it].w));
      v[i0 + it] = make_float4(d.x + __uint_as_float(r[it].x), d.y + __uint_as_float(r[it].y),
                               d.z + __uint_as_float(r[it].z), d.w + __uint_as_float(r[it].w));
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Rotated block-wise quantisation: a full unit (len == UNIT) is multiplied by a pseudo-random sign
// diagonal and by the orthonormal Walsh-Hadamard matrix of order 4096 before it is quantised, and by both again, in the
// other order, after it is dequantised (the matrix is its own inverse). A unit shorter than UNIT is not rotated.
//   signs      element e of the unit at flat position c0 has its sign bit inverted where bit 23 of sr_u24(rot_seed,
//              c0 + e) is set: §18's hash under a seed of its own, an XOR on the bit pattern whatever the value is
//   transform  for h = 1, 2, 4, ..., 2048 in this order, every pair (i, i + h) with i & h == 0 becomes (t[i] + t[i+h],
//              t[i] - t[i+h]), fp32 adds and subtracts only; then every value * 2^-6
// Element e = (it * 64 + lane) * 4 + j lies in register r = 4 it + j of its lane: h = 1, 2 pair registers (j), h = 4 ..
// 128 pair lanes l and l ^ (h / 4), h = 256 .. 2048 pair registers again (it). A lane pair inside a row of 16 moves by
// DPP: the upper lane's value is p - t, computed as p + (-t), the same IEEE operation. Lanes 16 and 32 apart move by
// gfx950's half-exchange swaps, two registers a, b at a time: after swap(a, b) the lower lanes of a pair hold both
// halves of a's pair and the upper lanes both of b's, so one add and one subtract are the butterflies of both
// registers, and a second swap of (sum, difference) puts every result back in its lane. No select, no LDS.
// ------------------------------------------------------------------------------------------------
constexpr float ROT_NORM = 0.015625f;  // 1 / sqrt(4096)

template <uint32_t K>
DEV float rot_lane_xor(float x) {  // lane l reads lane l ^ K, K < 16: inside a DPP row
  static_assert(K == 1 || K == 2 || K == 4 || K == 8, "a lane pair inside a row of 16");
  const uint32_t v = __float_as_uint(x);
  if constexpr (K == 1) return __uint_as_float(dpp<0xB1>(v));  // quad_perm [1, 0, 3, 2]
  if constexpr (K == 2) return __uint_as_float(dpp<0x4E>(v));  // quad_perm [2, 3, 0, 1]
  if constexpr (K == 4) return __uint_as_float(dpp<0x1B>(dpp<0x141>(v)));  // l ^ 7 (row_half_mirror), then l ^ 3
  return __uint_as_float(dpp<0x128>(v));                       // row_ror:8
}

template <uint32_t K>
DEV void rot_stage_dpp(float (&t)[UNIT_IT * 4], uint32_t lane) {
  const uint32_t neg = (lane & K) ? 0x80000000u : 0u;
#pragma unroll
  for (uint32_t r = 0; r < UNIT_IT * 4; ++r)
    t[r] = rot_lane_xor<K>(t[r]) + __uint_as_float(__float_as_uint(t[r]) ^ neg);
}

template <bool HALF>  // lanes 32 apart (HALF), else 16 apart
DEV void rot_swap(float& a, float& b) {
  const uint32_t x = __float_as_uint(a), y = __float_as_uint(b);
  if constexpr (HALF) {
    const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
    a = __uint_as_float(r[0]), b = __uint_as_float(r[1]);
  } else {
    const auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
    a = __uint_as_float(r[0]), b = __uint_as_float(r[1]);
  }
}

template <bool HALF>
DEV void rot_stage_swap(float (&t)[UNIT_IT * 4]) {
#pragma unroll
  for (uint32_t r = 0; r < UNIT_IT * 4; r += 2) {
    float a = t[r], b = t[r + 1];
    rot_swap<HALF>(a, b);
    float s = a + b, d = a - b;
    rot_swap<HALF>(s, d);
    t[r] = s, t[r + 1] = d;
  }
}

template <uint32_t S>  // registers S apart
DEV void rot_stage_reg(float (&t)[UNIT_IT * 4]) {
#pragma unroll
  for (uint32_t r = 0; r < UNIT_IT * 4; ++r)
    if ((r & S) == 0) {
      const float s = t[r] + t[r + S], d = t[r] - t[r + S];
      t[r] = s, t[r + S] = d;
    }
}

// the transform of a full unit in its lanes' registers (encode and decode: the one copy)
DEV void rot_hadamard(float4 (&v)[UNIT_IT], uint32_t lane) {
  float t[UNIT_IT * 4];
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it)
    t[4 * it] = v[it].x, t[4 * it + 1] = v[it].y, t[4 * it + 2] = v[it].z, t[4 * it + 3] = v[it].w;
  rot_stage_reg<1>(t);
  rot_stage_reg<2>(t);
  rot_stage_dpp<1>(t, lane);
  rot_stage_dpp<2>(t, lane);
  rot_stage_dpp<4>(t, lane);
  rot_stage_dpp<8>(t, lane);
  rot_stage_swap<false>(t);
  rot_stage_swap<true>(t);
  rot_stage_reg<4>(t);
  rot_stage_reg<8>(t);
  rot_stage_reg<16>(t);
  rot_stage_reg<32>(t);
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it)
    v[it] = make_float4(t[4 * it] * ROT_NORM, t[4 * it + 1] * ROT_NORM, t[4 * it + 2] * ROT_NORM, t[4 * it + 3] * ROT_NORM);
}

// the sign diagonal of a full unit whose first element is at flat position c0
DEV void rot_signs(float4 (&v)[UNIT_IT], uint64_t rot_seed, uint64_t c0, uint32_t lane) {
  const SrUnit sr = sr_unit(rot_seed, c0, UNIT);
  auto flip = [&](float x, uint32_t e) { return __uint_as_float(__float_as_uint(x) ^ ((sr_draw(sr, e) & 0x800000u) << 8)); };
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    const uint32_t e0 = (it * 64 + lane) * 4;
    v[it] = make_float4(flip(v[it].x, e0), flip(v[it].y, e0 + 1), flip(v[it].z, e0 + 2), flip(v[it].w, e0 + 3));
  }
}

// SR: stochastic rounding, as dense_quant_unit's. EF: error feedback in the same pass:
// the unit quantised is a = (x - base) + r, and r (P.out, laid out like the input) leaves as ef_residual(a, xhat).
// G: the block size: 4096, the unit itself, or 256 / 1024 — a block is then G / 256 of the unit's rows,
// its range one wave reduction pair, written at dense_block_index (gb: the plan's block table for G).
// ROT: a full unit is rotated between the load and the min / max (rot_signs under rot_seed, then
// rot_hadamard), behind a wave-uniform len == UNIT; everything from the min / max on sees the coefficients.
template <bool DELTA, uint32_t B, bool XCD, bool SR, bool EF = false, uint32_t G = UNIT, bool ROT = false>
DEV void dense_block_quant_unit(const Params& P, const uint64_t* __restrict__ pw, float* __restrict__ bmn,
                                float* __restrict__ bscale, uint32_t* __restrict__ packed, uint64_t seed,
                                const uint64_t* __restrict__ gb = nullptr, uint64_t rot_seed = 0) {
  static_assert(!(SR && EF), "stochastic rounding and error feedback are not combined (DESIGN.md §18)");
  static_assert(!ROT || (!EF && G == UNIT), "the rotation: 4096-element blocks, no error feedback (DESIGN.md §22)");
  static_assert(G == UNIT || (!SR && !EF && (G == 256u || G == 1024u)),
                "blocks below the unit: 256 or 1024 elements, deterministic only (DESIGN.md §20)");
  constexpr uint32_t FB = 4u * B;                    // bits per field
  constexpr uint32_t NFIELD = UNIT / 4u;             // fields per unit (1024)
  constexpr bool ALIGNED = (32u % FB) == 0u;         // every word starts on a field (B = 1, 2, 4, 8)
  constexpr uint32_t NF = ALIGNED ? 32u / FB : 1u + (31u + FB - 1u) / FB;  // fields that can overlap one word
  __shared__ uint32_t sfld[WAVES][NFIELD];
  const uint32_t u = (XCD ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6);
  if (u >= P.n_units) return;  // (no block-wide barrier below: a wave owns its row of sfld)
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id(), len = U.len;
  uint32_t* fld = sfld[threadIdx.x >> 6];
  float4 v[UNIT_IT];
  if constexpr (EF)
    ef_unit_load<DELTA>(P, U, v);
  else
    dense_unit_load<DELTA, DENSE_Q_AUX>(P, U, v);
  if constexpr (ROT) {
    if (__builtin_amdgcn_readfirstlane(len) == UNIT) {
      rot_signs(v, rot_seed, U.off, lane);
      rot_hadamard(v, lane);
    }
  }
  float a, b, mn, scale;
  if constexpr (G == UNIT) {
    dense_unit_minmax(v, len, lane, a, b);
    codec_range(a, b, P.levels, mn, scale);
    if (lane == 0) {
      bmn[u] = mn;
      bscale[u] = scale;
    }
  }
  if constexpr (G != UNIT) {
    constexpr uint32_t RB = G / 256u;  // rows per block
    const uint64_t g0 = dense_block_index<G>(gb, U);
#pragma unroll
    for (uint32_t j = 0; j < UNIT / G; ++j) {
      dense_rows_minmax<RB>(v, j * RB, len, lane, a, b);
      codec_range(a, b, P.levels, mn, scale);
      if (lane == 0 && j * G < len) {  // (a block past the segment's end does not exist: no range is written)
        bmn[g0 + j] = mn;
        bscale[g0 + j] = scale;
      }
      with_rcp(mn, scale, P.levels, [&](auto qz) {
#pragma unroll
        for (uint32_t it = j * RB; it < (j + 1) * RB; ++it) {
          const uint32_t e0 = (it * 64 + lane) * 4;
          const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
          uint32_t f = 0;
#pragma unroll
          for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t q = qz(xs[i]);
            f |= ((len == UNIT || e0 + i < len) ? q : 0u) << (i * B);  // (a code past len is 0: the padding)
          }
          fld[it * 64 + lane] = f;
        }
      });
    }
  } else if constexpr (EF) {
    // (every load of r has returned: the range above is a reduction over all of v, so no store below can pass one)
    const __amdgpu_buffer_rsrc_t rr = unit_rsrc(P.out + U.off, len);
    with_rcp(mn, scale, P.levels, [&](auto qz) {
#pragma unroll
      for (uint32_t it = 0; it < UNIT_IT; ++it) {
        const uint32_t e0 = (it * 64 + lane) * 4;
        const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
        float rs[4];
        uint32_t f = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t q = qz(xs[j]);
          rs[j] = ef_residual(xs[j], dequantize((uint8_t)q, mn, scale));
          f |= ((len == UNIT || e0 + j < len) ? q : 0u) << (j * B);  // (a code past len is 0: the padding)
        }
        fld[it * 64 + lane] = f;
        // (a store past len is dropped: the padding between segments keeps what it held)
        dense_store_row<BLOCK_EF_STORE_AUX>(rr, len, it, lane, make_float4(rs[0], rs[1], rs[2], rs[3]));
      }
    });
  } else if constexpr (SR) {
    const SrUnit sr = sr_unit(seed, U.off, len);
    with_rcp_quotient(mn, scale, dense_rcp_scale(scale) && dense_unit_proven(v, mn), [&](auto tq) {
#pragma unroll
      for (uint32_t it = 0; it < UNIT_IT; ++it) {
        const uint32_t e0 = (it * 64 + lane) * 4;
        const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
        uint32_t f = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t q = sr_code(tq(xs[j]), sr_draw(sr, e0 + j), P.levels);
          f |= ((len == UNIT || e0 + j < len) ? q : 0u) << (j * B);  // (a code past len is 0: the padding)
        }
        fld[it * 64 + lane] = f;
      }
    });
  } else {
    with_rcp(mn, scale, P.levels, [&](auto qz) {
#pragma unroll
      for (uint32_t it = 0; it < UNIT_IT; ++it) {
        const uint32_t e0 = (it * 64 + lane) * 4;
        const float xs[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
        uint32_t f = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t q = qz(xs[j]);
          f |= ((len == UNIT || e0 + j < len) ? q : 0u) << (j * B);  // (a code past len is 0: the padding)
        }
        fld[it * 64 + lane] = f;
      }
    });
  }
  lds_order();
  // (the offset and the resource apart, as k_aggregate_dense: through dense_unit_words_rsrc this kernel compiles to
  // another register allocation, which measured 2-3 % slower at B = 4)
  uint32_t nwords;
  const uint64_t woff = dense_unit_word_off<B>(pw, U, nwords);
  const __amdgpu_buffer_rsrc_t rout = bytes_rsrc(packed + woff, nwords * 4u);
#pragma unroll
  for (uint32_t i = 0; i < UNIT / 32u * B / 64u; ++i) {
    const uint32_t w = i * 64 + lane, bit = w * 32u;
    const uint32_t f0 = bit / FB, s = ALIGNED ? 0u : bit - f0 * FB;  // the word's first field, and its bits below the word
    uint64_t acc = fld[f0] >> s;
    uint32_t nb = FB - s;
#pragma unroll
    for (uint32_t j = 1; j < NF; ++j) {
      const uint32_t x = f0 + j < NFIELD ? fld[f0 + j] : 0u;
      if (nb < 32u) acc |= (uint64_t)x << nb;
      nb += FB;
    }
    __builtin_amdgcn_raw_buffer_store_b32((uint32_t)acc, rout, (int)(w * 4u), 0, 0);  // (past the unit's words: dropped)
  }
}

template <bool DELTA, uint32_t B, bool XCD>
__global__ __launch_bounds__(BLOCK) void k_dense_block_quant(Params P, const uint64_t* __restrict__ pw,
                                                             float* __restrict__ bmn, float* __restrict__ bscale,
                                                             uint32_t* __restrict__ packed) {
  dense_block_quant_unit<DELTA, B, XCD, false>(P, pw, bmn, bscale, packed, 0);
}

template <bool DELTA, uint32_t B, bool XCD>
__global__ __launch_bounds__(BLOCK) void k_dense_block_quant_sr(Params P, const uint64_t* __restrict__ pw,
                                                                float* __restrict__ bmn, float* __restrict__ bscale,
                                                                uint32_t* __restrict__ packed, uint64_t seed) {
  dense_block_quant_unit<DELTA, B, XCD, true>(P, pw, bmn, bscale, packed, seed);
}

// ... with the rotation of full units, rounding to nearest or (SR) stochastically under `seed`
template <bool DELTA, uint32_t B, bool XCD, bool SR>
__global__ __launch_bounds__(BLOCK) void k_dense_block_quant_rot(Params P, const uint64_t* __restrict__ pw,
                                                                 float* __restrict__ bmn, float* __restrict__ bscale,
                                                                 uint32_t* __restrict__ packed, uint64_t rot_seed,
                                                                 uint64_t seed) {
  dense_block_quant_unit<DELTA, B, XCD, SR, false, UNIT, true>(P, pw, bmn, bscale, packed, seed, nullptr, rot_seed);
}

// The decode of a rotated stream: one wave per unit with the unit's 64 values per lane resident —
// dequantise, the inverse rotation of a full unit (rot_hadamard, then rot_signs: each its own inverse), base + x, the
// stores range-checked to the unit. A unit shorter than UNIT is k_dense_deq_stream<PERUNIT>'s, value for value. The unit
// as a scalar, as k_dense_deq_stream_g: its record and its range are scalar loads.
template <uint32_t B, bool HASBASE, bool XCD>
__global__ __launch_bounds__(BLOCK) void k_dense_deq_stream_rot(Params P, const uint64_t* __restrict__ pw,
                                                                const uint32_t* __restrict__ packed,
                                                                const float* __restrict__ rmn,
                                                                const float* __restrict__ rscale, uint64_t rot_seed) {
  const uint32_t u =
      __builtin_amdgcn_readfirstlane((XCD ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6));
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  const uint32_t lane = lane_id();
  const float mn = rmn[u], scale = rscale[u];
  const __amdgpu_buffer_rsrc_t rin = dense_unit_words_rsrc<B>(packed, pw, U);
  uint32_t lo[UNIT_IT], hi[UNIT_IT];
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) dense_row_words<B>(rin, it, lane, lo[it], hi[it]);
  const __amdgpu_buffer_rsrc_t rout = unit_rsrc(P.out + U.off, U.len);
  const __amdgpu_buffer_rsrc_t rb = unit_rsrc(HASBASE ? P.base + U.off : P.out + U.off, U.len);
  float4 v[UNIT_IT];
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) v[it] = dense_row_values<B>(lo[it], hi[it], it, lane, mn, scale);
  if (U.len == UNIT) {  // (wave-uniform: U is scalar)
    rot_hadamard(v, lane);
    rot_signs(v, rot_seed, U.off, lane);
  }
#pragma unroll
  for (uint32_t it = 0; it < UNIT_IT; ++it) {
    float4 x = v[it];
    if (HASBASE) x = dense_add_base(unit_load_x4<false>(rb, rb, (it * 64 + lane) * 16), x);
    dense_store_row(rout, U.len, it, lane, x);
  }
}

// ... with G-element blocks below the unit: gb is the plan's block table for G
template <bool DELTA, uint32_t B, bool XCD, uint32_t G>
__global__ __launch_bounds__(BLOCK) void k_dense_block_quant_g(Params P, const uint64_t* __restrict__ pw,
                                                               const uint64_t* __restrict__ gb, float* __restrict__ bmn,
                                                               float* __restrict__ bscale, uint32_t* __restrict__ packed) {
  dense_block_quant_unit<DELTA, B, XCD, false, false, G>(P, pw, bmn, bscale, packed, 0, gb);
}

// ... with error feedback in the same pass: r is read and rewritten in place, nothing else aliases it
template <bool HASBASE, uint32_t B, bool XCD>
__global__ __launch_bounds__(BLOCK) void k_dense_block_quant_ef(Params P, const uint64_t* __restrict__ pw,
                                                                float* __restrict__ bmn, float* __restrict__ bscale,
                                                                uint32_t* __restrict__ packed, float* r) {
  P.out = r;
  dense_block_quant_unit<HASBASE, B, XCD, false, true>(P, pw, bmn, bscale, packed, 0);
}

// ------------------------------------------------------------------------------------------------
// dense aggregate: fused decode + FedAvg of C ratio-1 uploads of the plan's own layout, each read where
// it lies — its uint8 codes (CODES), its wire v4 stream with one range per segment (PACKED) or per 4096-element unit
// (BLOCK). k_aggregate's contract, element by element in client order:
//   x_i = base + (mn_i + float(q_i) * scale_i);  acc = x_0 * w_0, acc = acc + (x_i * w_i);  out = agg_final(acc)
// (a segment the avg mask leaves out: out = x_0). Nothing is sparse here, so there is no tile, no index, no search: the
// accumulator and the base stay in registers, every client adds one code word (two at the straddling widths) per row
// and lane, and the result is stored once. AGD_SPLIT waves share a unit (each owns UNIT_IT / AGD_SPLIT of its rows);
// the code words of AGD_DEPTH clients are in flight per wave, behind one round of wave-uniform loads of those clients'
// pointers, ranges and weights. The loaders are the decoders' own (dense_codes_row / dense_row_words), the arithmetic
// is dequantize, the end is agg_final, the stores are k_dense_deq's.
// ------------------------------------------------------------------------------------------------
#ifndef AGD_SPLIT
#define AGD_SPLIT 4
#endif
#ifndef AGD_DEPTH
#define AGD_DEPTH 4
#endif
static_assert(AGD_SPLIT >= 1 && UNIT_IT % AGD_SPLIT == 0 && AGD_DEPTH >= 1, "dense aggregate geometry");

struct AggDenseArgs {
  const void* const* codes;   // [clients] each client's codes (uint8) or stream (uint32 words)
  const float* const* mn;     // [clients] each client's mn / scale: one per segment, or (BLOCK) one per unit
  const float* const* scale;
  const float* weights;       // [clients]
  const uint8_t* avg_mask;    // [nseg] or null, as k_aggregate's
  uint32_t clients;
  int mode;                   // COALAC_AGG_*: a wave-uniform branch at the end
  uint32_t xcd;               // the XCD-aware block order (batch-sized plans, as the dense decoders')
  float total, inv_total;
};

template <uint32_t B, int KIND, bool HASBASE>
__global__ __launch_bounds__(BLOCK) void k_aggregate_dense(Params P, const uint64_t* __restrict__ pw, AggDenseArgs A) {
  constexpr uint32_t RI = UNIT_IT / AGD_SPLIT, HE = UNIT / AGD_SPLIT, D = AGD_DEPTH;
  const uint32_t lane = lane_id();
  const uint32_t wid = __builtin_amdgcn_readfirstlane((A.xcd ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6));
  const uint32_t u = wid / AGD_SPLIT, r0 = (wid % AGD_SPLIT) * RI;  // the unit, and the first of this wave's rows
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  if (r0 * 256u >= U.len) return;
  static_assert(HE == RI * 256u, "rows per wave");
  const uint32_t ri = dense_range_index<KIND == COALAC_AGGD_BLOCK>(u, U);
  const bool avg = A.avg_mask == nullptr || A.avg_mask[U.seg] != 0;
  const uint32_t ncl = avg ? A.clients : 1u;
  const uint64_t o = dense_unit_entry(U);  // (CODES)
  const bool vec = dense_unit_vec(U);
  uint32_t nwords = 0;
  const uint64_t woff = KIND == COALAC_AGGD_CODES ? 0 : dense_unit_word_off<B>(pw, U, nwords);
  const __amdgpu_buffer_rsrc_t rout = unit_rsrc(P.out + U.off, U.len);
  float4 bv[RI], acc[RI];
  if (HASBASE) {
    const __amdgpu_buffer_rsrc_t rb = unit_rsrc(P.base + U.off, U.len);
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) bv[it] = unit_load_x4<false>(rb, rb, ((r0 + it) * 64 + lane) * 16);
  }
  // acc starts at -0.0f, the exact additive identity, so no client is special (as k_aggregate)
#pragma unroll
  for (uint32_t it = 0; it < RI; ++it) acc[it] = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
  for (uint32_t c0 = 0; c0 < ncl; c0 += D) {
    // round 1, wave-uniform: the clients' pointers, ranges and weights (a chunk's tail repeats the last client: every
    // load stays inside some client's buffers, and the repeats are not accumulated)
    const void* cp[D];
    float mn[D], sc[D], w[D];
#pragma unroll
    for (uint32_t t = 0; t < D; ++t) {
      const uint32_t c = min(c0 + t, ncl - 1);
      cp[t] = A.codes[c];
      mn[t] = A.mn[c][ri];
      sc[t] = A.scale[c][ri];
      w[t] = avg ? A.weights[c] : 1.0f;  // (x_0 * 1.0f == x_0)
    }
    // round 2: every code word of the chunk
    uint32_t lo[D][RI], hi[D][RI];
#pragma unroll
    for (uint32_t t = 0; t < D; ++t) {
      if (KIND == COALAC_AGGD_CODES) {
        const __amdgpu_buffer_rsrc_t rin = bytes_rsrc(static_cast<const uint8_t*>(cp[t]) + o, U.len);
#pragma unroll
        for (uint32_t it = 0; it < RI; ++it) {
          lo[t][it] = dense_codes_row(rin, vec, ((r0 + it) * 64 + lane) * 4);
          hi[t][it] = 0u;
        }
      } else {  // (dense_unit_words_rsrc, the unit's offset shared by the clients' streams)
        const __amdgpu_buffer_rsrc_t rin = bytes_rsrc(static_cast<const uint32_t*>(cp[t]) + woff, nwords * 4u);
#pragma unroll
        for (uint32_t it = 0; it < RI; ++it) dense_row_words<B>(rin, r0 + it, lane, lo[t][it], hi[t][it]);
      }
    }
#pragma unroll
    for (uint32_t t = 0; t < D; ++t) {
      if (c0 + t >= ncl) break;
#pragma unroll
      for (uint32_t it = 0; it < RI; ++it) {
        float4 x = KIND == COALAC_AGGD_CODES ? dense_codes_values(lo[t][it], mn[t], sc[t])
                                             : dense_row_values<B>(lo[t][it], hi[t][it], r0 + it, lane, mn[t], sc[t]);
        if (HASBASE) x = dense_add_base(bv[it], x);
        const float4 p = make_float4(x.x * w[t], x.y * w[t], x.z * w[t], x.w * w[t]);
        acc[it] = make_float4(acc[it].x + p.x, acc[it].y + p.y, acc[it].z + p.z, acc[it].w + p.w);
      }
    }
  }
  auto store = [&](auto fin) {
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) dense_store_row(rout, U.len, r0 + it, lane, fin(acc[it]));
  };
  if (!avg || A.mode == COALAC_AGG_SUM)
    store([&](float4 a) { return a; });
  else if (A.mode == COALAC_AGG_DIV)
    store([&](float4 a) { return agg_final<COALAC_AGG_DIV>(a, A.total, A.inv_total); });
  else
    store([&](float4 a) { return agg_final<COALAC_AGG_RECIP>(a, A.total, A.inv_total); });
}

// k_aggregate_dense, kind BLOCK, for G-element blocks below the unit: per client, the ranges of the
// blocks this wave's rows lie in (NBW of them: one at G = 1024, four at G = 256), at dense_block_index (gb: the plan's
// block table for G). The client order, the arithmetic and the stores are k_aggregate_dense's, statement for statement;
// a kernel of its own, so that the 4096 kernel above keeps its registers.
template <uint32_t B, bool HASBASE, uint32_t G>
__global__ __launch_bounds__(BLOCK) void k_aggregate_dense_g(Params P, const uint64_t* __restrict__ pw,
                                                             const uint64_t* __restrict__ gb, AggDenseArgs A) {
  constexpr uint32_t RI = UNIT_IT / AGD_SPLIT, HE = UNIT / AGD_SPLIT, D = AGD_DEPTH;
  static_assert(G == 256u || G == 1024u, "blocks below the unit: 256 or 1024 elements");
  static_assert(G >= HE ? G % HE == 0 : HE % G == 0, "a wave's rows are whole blocks, or lie in one");
  constexpr uint32_t NBW = G >= HE ? 1u : HE / G, RB = G / 256u;  // blocks per wave, rows per block
  const uint32_t lane = lane_id();
  const uint32_t wid = __builtin_amdgcn_readfirstlane((A.xcd ? xcd_block(blockIdx.x) : blockIdx.x) * WAVES + (threadIdx.x >> 6));
  const uint32_t u = wid / AGD_SPLIT, r0 = (wid % AGD_SPLIT) * RI;  // the unit, and the first of this wave's rows
  if (u >= P.n_units) return;
  const UnitDev U = P.units[u];
  if (r0 * 256u >= U.len) return;
  static_assert(HE == RI * 256u, "rows per wave");
  const uint64_t ri = dense_block_index<G>(gb, U) + r0 / RB;  // the wave's first block
  const bool avg = A.avg_mask == nullptr || A.avg_mask[U.seg] != 0;
  const uint32_t ncl = avg ? A.clients : 1u;
  uint32_t nwords = 0;
  const uint64_t woff = dense_unit_word_off<B>(pw, U, nwords);
  const __amdgpu_buffer_rsrc_t rout = unit_rsrc(P.out + U.off, U.len);
  float4 bv[RI], acc[RI];
  if (HASBASE) {
    const __amdgpu_buffer_rsrc_t rb = unit_rsrc(P.base + U.off, U.len);
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) bv[it] = unit_load_x4<false>(rb, rb, ((r0 + it) * 64 + lane) * 16);
  }
  // acc starts at -0.0f, the exact additive identity, so no client is special (as k_aggregate)
#pragma unroll
  for (uint32_t it = 0; it < RI; ++it) acc[it] = make_float4(-0.0f, -0.0f, -0.0f, -0.0f);
  for (uint32_t c0 = 0; c0 < ncl; c0 += D) {
    // round 1, wave-uniform: the clients' pointers, ranges and weights (a chunk's tail repeats the last client: every
    // load stays inside some client's buffers, and the repeats are not accumulated)
    const void* cp[D];
    float mn[D][NBW], sc[D][NBW], w[D];
#pragma unroll
    for (uint32_t t = 0; t < D; ++t) {
      const uint32_t c = min(c0 + t, ncl - 1);
      cp[t] = A.codes[c];
#pragma unroll
      for (uint32_t j = 0; j < NBW; ++j) {
        // (the wave's first block exists: r0 * 256 < len above; a later one past the end is not read, its rows not stored)
        const bool there = j == 0 || (r0 + j * RB) * 256u < U.len;
        mn[t][j] = there ? A.mn[c][ri + j] : 0.0f;
        sc[t][j] = there ? A.scale[c][ri + j] : 0.0f;
      }
      w[t] = avg ? A.weights[c] : 1.0f;  // (x_0 * 1.0f == x_0)
    }
    // round 2: every code word of the chunk
    uint32_t lo[D][RI], hi[D][RI];
#pragma unroll
    for (uint32_t t = 0; t < D; ++t) {
      // (dense_unit_words_rsrc, the unit's offset shared by the clients' streams)
      const __amdgpu_buffer_rsrc_t rin = bytes_rsrc(static_cast<const uint32_t*>(cp[t]) + woff, nwords * 4u);
#pragma unroll
      for (uint32_t it = 0; it < RI; ++it) dense_row_words<B>(rin, r0 + it, lane, lo[t][it], hi[t][it]);
    }
#pragma unroll
    for (uint32_t t = 0; t < D; ++t) {
      if (c0 + t >= ncl) break;
#pragma unroll
      for (uint32_t it = 0; it < RI; ++it) {
        const uint32_t j = NBW == 1 ? 0u : it / RB;  // the row's block among the wave's
        float4 x = dense_row_values<B>(lo[t][it], hi[t][it], r0 + it, lane, mn[t][j], sc[t][j]);
        if (HASBASE) x = dense_add_base(bv[it], x);
        const float4 p = make_float4(x.x * w[t], x.y * w[t], x.z * w[t], x.w * w[t]);
        acc[it] = make_float4(acc[it].x + p.x, acc[it].y + p.y, acc[it].z + p.z, acc[it].w + p.w);
      }
    }
  }
  auto store = [&](auto fin) {
#pragma unroll
    for (uint32_t it = 0; it < RI; ++it) dense_store_row(rout, U.len, r0 + it, lane, fin(acc[it]));
  };
  if (!avg || A.mode == COALAC_AGG_SUM)
    store([&](float4 a) { return a; });
  else if (A.mode == COALAC_AGG_DIV)
    store([&](float4 a) { return agg_final<COALAC_AGG_DIV>(a, A.total, A.inv_total); });
  else
    store([&](float4 a) { return agg_final<COALAC_AGG_RECIP>(a, A.total, A.inv_total); });
}

// k_gather: n scalars of `bytes` each, from their own storage (one device pointer each), into one contiguous
// buffer — an update's passthrough entries (BatchNorm's int64 num_batches_tracked, one per layer) snapshotted
// in one launch instead of a stack of tensor copies
__global__ __launch_bounds__(BLOCK) void k_gather(const void* const* src, uint32_t n, uint32_t bytes, void* dst) {
  const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const void* s = src[i];
  uint8_t* d = static_cast<uint8_t*>(dst) + (uint64_t)i * bytes;
  if (bytes == 8)
    *reinterpret_cast<uint64_t*>(d) = *static_cast<const uint64_t*>(s);
  else if (bytes == 4)
    *reinterpret_cast<uint32_t*>(d) = *static_cast<const uint32_t*>(s);
  else if (bytes == 2)
    *reinterpret_cast<uint16_t*>(d) = *static_cast<const uint16_t*>(s);
  else
    *d = *static_cast<const uint8_t*>(s);
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_CHECK(expr)                                                                             \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return fail(COALAC_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
constexpr uint32_t ceil_div(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// Hands out typed, 256-byte-aligned sub-ranges of one allocation, in call order. With a null base it only measures
// (every pointer comes out null, `off` ends at the bytes needed), so one walk over a buffer's arrays gives both its
// size at plan creation and its pointers at a call.
struct Carver {
  uint8_t* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = align_up(off + sizeof(T) * count, 256);
    return p;
  }
};

// The encode workspace, listed once: sets P's workspace pointers inside `ws` (null: measures only) from the counts
// already in P, and returns the bytes the plan needs. A kernel that gets a new array gets it here, and nowhere else.
size_t carve_workspace(Params& P, bool dense, void* ws) {
  Carver c{static_cast<uint8_t*>(ws)};
  const size_t S = P.nseg, LU = P.n_lunits, NG = P.n_groups, NL = P.n_large, CC = P.ccap;
  if (dense) {  // a dense plan's encode workspace: the per-unit min / max only
    P.umm = c.take<float>(2 * (size_t)P.n_units);
    return std::max<size_t>(c.off, 256);
  }
  P.status = c.take<uint32_t>(S);
  P.tstar = c.take<uint32_t>(S);
  P.rtie = c.take<uint32_t>(S);
  P.tlo = c.take<uint32_t>(LU);
  P.thi = c.take<uint32_t>(LU);
  P.cntA = c.take<uint32_t>(LU);
  P.cntC = c.take<uint32_t>(LU);
  P.cntZ = c.take<uint32_t>(LU);
  P.tsgn = c.take<uint32_t>(LU);
  P.gtC = c.take<uint32_t>(LU);
  P.eqC = c.take<uint32_t>(LU);
  P.eqpre = c.take<uint32_t>(LU);
  P.outoff = c.take<uint32_t>(LU);
  P.uemit = c.take<uint4>(LU);
  P.cval = c.take<uint32_t>(CC * LU);
  P.cpos = c.take<uint16_t>(CC * LU);
  P.stamps = c.take<uint64_t>(NSTAMP * std::max<size_t>(S, 1));  // (a call without COALAC_FLAG_STAMPS nulls it)
  P.ghist = c.take<uint32_t>(HB2 * NG);
  P.gcnt = c.take<uint32_t>(NG);
  P.glist = c.take<uint2>(GCAP * NG);
  P.gmm = c.take<float>(2 * NG);
  P.sstate = c.take<uint4>(NL);
  P.shhi = c.take<uint32_t>(NL);
  return std::max<size_t>(c.off, 256);
}

// The plan's metadata tables on the host, and — listed once, in blob order — the Params pointer each becomes in the
// plan's one device allocation. host null: returns the blob's size; else packs the vectors into `host` (a staging
// buffer of that size, copied to `dev` by the caller) and points P's members into `dev`.
struct PlanTables {
  std::vector<SegDev> segs, lsegs, ssegs;
  std::vector<UnitDev> units, lunits;
  std::vector<uint32_t> small_list, large_list;
  std::vector<uint4> groups, gseg;
};

size_t place_tables(const PlanTables& T, Params& P, uint8_t* host, const uint8_t* dev) {
  Carver c{host};
  auto put = [&](auto*& dst, const auto& v) {
    using E = typename std::decay_t<decltype(v)>::value_type;
    static_assert(std::is_same<decltype(dst), const E*&>::value, "table and pointer types differ");
    E* h = c.take<E>(v.size());
    if (!host) return;
    if (!v.empty()) memcpy(h, v.data(), sizeof(E) * v.size());
    dst = reinterpret_cast<const E*>(dev + (reinterpret_cast<uint8_t*>(h) - host));
  };
  put(P.segs, T.segs);
  put(P.units, T.units);
  put(P.lunits, T.lunits);
  put(P.small_list, T.small_list);
  put(P.large_list, T.large_list);
  put(P.lsegs, T.lsegs);
  put(P.ssegs, T.ssegs);
  put(P.groups, T.groups);
  put(P.gseg, T.gseg);
  return c.off + 256;  // (the blob ends in a 256-byte pad)
}

// Runtime flags -> template arguments, the one way: with_flags(f, a, b, ...) calls the generic lambda f with one
// std::bool_constant per flag, so f's body names a kernel specialisation as k<a.value, b.value>. Every combination of
// the flags passed is instantiated — a launch site passes only the flags whose every combination exists.
template <typename F>
auto with_flags(F&& f) {
  return f();
}
template <typename F, typename... Rest>
auto with_flags(F&& f, bool flag, Rest... rest) {
  if (flag) return with_flags([&](auto... t) { return f(std::true_type{}, t...); }, rest...);
  return with_flags([&](auto... t) { return f(std::false_type{}, t...); }, rest...);
}
// ... and the aggregate's mode, as a std::integral_constant<int, COALAC_AGG_*>
template <typename F>
auto with_agg_mode(int mode, F&& f) {
  if (mode == COALAC_AGG_RECIP) return f(std::integral_constant<int, COALAC_AGG_RECIP>{});
  if (mode == COALAC_AGG_SUM) return f(std::integral_constant<int, COALAC_AGG_SUM>{});
  return f(std::integral_constant<int, COALAC_AGG_DIV>{});
}

// Small segments go beside the large ones' pipeline on a side stream once the batch is big enough for
// the fork / join (~10-20 us) to pay off (>= 16384 large units, ~3 ResNet-50 updates).
constexpr uint32_t FORK_MIN_LUNITS = 16384;

// the block sizes below the unit, in the order of coalac_plan's n_blocks / dense_gb
constexpr uint32_t SUB_BLOCKS[2] = {256u, 1024u};

}  // namespace

struct coalac_plan {
  int device = -1;
  int bits = 8;
  bool dense = false;        // every segment keeps all its elements: the dense codec (indices implied)
  bool dense_empty = false;  // a dense plan with a 0-element segment (keeps the separate k_dense_seg)
  // Launch choices, decided once at plan creation. Two unit counts are in play: the encode kernels run over the large
  // units only (a small segment is encoded whole by one block, off the streaming kernels' grid), the decode, dense and
  // error-feedback kernels over all units — so "latency-bound" (<= LATENCY_PLAN_UNITS) is one predicate per count.
  bool encode_latency = false;  // n_lunits: the sparse encode's kernel variants
  bool decode_latency = false;  // n_units: the decode's and the dense codec's (and the default small-segment limit)
  bool high_ratio = false;      // the largest k / n of the large segments > HIGH_RATIO: more record rows per round in
                                // k_ghist / k_gwin / k_emit, and 8 entry chunks in registers in k_decode_lds
  bool small_1k = false;        // small segments hold <= SMALL_MAX_LATENCY elements: k_scan's 16 KB small arena
  bool fork_sized = false;      // small segments beside >= FORK_MIN_LUNITS large units: the encode forks them to a
                                // side stream unless the call says COALAC_FLAG_NO_FORK
  uint64_t span = 0, total_k = 0, ws_bytes = 0;
  // dense plans: the bit-packed code stream (wire v4) — its length in words at the plan's code width, and each segment
  // row's word offset in it (a device array inside meta)
  uint64_t dense_words = 0;
  const uint64_t* dense_pw = nullptr;
  // ... and its blocks below the unit, for G = 256 [0] and G = 1024 [1]: the block count NB = sum of
  // ceil(n_s / G), and each segment row's first block gb_s (a device array inside meta, behind dense_pw)
  uint64_t n_blocks[2] = {0, 0};
  const uint64_t* dense_gb[2] = {nullptr, nullptr};
  Params proto{};  // what every call's Params starts as: the metadata pointers (into meta), counts, levels and ccap
  void* meta = nullptr;
  std::vector<SegDev> hsegs;  // host copy (aggregate validates the client-copy structure)
  // encode fork/join: k_small runs on `side`, concurrently with k_sample / k_scan on the caller's stream
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  std::mutex mu;  // serialises the (asynchronous) enqueue sequences that use side / fork / join
};

namespace {

int check_device(coalac_plan_t plan) {
  int dev = -1;
  HIP_CHECK(hipGetDevice(&dev));
  if (dev != plan->device)
    return fail(COALAC_EDEVICE, "current device %d differs from the plan's device %d", dev, plan->device);
  return COALAC_OK;
}

// shared by the entry points: the OR of some addresses (for one alignment test), the decoders' payload operands,
// and the end of every launch sequence
uintptr_t addr_bits(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c);
}

void set_payload(Params& P, const int32_t* d_idx, const void* d_vals, const float* d_mn, const float* d_scale) {
  P.cidx = d_idx;
  P.cvals = d_vals;
  P.cmn = d_mn;
  P.cscale = d_scale;
}

int launched() {
  HIP_CHECK(hipGetLastError());
  return COALAC_OK;
}

// Timing events of the _ev variants: hipEventRecord(ev[i], stream) at boundary i of a call (NULL array or entries:
// nothing recorded). Encode: [0] before k_sample, [1] after it, [2] after k_scan, [3] after the select kernels,
// [4] after k_emit; decode and aggregate: [0] at the start, [1] before the decode kernel, [2] after it.
struct Marks {
  void* const* ev;
  int n;
  int at(int i, hipStream_t st) const {
    if (ev != nullptr && i < n && ev[i] != nullptr) HIP_CHECK(hipEventRecord(static_cast<hipEvent_t>(ev[i]), st));
    return COALAC_OK;
  }
};

#define MARK(i)                         \
  do {                                  \
    const int rc_ = marks.at((i), st);  \
    if (rc_) return rc_;                \
  } while (0)

// the dense encode: the min / max pass and the per-segment reduction between marks 0 and 1, the quantise stream
// between 1 and 2 (where k_scan sits in a sparse encode)
template <bool DELTA, bool RAW>
int launch_dense_encode(const Params& P, coalac_plan_t plan, hipStream_t st, const Marks& marks) {
  const dim3 g(ceil_div(P.n_units, WAVES));
  const bool xcd = !plan->decode_latency;
  MARK(0);
  if (!RAW)
    with_flags([&](auto x) { hipLaunchKernelGGL((k_dense_minmax<DELTA, x.value>), g, dim3(BLOCK), 0, st, P); }, xcd);
  // a segment without units: k_dense_seg writes every segment's mn / scale (else the quantise waves reduce their own)
  if (plan->dense_empty) hipLaunchKernelGGL((k_dense_seg<RAW>), dim3(P.nseg), dim3(BLOCK), 0, st, P);
  MARK(1);
  with_flags(
      [&](auto x, auto segred) {
        hipLaunchKernelGGL((k_dense_quant<DELTA, RAW, x.value, segred.value>), g, dim3(BLOCK), 0, st, P);
      },
      xcd, !plan->dense_empty);
  MARK(2);
  MARK(3);
  MARK(4);
  return COALAC_OK;
}

// the same sequence with the stochastic quantise stream (coalac_encode_sr: bits 1..8, no marks)
template <bool DELTA>
void launch_dense_encode_sr(const Params& P, coalac_plan_t plan, hipStream_t st, uint64_t seed) {
  const dim3 g(ceil_div(P.n_units, WAVES));
  const bool xcd = !plan->decode_latency;
  with_flags([&](auto x) { hipLaunchKernelGGL((k_dense_minmax<DELTA, x.value>), g, dim3(BLOCK), 0, st, P); }, xcd);
  if (plan->dense_empty) hipLaunchKernelGGL((k_dense_seg<false>), dim3(P.nseg), dim3(BLOCK), 0, st, P);
  with_flags(
      [&](auto x, auto segred) {
        hipLaunchKernelGGL((k_dense_quant_sr<DELTA, x.value, segred.value>), g, dim3(BLOCK), 0, st, P, seed);
      },
      xcd, !plan->dense_empty);
}

// The sparse encode. By plan class (the file header lists the kernels):
//   latency-bound (encode_latency):  k_sample -> k_scan with the small segments in its first blocks -> the select
//                                    chain and k_emit in their *_LAT geometries
//   batch:                           k_presel (samplers + small segments) -> k_scan over large units only -> ...
//   fork class (fork_sized, unless the call says COALAC_FLAG_NO_FORK): k_small on the plan's side stream beside
//                                    k_sample -> k_scan -> ..., joined after k_emit
// A plan without small segments runs k_sample alone; one without large segments only its small-segment kernel.
template <bool DELTA, bool RAW>
int launch_encode(const Params& P, coalac_plan_t plan, hipStream_t st, const Marks& marks) {
  const bool lat = plan->encode_latency;
  const bool fork = plan->fork_sized && !(P.flags & COALAC_FLAG_NO_FORK);
  const bool presel = !fork && P.n_small;
  const bool small_in_scan = presel && lat;
  Params Q = P;
  Q.scan_small = 0u;
  std::unique_lock<std::mutex> lk(plan->mu, std::defer_lock);
  if (fork) {
    lk.lock();
    if (plan->side == nullptr) {  // created on first use: pipelined plans never need it
      if (hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&plan->fork, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&plan->join, hipEventDisableTiming) != hipSuccess)
        return fail(COALAC_EHIP, "creating the plan's side stream / events failed: %s",
                    hipGetErrorString(hipGetLastError()));
    }
  }
  MARK(0);
  if (fork) {
    HIP_CHECK(hipEventRecord(plan->fork, st));
    HIP_CHECK(hipStreamWaitEvent(plan->side, plan->fork, 0));
    hipLaunchKernelGGL((k_small<DELTA, RAW>), dim3(P.n_small), dim3(BLOCK), 0, plan->side, P);
    HIP_CHECK(hipEventRecord(plan->join, plan->side));
  }
  if (presel && !small_in_scan)
    hipLaunchKernelGGL((k_presel<DELTA, RAW>), dim3(P.n_large + P.n_small), dim3(BLOCK), 0, st, P);
  else if (P.n_large && lat)
    hipLaunchKernelGGL((k_sample<DELTA, RAW, SAMPLE_NT_LAT>), dim3(P.n_large), dim3(SAMPLE_NT_LAT), 0, st, P);
  else if (P.n_large)
    hipLaunchKernelGGL((k_sample<DELTA, RAW, BLOCK>), dim3(P.n_large), dim3(BLOCK), 0, st, P);
  MARK(1);
  if (small_in_scan) {
    Q.scan_small = P.n_small;
    const dim3 gs(ceil_div(P.n_lunits, SCAN_NT_LAT / 64) + P.n_small);
    if (plan->small_1k)
      hipLaunchKernelGGL((k_scan<DELTA, RAW, true, SCAN_WPE_LAT_1K, SCAN_NB_LAT, SCAN_NT_LAT, SMALL_MAX_LATENCY>), gs,
                         dim3(SCAN_NT_LAT), 0, st, Q);
    else
      hipLaunchKernelGGL((k_scan<DELTA, RAW, true, SCAN_WPE_LAT, SCAN_NB_LAT, SCAN_NT_LAT>), gs, dim3(SCAN_NT_LAT), 0, st,
                         Q);
  } else if (P.n_lunits) {
    hipLaunchKernelGGL((k_scan<DELTA, RAW, false, SCAN_WPE, SCAN_NB, SCAN_NT>), dim3(ceil_div(P.n_lunits, SCAN_NT / 64)),
                       dim3(SCAN_NT), 0, st, Q);
  }
  MARK(2);
  if (P.n_large && lat) {  // the speculative sweeps (no high-ratio variant of them)
    hipLaunchKernelGGL((k_ghist<GHIST_NT_LAT, true>), dim3(P.n_groups), dim3(GHIST_NT_LAT), 0, st, P);
    hipLaunchKernelGGL((k_gwin<GWIN_NT_LAT, true>), dim3(P.n_groups), dim3(GWIN_NT_LAT), 0, st, P);
    hipLaunchKernelGGL((k_select<DELTA, RAW, SEL_NT_LAT>), dim3(P.n_large), dim3(SEL_NT_LAT), 0, st, P);
  } else if (P.n_large) {
    with_flags(
        [&](auto hr) {
          hipLaunchKernelGGL((k_ghist<BLOCK, false, hr.value>), dim3(P.n_groups), dim3(BLOCK), 0, st, P);
          hipLaunchKernelGGL((k_gwin<BLOCK, false, hr.value>), dim3(P.n_groups), dim3(BLOCK), 0, st, P);
        },
        plan->high_ratio);
    hipLaunchKernelGGL((k_select<DELTA, RAW>), dim3(P.n_large), dim3(SEL_NT), 0, st, P);
  }
  MARK(3);
  if (P.n_large)
    with_flags(
        [&](auto l, auto hr) {
          constexpr uint32_t UPW = l.value ? EMIT_UPW_LAT : EMIT_UPW, TR = hr.value ? 4u : 1u;
          hipLaunchKernelGGL((k_emit<DELTA, RAW, UPW, TR>), dim3(ceil_div(P.n_lunits, UPW * WAVES)), dim3(BLOCK), 0, st, P);
        },
        lat, plan->high_ratio);
  if (fork) HIP_CHECK(hipStreamWaitEvent(st, plan->join, 0));
  MARK(4);
  return COALAC_OK;
}

int encode_impl(coalac_plan_t plan, const float* d_in, const float* const* d_inptr, const float* d_base,
                int32_t* d_idx, void* d_vals, float* d_mn, float* d_scale, uint32_t* d_ustart, void* d_ws,
                uint64_t ws_bytes, unsigned flags, void* stream, const Marks& marks) {
  if (!plan) return fail(COALAC_EINVAL, "coalac_encode: plan is NULL");
  if (plan->proto.nseg == 0) return COALAC_OK;
  if (!d_mn || !d_scale) return fail(COALAC_EINVAL, "coalac_encode: mn/scale pointers are NULL");
  if (plan->span && !d_in && !d_inptr) return fail(COALAC_EINVAL, "coalac_encode: input pointer is NULL");
  if (plan->total_k && (!(d_idx || plan->dense) || !d_vals))
    return fail(COALAC_EINVAL, "coalac_encode: idx/vals pointers are NULL (idx may be NULL for a dense plan only)");
  if (addr_bits(d_in, d_base) & 15) return fail(COALAC_EINVAL, "coalac_encode: input/base must be 16-byte aligned");
  if (addr_bits(d_ustart) & 3) return fail(COALAC_EINVAL, "coalac_encode: ustart must be 4-byte aligned");
  if (!d_ws || ws_bytes < plan->ws_bytes)
    return fail(COALAC_EWORKSPACE, "coalac_encode: workspace %llu < required %llu", (unsigned long long)ws_bytes,
                (unsigned long long)plan->ws_bytes);
  int rc = check_device(plan);
  if (rc) return rc;
  Params P = plan->proto;
  P.in = d_in;
  P.inptr = d_inptr;
  P.base = d_base;
  P.idx = d_idx;
  P.vals = d_vals;
  P.mn = d_mn;
  P.scale = d_scale;
  P.ustart_out = d_ustart;
  P.flags = flags;
  carve_workspace(P, plan->dense, d_ws);
  if (!(flags & COALAC_FLAG_STAMPS)) P.stamps = nullptr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rc = with_flags(
      [&](auto delta, auto raw) {
        return plan->dense ? launch_dense_encode<delta.value, raw.value>(P, plan, st, marks)
                           : launch_encode<delta.value, raw.value>(P, plan, st, marks);
      },
      d_base != nullptr, plan->bits == 32);
  return rc ? rc : launched();
}

// The write-once decode (k_decode_lds) of a whole plan: batches one wave per unit in two 8-row passes (4-row in
// delta mode) with non-temporal stores and the XCD-aware order; latency-bound plans DECODE_WPU_LAT waves per unit
// (one pass each: twice the waves, each with half the work, for a launch of one update's ~6.5 k units).
// HR: plans whose segments keep more than ~1.5 % (more than 64 entries in a unit on average) hold 8 entry chunks in
// registers (from ratio 0.02, the plan's high_ratio: C3 at ratio 0.1, decode 0.63 -> 0.37 ms)
template <bool RAW, bool HB, bool HR>
void launch_decode_lds(const Params& P, coalac_plan_t plan, hipStream_t st) {
  constexpr uint32_t DW = DECODE_NT / 64, NCH = HR ? 8u : 1u;
  if (plan->decode_latency) {
    constexpr uint32_t W = DECODE_WPU_LAT, Q = HB ? DECODE_QROWS_BASE : UNIT_IT / DECODE_WPU_LAT;
    hipLaunchKernelGGL((k_decode_lds<RAW, HB, W, (Q < 8u ? Q : 8u), DECODE_SAUX_LAT, false, NCH>),
                       dim3(ceil_div(P.n_units * W, DW)), dim3(DECODE_NT), 0, st, P);
  } else {
    hipLaunchKernelGGL((k_decode_lds<RAW, HB, 1u, HB ? DECODE_QROWS_BASE : DECODE_QROWS, STORE_AUX, true, NCH>),
                       dim3(ceil_div(P.n_units, DW)), dim3(DECODE_NT), 0, st, P);
  }
}

// the compact payload's geometry: field width and stream length of a plan
uint32_t packed_field_bits(const coalac_plan* plan) { return 12u + (plan->bits == 32 ? 0u : (uint32_t)plan->bits); }
uint64_t packed_words(const coalac_plan* plan) { return (plan->total_k * packed_field_bits(plan) + 31u) / 32u; }

// the checks pack and unpack share; *done: nothing to launch (an empty plan)
int packed_args(coalac_plan_t plan, const char* who, bool null_arg, uint64_t packed_bytes, bool* done) {
  *done = false;
  if (!plan) return fail(COALAC_EINVAL, "%s: plan is NULL", who);
  if (null_arg) return fail(COALAC_EINVAL, "%s: a pointer is NULL", who);
  if (plan->dense)
    return fail(COALAC_EINVAL, "%s: a dense plan's indices are implied, there is nothing to pack (wire v2 carries it)", who);
  if (packed_bytes < 4 * packed_words(plan))
    return fail(COALAC_EINVAL, "%s: packed_bytes=%llu < the plan's %llu", who, (unsigned long long)packed_bytes,
                (unsigned long long)(4 * packed_words(plan)));
  *done = plan->total_k == 0 || plan->proto.n_units == 0;
  return *done ? COALAC_OK : check_device(plan);
}

// The dense stream's entry points (coalac_pack_dense, coalac_unpack_dense, coalac_decode_packed, coalac_encode_block*
// and coalac_decode_block*): one description of a call's arguments and one walk over it, every
// COALAC_EINVAL case ahead of the empty-plan return and of the first device call. A new entry point fills a DenseCall
// and passes its launch as a lambda.
constexpr const char* A_POINTER = "a pointer";
constexpr const char* PACK_HINT = "; a sparse plan's payload is coalac_pack's";
constexpr const char* SR_HINT = "; the sparse emit rounds to nearest";
constexpr const char* EF_HINT = "; a sparse plan's error feedback is coalac_ef_accumulate / coalac_ef_commit";

struct DenseCall {
  const char* who;
  const char* null_what;  // how the message names a required pointer that is NULL (nullptr: none is)
  uint64_t packed_bytes;
  uintptr_t a16;  // addr_bits of the pointers that must be 16-byte aligned, and what the message calls them
  const char* names16;
  uintptr_t a4;  // ... 4-byte aligned
  const char* names4;
  const char* hint = "";  // the end of "needs a dense plan": where the caller of a sparse plan should go
  int inputs = 1;         // encoders: how many of d_in and d_seg_in were given
};

int input_count(const void* d_in, const void* d_seg_in) { return (d_in != nullptr) + (d_seg_in != nullptr); }

int misaligned(const char* who, uintptr_t addrs, unsigned align, const char* names) {
  if (addrs & (align - 1)) return fail(COALAC_EINVAL, "%s: %s must be %u-byte aligned", who, names, align);
  return COALAC_OK;
}

// the plan's part (also coalac_encode_sr's, which has no stream): NULL, the inputs, the pointers, dense, a code width
int dense_plan_args(coalac_plan_t plan, const char* who, int inputs, const char* null_what, const char* hint) {
  if (!plan) return fail(COALAC_EINVAL, "%s: plan is NULL", who);
  if (inputs != 1) return fail(COALAC_EINVAL, "%s: exactly one of d_in and d_seg_in must be given", who);
  if (null_what) return fail(COALAC_EINVAL, "%s: %s is NULL", who, null_what);
  if (!plan->dense) return fail(COALAC_EINVAL, "%s: needs a dense plan (every k == n)%s", who, hint);
  if (plan->bits == 32) return fail(COALAC_EINVAL, "%s: bits == 32 has no codes (the fp32 values travel as they are)", who);
  return COALAC_OK;
}

// *done: nothing to launch (a plan without units)
int dense_stream_args(coalac_plan_t plan, const DenseCall& c, bool* done) {
  *done = false;
  int rc = dense_plan_args(plan, c.who, c.inputs, c.null_what, c.hint);
  if (rc) return rc;
  if (c.packed_bytes < 4 * plan->dense_words)
    return fail(COALAC_EINVAL, "%s: packed_bytes=%llu < the plan's %llu", c.who, (unsigned long long)c.packed_bytes,
                (unsigned long long)(4 * plan->dense_words));
  if ((rc = misaligned(c.who, c.a16, 16, c.names16)) || (rc = misaligned(c.who, c.a4, 4, c.names4))) return rc;
  *done = plan->proto.n_units == 0;
  return *done ? COALAC_OK : check_device(plan);
}

// f(b, t...) with the code width as a std::integral_constant<uint32_t, b>, b in [B, 8] (B = 0: k_pack's raw plans,
// which carry no code), and one std::bool_constant per flag behind it (with_flags): a launch is one lambda
template <uint32_t B = 1, typename F, typename... Flags>
void with_code_bits(uint32_t b, F&& f, Flags... flags) {
  if (b == B)
    with_flags([&](auto... t) { f(std::integral_constant<uint32_t, B>{}, t...); }, flags...);
  else if constexpr (B < 8)
    with_code_bits<B + 1>(b, f, flags...);
}

// one wave per unit of the plan: kernel(P, args...) on the call's stream
template <typename K, typename... Args>
void launch_units(const Params& P, void* stream, K kernel, Args... args) {
  hipLaunchKernelGGL(kernel, dim3(ceil_div(P.n_units, WAVES)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), P, args...);
}

// the block size of a _g entry point: 4096 forwards to the twin (-1), 256 / 1024 give the plan's table index, anything
// else is an error (-2)
int sub_block_slot(uint32_t block) {
  if (block == UNIT) return -1;
  for (int i = 0; i < 2; ++i)
    if (block == SUB_BLOCKS[i]) return i;
  return -2;
}

int bad_block(const char* who, uint32_t block) {
  return fail(COALAC_EINVAL, "%s: block=%u, need 256, 1024 or 4096", who, block);
}

// f(g) with the block size below the unit as a std::integral_constant<uint32_t, 256 | 1024>
template <typename F>
void with_sub_block(int slot, F&& f) {
  if (slot == 0)
    f(std::integral_constant<uint32_t, SUB_BLOCKS[0]>{});
  else
    f(std::integral_constant<uint32_t, SUB_BLOCKS[1]>{});
}

// The block-wise encoders (coalac_encode_block, _sr, _ef, _g, _rot, _rot_sr), checks and launch: the call's Params,
// then k(P, b, delta, x) with the code width, delta mode and the XCD-aware order as constants — the entry point names its
// kernel there and appends its own arguments. ef: d_resid is required too, and read and written 16 bytes at a time.
template <typename K>
int block_encode(const char* who, const char* hint, coalac_plan_t plan, const float* d_in, const float* const* d_seg_in,
                 const float* d_base, float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, K&& k,
                 bool ef = false, const float* d_resid = nullptr) {
  const char* null_what = ef && !d_resid ? "residual pointer" : !d_bmn || !d_bscale || !d_packed ? A_POINTER : nullptr;
  bool done = false;
  int rc = dense_stream_args(plan, {who, null_what, packed_bytes, addr_bits(d_in, d_base, d_resid),
                                    ef ? "input/base/residual" : "input/base", addr_bits(d_bmn, d_bscale, d_packed),
                                    "bmn / bscale / packed", hint, input_count(d_in, d_seg_in)}, &done);
  if (rc || done) return rc;
  Params P = plan->proto;
  P.in = d_in;
  P.inptr = d_seg_in;
  P.base = d_base;
  with_code_bits((uint32_t)plan->bits, [&](auto b, auto delta, auto x) { k(P, b, delta, x); }, d_base != nullptr,
                 !plan->decode_latency);
  return launched();
}

// The stream decoders (coalac_decode_packed, coalac_decode_block, _g, _rot), checks and launch:
// k_dense_deq_stream with one range per segment or (per_unit) per unit, (slot >= 0) k_dense_deq_stream_g with one
// per block of SUB_BLOCKS[slot] elements, or (rot_seed) k_dense_deq_stream_rot, per unit, with the inverse rotation.
// The per-segment ranges are coalac_decode's: their alignment is not tested.
int decode_stream(const char* who, coalac_plan_t plan, int slot, bool per_unit, const void* d_packed,
                  uint64_t packed_bytes, const float* d_mn, const float* d_scale, const float* d_base, float* d_out,
                  void* stream, const uint64_t* rot_seed = nullptr) {
  const bool blocks = per_unit || slot >= 0;
  bool done = false;
  int rc = dense_stream_args(plan, {who, !d_packed || !d_mn || !d_scale || !d_out ? A_POINTER : nullptr, packed_bytes,
                                    addr_bits(d_out, d_base), "output/base",
                                    blocks ? addr_bits(d_packed, d_mn, d_scale) : addr_bits(d_packed),
                                    blocks ? "packed / bmn / bscale" : "packed", PACK_HINT}, &done);
  if (rc || done) return rc;
  Params P = plan->proto;
  P.base = d_base;
  P.out = d_out;
  const uint32_t bits = (uint32_t)plan->bits, *packed = static_cast<const uint32_t*>(d_packed);
  const bool hb = d_base != nullptr, xcd = !plan->decode_latency;
  if (rot_seed)  // (per unit)
    with_code_bits(
        bits,
        [&](auto b, auto h, auto x) {
          launch_units(P, stream, k_dense_deq_stream_rot<b.value, h.value, x.value>, plan->dense_pw, packed, d_mn,
                       d_scale, *rot_seed);
        },
        hb, xcd);
  else if (slot < 0)
    with_code_bits(
        bits,
        [&](auto b, auto pu, auto h, auto x) {
          launch_units(P, stream, k_dense_deq_stream<b.value, pu.value, h.value, x.value>, plan->dense_pw, packed, d_mn,
                       d_scale);
        },
        per_unit, hb, xcd);
  else
    with_sub_block(slot, [&](auto g) {
      with_code_bits(
          bits,
          [&](auto b, auto h, auto x) {
            launch_units(P, stream, k_dense_deq_stream_g<b.value, h.value, x.value, g.value>, plan->dense_pw,
                         plan->dense_gb[slot], packed, d_mn, d_scale);
          },
          hb, xcd);
    });
  return launched();
}

// The dense aggregates' shared checks, every one ahead of the first device call (*done: nothing to launch). kind is
// coalac_aggregate_dense's argument; the block sizes below the unit read the stream as COALAC_AGGD_BLOCK does.
int agg_dense_args(const char* who, coalac_plan_t plan, int clients, int kind, int mode, const void* const* d_codes,
                   uint64_t code_bytes, const float* const* d_mn, const float* const* d_scale, const float* d_weights,
                   const float* d_base, float* d_out, bool* done) {
  *done = false;
  if (!plan) return fail(COALAC_EINVAL, "%s: plan is NULL", who);
  if (!plan->dense) return fail(COALAC_EINVAL, "%s: needs a dense plan (every k == n); a sparse round is coalac_aggregate's", who);
  if (plan->bits == 32) return fail(COALAC_EINVAL, "%s: bits == 32 has no codes to dequantise", who);
  if (clients < 1) return fail(COALAC_EINVAL, "%s: clients=%d, need at least 1", who, clients);
  if (kind != COALAC_AGGD_CODES && kind != COALAC_AGGD_PACKED && kind != COALAC_AGGD_BLOCK)
    return fail(COALAC_EINVAL, "%s: bad kind %d", who, kind);
  if (mode != COALAC_AGG_DIV && mode != COALAC_AGG_RECIP && mode != COALAC_AGG_SUM)
    return fail(COALAC_EINVAL, "%s: bad mode %d", who, mode);
  if (!d_codes || !d_mn || !d_scale || !d_weights || !d_out) return fail(COALAC_EINVAL, "%s: a pointer is NULL", who);
  const uint64_t need = kind == COALAC_AGGD_CODES ? plan->total_k : 4 * plan->dense_words;
  if (code_bytes < need)
    return fail(COALAC_EINVAL, "%s: code_bytes=%llu < the plan's %llu", who, (unsigned long long)code_bytes,
                (unsigned long long)need);
  if (int rc = misaligned(who, addr_bits(d_out, d_base), 16, "output/base")) return rc;
  if (addr_bits(d_codes, d_mn, d_scale) & 7 || addr_bits(d_weights) & 3)
    return fail(COALAC_EINVAL, "%s: the pointer arrays must be 8-byte, the weights 4-byte aligned", who);
  *done = plan->proto.n_units == 0;
  return *done ? COALAC_OK : check_device(plan);
}

// ... and their launch operands: the call's Params and the kernels' AggDenseArgs; returns the grid
dim3 agg_dense_setup(coalac_plan_t plan, int clients, const void* const* d_codes, const float* const* d_mn,
                     const float* const* d_scale, const float* d_weights, float total, int mode,
                     const uint8_t* d_avg_mask, const float* d_base, float* d_out, Params& P, AggDenseArgs& A) {
  P = plan->proto;
  P.base = d_base;
  P.out = d_out;
  A = AggDenseArgs{};
  A.codes = d_codes;
  A.mn = d_mn;
  A.scale = d_scale;
  A.weights = d_weights;
  A.avg_mask = d_avg_mask;
  A.clients = (uint32_t)clients;
  A.mode = mode;
  A.xcd = !plan->decode_latency;
  A.total = total;
  A.inv_total = 1.0f / total;
  return dim3(ceil_div(P.n_units * (uint32_t)AGD_SPLIT, WAVES));
}

}  // namespace

extern "C" {

int coalac_version(void) { return COALAC_ABI_VERSION; }

const char* coalac_last_error(void) { return g_err.c_str(); }

int coalac_plan_create(const coalac_seg_t* h_segs, int nseg, int bits, coalac_plan_t* out) {
  if (!out) return fail(COALAC_EINVAL, "coalac_plan_create: out is NULL");
  *out = nullptr;
  if (nseg < 0 || (nseg > 0 && !h_segs)) return fail(COALAC_EINVAL, "coalac_plan_create: bad segment table");
  if (!((bits >= 1 && bits <= 8) || bits == 32)) return fail(COALAC_EBITS, "unsupported bits=%d (1..8 or 32)", bits);

  PlanTables T;
  T.segs.resize(nseg);
  uint64_t span = 0, total_k = 0;
  std::vector<std::pair<uint64_t, uint64_t>> in_r, out_r;
  // the table's unit count, before the units exist: it classes the plan, and the class sets the small-segment limit
  // the units are built under (an n the validation below rejects is clamped, so the sum cannot wrap)
  uint64_t n_units = 0;
  for (int s = 0; s < nseg; ++s) n_units += (std::min<uint64_t>(h_segs[s].n, 1ull << 31) + UNIT - 1) / UNIT;
  const bool decode_latency = n_units <= LATENCY_PLAN_UNITS;
  uint32_t small_max = decode_latency ? SMALL_MAX_LATENCY : SMALL_MAX_BATCH;
  if (const char* e = getenv("COALAC_SMALL_MAX")) small_max = std::min<uint32_t>(std::max(atoi(e), 1024), SMALL_MAX);
  for (int s = 0; s < nseg; ++s) {
    const coalac_seg_t& g = h_segs[s];
    if (g.n >= (1ull << 31)) return fail(COALAC_EINVAL, "segment %d: n=%llu >= 2^31", s, (unsigned long long)g.n);
    if (g.in_off % 4)
      return fail(COALAC_EINVAL, "segment %d: in_off=%llu not a multiple of 4", s, (unsigned long long)g.in_off);
    if (g.n == 0 ? g.k != 0 : (g.k < 1 || g.k > g.n))
      return fail(COALAC_EINVAL, "segment %d: k=%llu invalid for n=%llu", s, (unsigned long long)g.k,
                  (unsigned long long)g.n);
    if (g.in_off > (1ull << 46) || g.out_off > (1ull << 46)) return fail(COALAC_EINVAL, "segment %d: offset too large", s);
    SegDev d{};
    d.in_off = g.in_off;
    d.out_off = g.out_off;
    d.n = (uint32_t)g.n;
    d.k = (uint32_t)g.k;
    d.unit_begin = (uint32_t)T.units.size();
    const bool large = g.n > small_max;
    d.lu_begin = large ? (uint32_t)T.lunits.size() : 0u;
    for (uint64_t st = 0; st < g.n; st += UNIT) {
      UnitDev u{};
      u.off = g.in_off + st;
      u.out_off = g.out_off;
      u.seg = (uint32_t)s;
      u.start = (uint32_t)st;
      u.k = (uint32_t)g.k;
      u.len = (uint16_t)std::min<uint64_t>(UNIT, g.n - st);
      u.last = st + UNIT >= g.n ? 1 : 0;
      T.units.push_back(u);
      if (large) T.lunits.push_back(u);
    }
    d.unit_end = (uint32_t)T.units.size();
    if (large) {
      d.g_begin = (uint32_t)T.groups.size();
      const uint32_t nu = d.unit_end - d.unit_begin;
      for (uint32_t g0 = 0; g0 < nu; g0 += GU) {
        T.groups.push_back(make_uint4((uint32_t)T.large_list.size(), d.lu_begin + g0, std::min(GU, nu - g0), (uint32_t)s));
        T.gseg.push_back(make_uint4(d.lu_begin, nu, (uint32_t)g.k, d.g_begin));
      }
    }
    (large ? T.large_list : T.small_list).push_back((uint32_t)s);
    (large ? T.lsegs : T.ssegs).push_back(d);
    T.segs[s] = d;
    if (g.n) {
      span = std::max<uint64_t>(span, g.in_off + g.n);
      total_k = std::max<uint64_t>(total_k, g.out_off + g.k);
      in_r.push_back({g.in_off, g.in_off + g.n});
      out_r.push_back({g.out_off, g.out_off + g.k});
    }
  }
  if (T.lunits.size() >= (1ull << 32) / UNIT)
    return fail(COALAC_EINVAL, "plan too large (%zu large units)", T.lunits.size());
  auto overlaps = [](std::vector<std::pair<uint64_t, uint64_t>>& r) {
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); ++i)
      if (r[i].first < r[i - 1].second) return true;
    return false;
  };
  if (overlaps(in_r)) return fail(COALAC_EINVAL, "segment input ranges overlap");
  if (overlaps(out_r)) return fail(COALAC_EINVAL, "segment output ranges overlap");

  int dev = 0;
  HIP_CHECK(hipGetDevice(&dev));
  coalac_plan* p = new coalac_plan();
  p->device = dev;
  p->bits = bits;
  p->span = span;
  p->total_k = total_k;
  p->hsegs = T.segs;
  Params& M = p->proto;
  M.nseg = (uint32_t)nseg;
  M.n_small = (uint32_t)T.small_list.size();
  M.n_large = (uint32_t)T.large_list.size();
  M.n_units = (uint32_t)T.units.size();
  M.n_lunits = (uint32_t)T.lunits.size();
  M.n_groups = (uint32_t)T.groups.size();
  M.levels = bits == 32 ? 0.0f : (float)((1u << bits) - 1u);
  // record slots per large unit: the candidates a unit can expect at the plan's largest ratio (kept
  // share + the sampled band + margin), so the workspace is ~1 B/element at ratio 0.01 instead of 8
  double rmax = 0.0;
  for (const SegDev& d : T.lsegs) rmax = std::max(rmax, (double)d.k / (double)d.n);
  uint32_t ccap = (uint32_t)align_up((size_t)(UNIT * std::min(1.0, 2.0 * rmax + 0.05) + 256.0), 64);
  if (const char* e = getenv("COALAC_CCAP")) ccap = (uint32_t)atoi(e);  // tests: force overflow
  M.ccap = std::max<uint32_t>(STAGE_CAP, std::min<uint32_t>(UNIT, ccap));
  p->dense = true;
  for (const SegDev& d : T.segs) p->dense = p->dense && d.k == d.n;
  for (const SegDev& d : T.segs) p->dense_empty = p->dense_empty || d.unit_begin == d.unit_end;
  p->encode_latency = M.n_lunits <= LATENCY_PLAN_UNITS;
  p->decode_latency = decode_latency;
  p->high_ratio = rmax > HIGH_RATIO;
  p->small_1k = small_max <= SMALL_MAX_LATENCY;
  p->fork_sized = M.n_small && M.n_lunits >= FORK_MIN_LUNITS;
  p->ws_bytes = carve_workspace(M, p->dense, nullptr);
  // a dense plan's bit-packed code stream (wire v4): each segment row's word offset, behind the tables in the plan's
  // one allocation (the stream's kernels take the array as an argument of their own: it is not in Params)
  std::vector<uint64_t> dense_pw, dense_gb[2];
  if (p->dense && bits != 32) {
    dense_pw.reserve(T.segs.size());
    for (const SegDev& d : T.segs) {
      dense_pw.push_back(p->dense_words);
      p->dense_words += ((uint64_t)d.n * (uint64_t)bits + 31u) / 32u;
      for (int i = 0; i < 2; ++i) {  // (the block tables of DESIGN.md §20, in the same row order)
        dense_gb[i].push_back(p->n_blocks[i]);
        p->n_blocks[i] += ceil_div(d.n, SUB_BLOCKS[i]);
      }
    }
  }

  const size_t tables = place_tables(T, M, nullptr, nullptr);
  const size_t pw_bytes = align_up(sizeof(uint64_t) * dense_pw.size(), 256);
  const size_t bytes = tables + 3 * pw_bytes;
  std::vector<uint8_t> host(bytes, 0);
  hipError_t e = hipMalloc(&p->meta, bytes);
  if (e != hipSuccess) {
    delete p;
    return fail(COALAC_ENOMEM, "hipMalloc(%zu) for plan metadata failed: %s", bytes, hipGetErrorString(e));
  }
  place_tables(T, M, host.data(), static_cast<const uint8_t*>(p->meta));
  if (!dense_pw.empty()) {
    memcpy(host.data() + tables, dense_pw.data(), sizeof(uint64_t) * dense_pw.size());
    p->dense_pw = reinterpret_cast<const uint64_t*>(static_cast<const uint8_t*>(p->meta) + tables);
    for (int i = 0; i < 2; ++i) {
      const size_t at = tables + (1 + i) * pw_bytes;
      memcpy(host.data() + at, dense_gb[i].data(), sizeof(uint64_t) * dense_gb[i].size());
      p->dense_gb[i] = reinterpret_cast<const uint64_t*>(static_cast<const uint8_t*>(p->meta) + at);
    }
  }
  e = hipMemcpy(p->meta, host.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p->meta);
    delete p;
    return fail(COALAC_EHIP, "hipMemcpy of plan metadata failed: %s", hipGetErrorString(e));
  }
  *out = p;
  return COALAC_OK;
}

int coalac_plan_destroy(coalac_plan_t plan) {
  if (!plan) return COALAC_OK;
  int cur = 0;
  if (hipGetDevice(&cur) == hipSuccess && cur != plan->device) (void)hipSetDevice(plan->device);
  hipError_t e = hipFree(plan->meta);
  if (plan->side) (void)hipStreamDestroy(plan->side);
  if (plan->fork) (void)hipEventDestroy(plan->fork);
  if (plan->join) (void)hipEventDestroy(plan->join);
  if (cur != plan->device) (void)hipSetDevice(cur);
  delete plan;
  if (e != hipSuccess) return fail(COALAC_EHIP, "hipFree failed: %s", hipGetErrorString(e));
  return COALAC_OK;
}

int coalac_plan_query(coalac_plan_t plan, uint64_t* ws_bytes, uint64_t* total_k, uint64_t* span, uint64_t* n_units) {
  if (!plan) return fail(COALAC_EINVAL, "coalac_plan_query: plan is NULL");
  if (ws_bytes) *ws_bytes = plan->ws_bytes;
  if (total_k) *total_k = plan->total_k;
  if (span) *span = plan->span;
  if (n_units) *n_units = plan->proto.n_units;
  return COALAC_OK;
}

int coalac_encode_ev(coalac_plan_t plan, const float* d_in, const float* d_base, int32_t* d_idx,
                     void* d_vals, float* d_mn, float* d_scale, uint32_t* d_ustart, void* d_ws, uint64_t ws_bytes,
                     unsigned flags, void* stream, void* const* events) {
  return encode_impl(plan, d_in, nullptr, d_base, d_idx, d_vals, d_mn, d_scale, d_ustart, d_ws, ws_bytes, flags, stream,
                     Marks{events, 5});
}

int coalac_encode_segptr(coalac_plan_t plan, const float* const* d_seg_in, const float* d_base, int32_t* d_idx,
                         void* d_vals, float* d_mn, float* d_scale, uint32_t* d_ustart, void* d_ws, uint64_t ws_bytes,
                         unsigned flags, void* stream) {
  if (plan && plan->proto.nseg && !d_seg_in) return fail(COALAC_EINVAL, "coalac_encode_segptr: d_seg_in is NULL");
  return encode_impl(plan, nullptr, d_seg_in, d_base, d_idx, d_vals, d_mn, d_scale, d_ustart, d_ws, ws_bytes, flags,
                     stream, Marks{nullptr, 0});
}

int coalac_encode(coalac_plan_t plan, const float* d_in, const float* d_base, int32_t* d_idx, void* d_vals,
                  float* d_mn, float* d_scale, uint32_t* d_ustart, void* d_ws, uint64_t ws_bytes, unsigned flags,
                  void* stream) {
  return coalac_encode_ev(plan, d_in, d_base, d_idx, d_vals, d_mn, d_scale, d_ustart, d_ws, ws_bytes, flags, stream,
                          nullptr);
}

int coalac_decode_ev(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, const float* d_mn,
                     const float* d_scale, const uint32_t* d_ustart, const float* d_base, float* d_out, void* stream,
                     void* const* events) {
  if (!plan) return fail(COALAC_EINVAL, "coalac_decode: plan is NULL");
  if (plan->proto.n_units == 0) return COALAC_OK;
  if (!d_out) return fail(COALAC_EINVAL, "coalac_decode: output pointer is NULL");
  // a sparse plan decodes every unit's entry range from the per-unit starts (wire v2; the host computes them for a
  // v1 payload); a dense plan's indices and starts are implied (neither is read)
  if (plan->total_k && (!(plan->dense || (d_idx && d_ustart)) || !d_vals))
    return fail(COALAC_EINVAL, "coalac_decode: idx/vals/ustart pointers are NULL (a sparse plan needs the per-unit "
                "starts of wire v2)");
  if (plan->total_k && plan->bits != 32 && (!d_mn || !d_scale))
    return fail(COALAC_EINVAL, "coalac_decode: mn/scale pointers are NULL");
  if (addr_bits(d_out, d_base) & 15) return fail(COALAC_EINVAL, "coalac_decode: output/base must be 16-byte aligned");
  if (addr_bits(d_ustart) & 3) return fail(COALAC_EINVAL, "coalac_decode: ustart must be 4-byte aligned");
  int rc = check_device(plan);
  if (rc) return rc;
  Params P = plan->proto;
  set_payload(P, d_idx, d_vals, d_mn, d_scale);
  P.base = d_base;
  P.out = d_out;
  P.ustart = d_ustart;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool raw = plan->bits == 32, hb = d_base != nullptr;
  const Marks marks{events, 3};
  MARK(0);
  MARK(1);
  if (plan->dense)  // every element kept: one positional dequantise stream
    with_flags(
        [&](auto r, auto h, auto x) {
          hipLaunchKernelGGL((k_dense_deq<r.value, h.value, x.value>), dim3(ceil_div(P.n_units, WAVES)), dim3(BLOCK), 0, st,
                             P);
        },
        raw, hb, !plan->decode_latency);
  else
    with_flags([&](auto r, auto h, auto hr) { launch_decode_lds<r.value, h.value, hr.value>(P, plan, st); }, raw, hb,
               plan->high_ratio);
  MARK(2);
  return launched();
}

int coalac_decode(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, const float* d_mn,
                  const float* d_scale, const uint32_t* d_ustart, const float* d_base, float* d_out, void* stream) {
  return coalac_decode_ev(plan, d_idx, d_vals, d_mn, d_scale, d_ustart, d_base, d_out, stream, nullptr);
}

int coalac_ef_accumulate(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                         float* d_resid, void* stream) {
  // (the argument checks come before any use of the plan)
  if (!plan) return fail(COALAC_EINVAL, "coalac_ef_accumulate: plan is NULL");
  if ((d_in != nullptr) == (d_seg_in != nullptr))
    return fail(COALAC_EINVAL, "coalac_ef_accumulate: exactly one of d_in and d_seg_in must be given");
  if (!d_resid) return fail(COALAC_EINVAL, "coalac_ef_accumulate: residual pointer is NULL");
  if (addr_bits(d_in, d_base, d_resid) & 15)
    return fail(COALAC_EINVAL, "coalac_ef_accumulate: input/base/residual must be 16-byte aligned");
  if (plan->proto.n_units == 0) return COALAC_OK;
  int rc = check_device(plan);
  if (rc) return rc;
  Params P = plan->proto;
  P.in = d_in;
  P.inptr = d_seg_in;
  P.base = d_base;
  P.out = d_resid;
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_flags(
      [&](auto hb) {
        hipLaunchKernelGGL((k_ef_accumulate<hb.value>), dim3(ceil_div(P.n_units, WAVES)), dim3(BLOCK), 0, st, P);
      },
      d_base != nullptr);
  return launched();
}

int coalac_ef_commit(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, const float* d_mn,
                     const float* d_scale, const uint32_t* d_ustart, float* d_resid, void* stream) {
  if (!plan) return fail(COALAC_EINVAL, "coalac_ef_commit: plan is NULL");
  if (plan->proto.n_units == 0 || plan->total_k == 0) return COALAC_OK;
  if (!d_resid) return fail(COALAC_EINVAL, "coalac_ef_commit: residual pointer is NULL");
  if (!(plan->dense || (d_idx && d_ustart)) || !d_vals)
    return fail(COALAC_EINVAL, "coalac_ef_commit: idx/vals/ustart pointers are NULL (a sparse plan needs the per-unit "
                "starts the encode wrote)");
  if (plan->bits != 32 && (!d_mn || !d_scale)) return fail(COALAC_EINVAL, "coalac_ef_commit: mn/scale pointers are NULL");
  if (addr_bits(d_resid) & 15) return fail(COALAC_EINVAL, "coalac_ef_commit: residual must be 16-byte aligned");
  if (addr_bits(d_ustart) & 3) return fail(COALAC_EINVAL, "coalac_ef_commit: ustart must be 4-byte aligned");
  int rc = check_device(plan);
  if (rc) return rc;
  Params P = plan->proto;
  set_payload(P, d_idx, d_vals, d_mn, d_scale);
  P.ustart = d_ustart;
  P.out = d_resid;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 g(ceil_div(P.n_units, WAVES));
  with_flags(
      [&](auto raw) {
        if (plan->dense)
          hipLaunchKernelGGL((k_ef_commit_dense<raw.value>), g, dim3(BLOCK), 0, st, P);
        else
          hipLaunchKernelGGL((k_ef_commit<raw.value>), g, dim3(BLOCK), 0, st, P);
      },
      plan->bits == 32);
  return launched();
}

int coalac_plan_packed_bytes(coalac_plan_t plan, uint64_t* bytes) {
  if (!plan || !bytes) return fail(COALAC_EINVAL, "coalac_plan_packed_bytes: plan or output pointer is NULL");
  *bytes = 4 * packed_words(plan);
  return COALAC_OK;
}

int coalac_pack(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, void* d_packed, uint64_t packed_bytes,
                void* stream) {
  bool done = false;
  int rc = packed_args(plan, "coalac_pack", !d_idx || !d_vals || !d_packed, packed_bytes, &done);
  if (rc || done) return rc;
  if ((addr_bits(d_idx, d_vals) & 15) || (addr_bits(d_packed) & 3))
    return fail(COALAC_EINVAL, "coalac_pack: idx / vals must be 16-byte aligned, packed 4-byte aligned");
  const uint64_t lanes = (plan->total_k + PACK_E - 1) / PACK_E, blocks = (lanes + BLOCK - 1) / BLOCK;
  if (blocks > 0x7FFFFFFFull) return fail(COALAC_EINVAL, "coalac_pack: plan too large");
  with_code_bits<0>(packed_field_bits(plan) - 12u, [&](auto b) {
    hipLaunchKernelGGL((k_pack<b.value>), dim3((uint32_t)blocks), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), d_idx,
                       static_cast<const uint8_t*>(d_vals), static_cast<uint32_t*>(d_packed), plan->total_k);
  });
  return launched();
}

int coalac_unpack(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const uint32_t* d_ustart,
                  int32_t* d_idx, void* d_vals, void* stream) {
  bool done = false;
  int rc = packed_args(plan, "coalac_unpack", !d_packed || !d_ustart || !d_idx || !d_vals, packed_bytes, &done);
  if (rc || done) return rc;
  if (addr_bits(d_packed, d_ustart, d_idx) & 3)
    return fail(COALAC_EINVAL, "coalac_unpack: packed / ustart / idx must be 4-byte aligned");
  Params P = plan->proto;
  P.ustart = d_ustart;
  P.idx = d_idx;
  P.vals = d_vals;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 g(ceil_div(P.n_units, WAVES));
  const uint32_t* packed = static_cast<const uint32_t*>(d_packed);
  with_flags(
      [&](auto raw) {
        hipLaunchKernelGGL((k_unpack<raw.value>), g, dim3(BLOCK), 0, st, P, packed, packed_bytes / 4,
                           packed_field_bits(plan));
      },
      plan->bits == 32);
  return launched();
}

int coalac_plan_dense_packed_bytes(coalac_plan_t plan, uint64_t* bytes) {
  if (!plan || !bytes) return fail(COALAC_EINVAL, "coalac_plan_dense_packed_bytes: plan or output pointer is NULL");
  if (!plan->dense || plan->bits == 32)
    return fail(COALAC_EINVAL, "coalac_plan_dense_packed_bytes: needs a dense plan (every k == n) with bits 1..8");
  *bytes = 4 * plan->dense_words;
  return COALAC_OK;
}

int coalac_pack_dense(coalac_plan_t plan, const void* d_vals, void* d_packed, uint64_t packed_bytes, void* stream) {
  bool done = false;
  int rc = dense_stream_args(plan, {"coalac_pack_dense", !d_vals || !d_packed ? A_POINTER : nullptr, packed_bytes, 0, "",
                                    addr_bits(d_packed, d_vals), "vals / packed", PACK_HINT}, &done);
  if (rc || done) return rc;
  with_code_bits((uint32_t)plan->bits, [&](auto b) {
    launch_units(plan->proto, stream, k_pack_dense<b.value>, plan->dense_pw, static_cast<const uint8_t*>(d_vals),
                 static_cast<uint32_t*>(d_packed));
  });
  return launched();
}

int coalac_unpack_dense(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, void* d_vals, void* stream) {
  bool done = false;
  int rc = dense_stream_args(plan, {"coalac_unpack_dense", !d_packed || !d_vals ? A_POINTER : nullptr, packed_bytes, 0, "",
                                    addr_bits(d_packed, d_vals), "packed / vals", PACK_HINT}, &done);
  if (rc || done) return rc;
  with_code_bits((uint32_t)plan->bits, [&](auto b) {
    launch_units(plan->proto, stream, k_unpack_dense<b.value>, plan->dense_pw, static_cast<const uint32_t*>(d_packed),
                 static_cast<uint8_t*>(d_vals));
  });
  return launched();
}

int coalac_decode_packed(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const float* d_mn,
                         const float* d_scale, const float* d_base, float* d_out, void* stream) {
  return decode_stream("coalac_decode_packed", plan, -1, false, d_packed, packed_bytes, d_mn, d_scale, d_base, d_out, stream);
}

int coalac_encode_block(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                        float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, void* stream) {
  return block_encode("coalac_encode_block", PACK_HINT, plan, d_in, d_seg_in, d_base, d_bmn, d_bscale, d_packed, packed_bytes,
                      [&](const Params& P, auto b, auto delta, auto x) {
                        launch_units(P, stream, k_dense_block_quant<delta.value, b.value, x.value>, plan->dense_pw, d_bmn,
                                     d_bscale, static_cast<uint32_t*>(d_packed));
                      });
}

int coalac_encode_sr(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                     void* d_vals, float* d_mn, float* d_scale, void* d_ws, uint64_t ws_bytes, uint64_t seed,
                     unsigned flags, void* stream) {
  // (no stream: the plan's part of the family's checks, then its own, every one ahead of the first device call)
  int rc = dense_plan_args(plan, "coalac_encode_sr", input_count(d_in, d_seg_in), nullptr, SR_HINT);
  if (rc) return rc;
  if (plan->proto.nseg == 0) return COALAC_OK;
  if (!d_mn || !d_scale) return fail(COALAC_EINVAL, "coalac_encode_sr: mn/scale pointers are NULL");
  if (plan->total_k && !d_vals) return fail(COALAC_EINVAL, "coalac_encode_sr: the vals pointer is NULL");
  if ((rc = misaligned("coalac_encode_sr", addr_bits(d_in, d_base), 16, "input/base"))) return rc;
  if (!d_ws || ws_bytes < plan->ws_bytes)
    return fail(COALAC_EWORKSPACE, "coalac_encode_sr: workspace %llu < required %llu", (unsigned long long)ws_bytes,
                (unsigned long long)plan->ws_bytes);
  rc = check_device(plan);
  if (rc) return rc;
  Params P = plan->proto;
  P.in = d_in;
  P.inptr = d_seg_in;
  P.base = d_base;
  P.idx = nullptr;  // (implied, as the per-unit starts are)
  P.vals = d_vals;
  P.mn = d_mn;
  P.scale = d_scale;
  P.ustart_out = nullptr;
  P.flags = flags;
  carve_workspace(P, true, d_ws);
  P.stamps = nullptr;
  with_flags([&](auto delta) { launch_dense_encode_sr<delta.value>(P, plan, static_cast<hipStream_t>(stream), seed); },
             d_base != nullptr);
  return launched();
}

int coalac_encode_block_sr(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                           float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, uint64_t seed,
                           void* stream) {
  return block_encode("coalac_encode_block_sr", SR_HINT, plan, d_in, d_seg_in, d_base, d_bmn, d_bscale, d_packed, packed_bytes,
                      [&](const Params& P, auto b, auto delta, auto x) {
                        launch_units(P, stream, k_dense_block_quant_sr<delta.value, b.value, x.value>, plan->dense_pw,
                                     d_bmn, d_bscale, static_cast<uint32_t*>(d_packed), seed);
                      });
}

int coalac_encode_block_ef(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                           float* d_resid, float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes,
                           void* stream) {
  return block_encode(
      "coalac_encode_block_ef", EF_HINT, plan, d_in, d_seg_in, d_base, d_bmn, d_bscale, d_packed, packed_bytes,
      [&](const Params& P, auto b, auto hb, auto x) {
        launch_units(P, stream, k_dense_block_quant_ef<hb.value, b.value, x.value>, plan->dense_pw, d_bmn, d_bscale,
                     static_cast<uint32_t*>(d_packed), d_resid);
      },
      true, d_resid);
}

int coalac_decode_block(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const float* d_bmn,
                        const float* d_bscale, const float* d_base, float* d_out, void* stream) {
  return decode_stream("coalac_decode_block", plan, -1, true, d_packed, packed_bytes, d_bmn, d_bscale, d_base, d_out, stream);
}

int coalac_encode_block_rot(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                            float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, uint64_t rot_seed,
                            void* stream) {
  return block_encode("coalac_encode_block_rot", PACK_HINT, plan, d_in, d_seg_in, d_base, d_bmn, d_bscale, d_packed,
                      packed_bytes, [&](const Params& P, auto b, auto delta, auto x) {
                        launch_units(P, stream, k_dense_block_quant_rot<delta.value, b.value, x.value, false>,
                                     plan->dense_pw, d_bmn, d_bscale, static_cast<uint32_t*>(d_packed), rot_seed,
                                     (uint64_t)0);
                      });
}

int coalac_encode_block_rot_sr(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                               float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, uint64_t rot_seed,
                               uint64_t seed, void* stream) {
  return block_encode("coalac_encode_block_rot_sr", SR_HINT, plan, d_in, d_seg_in, d_base, d_bmn, d_bscale, d_packed,
                      packed_bytes, [&](const Params& P, auto b, auto delta, auto x) {
                        launch_units(P, stream, k_dense_block_quant_rot<delta.value, b.value, x.value, true>,
                                     plan->dense_pw, d_bmn, d_bscale, static_cast<uint32_t*>(d_packed), rot_seed, seed);
                      });
}

int coalac_decode_block_rot(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const float* d_bmn,
                            const float* d_bscale, uint64_t rot_seed, const float* d_base, float* d_out, void* stream) {
  return decode_stream("coalac_decode_block_rot", plan, -1, true, d_packed, packed_bytes, d_bmn, d_bscale, d_base, d_out,
                       stream, &rot_seed);
}

int coalac_plan_block_count(coalac_plan_t plan, uint32_t block, uint64_t* n_blocks) {
  const char* who = "coalac_plan_block_count";
  if (!plan || !n_blocks) return fail(COALAC_EINVAL, "%s: plan or output pointer is NULL", who);
  if (!plan->dense || plan->bits == 32)
    return fail(COALAC_EINVAL, "%s: needs a dense plan (every k == n) with bits 1..8", who);
  const int slot = sub_block_slot(block);
  if (slot == -2) return bad_block(who, block);
  *n_blocks = slot < 0 ? plan->proto.n_units : plan->n_blocks[slot];
  return COALAC_OK;
}

int coalac_encode_block_g(coalac_plan_t plan, uint32_t block, const float* d_in, const float* const* d_seg_in,
                          const float* d_base, float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes,
                          void* stream) {
  const char* who = "coalac_encode_block_g";
  const int slot = sub_block_slot(block);
  if (slot == -2) return bad_block(who, block);
  if (slot < 0) return coalac_encode_block(plan, d_in, d_seg_in, d_base, d_bmn, d_bscale, d_packed, packed_bytes, stream);
  int rc = COALAC_OK;
  with_sub_block(slot, [&](auto g) {
    rc = block_encode(who, PACK_HINT, plan, d_in, d_seg_in, d_base, d_bmn, d_bscale, d_packed, packed_bytes,
                      [&](const Params& P, auto b, auto delta, auto x) {
                        launch_units(P, stream, k_dense_block_quant_g<delta.value, b.value, x.value, g.value>,
                                     plan->dense_pw, plan->dense_gb[slot], d_bmn, d_bscale, static_cast<uint32_t*>(d_packed));
                      });
  });
  return rc;
}

int coalac_decode_block_g(coalac_plan_t plan, uint32_t block, const void* d_packed, uint64_t packed_bytes,
                          const float* d_bmn, const float* d_bscale, const float* d_base, float* d_out, void* stream) {
  const char* who = "coalac_decode_block_g";
  const int slot = sub_block_slot(block);
  if (slot == -2) return bad_block(who, block);
  if (slot < 0) return coalac_decode_block(plan, d_packed, packed_bytes, d_bmn, d_bscale, d_base, d_out, stream);
  return decode_stream(who, plan, slot, false, d_packed, packed_bytes, d_bmn, d_bscale, d_base, d_out, stream);
}

int coalac_aggregate_ev(coalac_plan_t plan, int clients, const int32_t* d_idx, const void* d_vals,
                        const float* d_mn, const float* d_scale, const uint32_t* d_ustart, const float* d_weights,
                        float total, int mode,
                        const uint8_t* d_avg_mask, const float* d_base, float* d_out, void* stream,
                        void* const* events) {
  if (!plan) return fail(COALAC_EINVAL, "coalac_aggregate: plan is NULL");
  const int nseg = (int)plan->proto.nseg;
  const uint32_t n_units = plan->proto.n_units;
  if (clients < 1 || nseg % clients)
    return fail(COALAC_EINVAL, "coalac_aggregate: %d segments are not %d copies of one layout", nseg, clients);
  if (mode != COALAC_AGG_DIV && mode != COALAC_AGG_RECIP && mode != COALAC_AGG_SUM)
    return fail(COALAC_EINVAL, "coalac_aggregate: bad mode %d", mode);
  if (n_units == 0) return COALAC_OK;
  if (!d_out || !d_weights) return fail(COALAC_EINVAL, "coalac_aggregate: output/weights pointer is NULL");
  if (plan->total_k && (!d_idx || !d_vals || !d_ustart))
    return fail(COALAC_EINVAL, "coalac_aggregate: idx/vals/ustart pointers are NULL (the per-unit starts of wire v2; a "
                "dense plan's implied indices and starts must be passed here)");
  if (plan->bits != 32 && (!d_mn || !d_scale)) return fail(COALAC_EINVAL, "coalac_aggregate: mn/scale pointers are NULL");
  if (addr_bits(d_out, d_base) & 15) return fail(COALAC_EINVAL, "coalac_aggregate: output/base must be 16-byte aligned");
  if (addr_bits(d_ustart) & 3) return fail(COALAC_EINVAL, "coalac_aggregate: ustart must be 4-byte aligned");
  // the table must be `clients` copies of one layout at constant input / output strides
  const uint32_t T = (uint32_t)(nseg / clients);
  const std::vector<SegDev>& H = plan->hsegs;
  const uint32_t U0 = n_units / (uint32_t)clients;
  if (n_units % (uint32_t)clients) return fail(COALAC_EINVAL, "coalac_aggregate: unit count not divisible");
  const uint64_t S = clients > 1 ? H[T].in_off - H[0].in_off : 0, Kc = clients > 1 ? H[T].out_off - H[0].out_off : 0;
  for (uint32_t c = 1; c < (uint32_t)clients; ++c)
    for (uint32_t t = 0; t < T; ++t) {
      const SegDev &a = H[t], &b = H[c * T + t];
      if (b.n != a.n || b.k != a.k || b.in_off != a.in_off + c * S || b.out_off != a.out_off + c * Kc ||
          b.unit_begin != a.unit_begin + c * U0)
        return fail(COALAC_EINVAL, "coalac_aggregate: segment %u of client %u is not a copy of segment %u of client 0",
                    c * T + t, c, t);
    }
  int rc = check_device(plan);
  if (rc) return rc;
  Params P = plan->proto;
  set_payload(P, d_idx, d_vals, d_mn, d_scale);
  P.base = d_base;
  P.out = d_out;
  AggArgs A{};
  A.ustart = d_ustart;
  A.weights = d_weights;
  A.clients = (uint32_t)clients;
  A.T = T;
  A.U0 = U0;
  A.Kc = Kc;
  A.total = total;
  A.inv_total = 1.0f / total;
  A.avg_mask = d_avg_mask;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const Marks marks{events, 3};
  MARK(0);
  MARK(1);
  with_flags(
      [&](auto raw, auto hb) {
        with_agg_mode(mode, [&](auto m) {
          hipLaunchKernelGGL((k_aggregate<raw.value, hb.value, m.value>), dim3(ceil_div(U0 * AGG_SPLIT, WAVES)),
                             dim3(BLOCK), 0, st, P, A);
        });
      },
      plan->bits == 32, d_base != nullptr);
  MARK(2);
  return launched();
}

int coalac_aggregate(coalac_plan_t plan, int clients, const int32_t* d_idx, const void* d_vals, const float* d_mn,
                     const float* d_scale, const uint32_t* d_ustart, const float* d_weights, float total, int mode,
                     const uint8_t* d_avg_mask, const float* d_base, float* d_out, void* stream) {
  return coalac_aggregate_ev(plan, clients, d_idx, d_vals, d_mn, d_scale, d_ustart, d_weights, total, mode, d_avg_mask,
                             d_base, d_out, stream, nullptr);
}

int coalac_aggregate_dense(coalac_plan_t plan, int clients, int kind, const void* const* d_codes, uint64_t code_bytes,
                           const float* const* d_mn, const float* const* d_scale, const float* d_weights, float total,
                           int mode, const uint8_t* d_avg_mask, const float* d_base, float* d_out, void* stream) {
  bool done = false;
  int rc = agg_dense_args("coalac_aggregate_dense", plan, clients, kind, mode, d_codes, code_bytes, d_mn, d_scale,
                          d_weights, d_base, d_out, &done);
  if (rc || done) return rc;
  Params P;
  AggDenseArgs A;
  const dim3 g =
      agg_dense_setup(plan, clients, d_codes, d_mn, d_scale, d_weights, total, mode, d_avg_mask, d_base, d_out, P, A);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // One with_code_bits for the three kinds. CODES ignores the width it is handed: its codes are whole bytes, so all
  // eight arms launch the same <8, CODES, hb>, and it relies on bits being in [1, 8] here (agg_dense_args rejects 32) —
  // a width outside that range would launch nothing.
  auto launch = [&](auto k) {
    with_code_bits(
        (uint32_t)plan->bits,
        [&](auto b, auto hb) {
          constexpr int KIND = decltype(k)::value;
          constexpr uint32_t B = KIND == COALAC_AGGD_CODES ? 8u : decltype(b)::value;  // (CODES: whole bytes at any width)
          hipLaunchKernelGGL((k_aggregate_dense<B, KIND, hb.value>), g, dim3(BLOCK), 0, st, P, plan->dense_pw, A);
        },
        d_base != nullptr);
  };
  if (kind == COALAC_AGGD_CODES)
    launch(std::integral_constant<int, COALAC_AGGD_CODES>{});
  else if (kind == COALAC_AGGD_PACKED)
    launch(std::integral_constant<int, COALAC_AGGD_PACKED>{});
  else
    launch(std::integral_constant<int, COALAC_AGGD_BLOCK>{});
  return launched();
}

int coalac_aggregate_dense_g(coalac_plan_t plan, int clients, uint32_t block, const void* const* d_codes,
                             uint64_t code_bytes, const float* const* d_mn, const float* const* d_scale,
                             const float* d_weights, float total, int mode, const uint8_t* d_avg_mask,
                             const float* d_base, float* d_out, void* stream) {
  const char* who = "coalac_aggregate_dense_g";
  const int slot = sub_block_slot(block);
  if (slot == -2) return bad_block(who, block);
  if (slot < 0)
    return coalac_aggregate_dense(plan, clients, COALAC_AGGD_BLOCK, d_codes, code_bytes, d_mn, d_scale, d_weights, total,
                                  mode, d_avg_mask, d_base, d_out, stream);
  bool done = false;
  int rc = agg_dense_args(who, plan, clients, COALAC_AGGD_BLOCK, mode, d_codes, code_bytes, d_mn, d_scale, d_weights,
                          d_base, d_out, &done);
  if (rc || done) return rc;
  Params P;
  AggDenseArgs A;
  const dim3 grid =
      agg_dense_setup(plan, clients, d_codes, d_mn, d_scale, d_weights, total, mode, d_avg_mask, d_base, d_out, P, A);
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_sub_block(slot, [&](auto g) {
    with_code_bits(
        (uint32_t)plan->bits,
        [&](auto b, auto hb) {
          hipLaunchKernelGGL((k_aggregate_dense_g<b.value, hb.value, g.value>), grid, dim3(BLOCK), 0, st, P,
                             plan->dense_pw, plan->dense_gb[slot], A);
        },
        d_base != nullptr);
  });
  return launched();
}

int coalac_aggregate_uploads(coalac_plan_t plan, int clients, int kind, const int32_t* const* d_idx,
                             const void* const* d_packed, uint64_t packed_bytes, const void* const* d_vals,
                             const float* const* d_mn, const float* const* d_scale, const uint32_t* const* d_ustart,
                             const float* d_weights, float total, int mode, const uint8_t* d_avg_mask,
                             const float* d_base, float* d_out, void* stream) {
  const char* who = "coalac_aggregate_uploads";
  if (!plan) return fail(COALAC_EINVAL, "%s: plan is NULL", who);
  // (a plan without units is dense by definition and has nothing to aggregate: OK below)
  if (plan->dense && plan->proto.n_units)
    return fail(COALAC_EINVAL, "%s: a dense plan (every k == n) is coalac_aggregate_dense's", who);
  if (clients < 1) return fail(COALAC_EINVAL, "%s: clients=%d, need at least 1", who, clients);
  if (kind != COALAC_AGGS_ENTRIES && kind != COALAC_AGGS_COMPACT) return fail(COALAC_EINVAL, "%s: bad kind %d", who, kind);
  if (mode != COALAC_AGG_DIV && mode != COALAC_AGG_RECIP && mode != COALAC_AGG_SUM)
    return fail(COALAC_EINVAL, "%s: bad mode %d", who, mode);
  if (plan->proto.n_units == 0) return COALAC_OK;
  const bool raw = plan->bits == 32, compact = kind == COALAC_AGGS_COMPACT;
  if (!d_ustart || !d_weights || !d_out) return fail(COALAC_EINVAL, "%s: ustart/weights/output pointer is NULL", who);
  if (compact ? !d_packed : !d_idx) return fail(COALAC_EINVAL, "%s: the %s pointer array is NULL", who, compact ? "packed" : "idx");
  if ((!compact || raw) && !d_vals) return fail(COALAC_EINVAL, "%s: the vals pointer array is NULL", who);
  if (!raw && (!d_mn || !d_scale)) return fail(COALAC_EINVAL, "%s: mn/scale pointer arrays are NULL", who);
  const uint64_t need = 4 * packed_words(plan);
  if (compact && packed_bytes < need)
    return fail(COALAC_EINVAL, "%s: packed_bytes=%llu < the plan's %llu", who, (unsigned long long)packed_bytes,
                (unsigned long long)need);
  if (addr_bits(d_out, d_base) & 15) return fail(COALAC_EINVAL, "%s: output/base must be 16-byte aligned", who);
  if ((addr_bits(d_idx, d_packed, d_vals) | addr_bits(d_mn, d_scale, d_ustart)) & 7 || addr_bits(d_weights) & 3)
    return fail(COALAC_EINVAL, "%s: the pointer arrays must be 8-byte, the weights 4-byte aligned", who);
  int rc = check_device(plan);
  if (rc) return rc;
  Params P = plan->proto;
  P.base = d_base;
  P.out = d_out;
  AggArgs A{};
  A.weights = d_weights;
  A.clients = (uint32_t)clients;
  A.T = P.nseg;
  A.U0 = P.n_units;
  A.total = total;
  A.inv_total = 1.0f / total;
  A.avg_mask = d_avg_mask;
  AggUploads S{};
  S.idx = d_idx;
  S.packed = reinterpret_cast<const uint32_t* const*>(d_packed);
  S.vals = d_vals;
  S.mn = d_mn;
  S.scale = d_scale;
  S.ustart = d_ustart;
  S.nwords = packed_bytes / 4;
  S.w = packed_field_bits(plan);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto launch = [&](auto src) {
    with_flags(
        [&](auto rw, auto hb) {
          with_agg_mode(mode, [&](auto m) {
            hipLaunchKernelGGL((k_aggregate_uploads<decltype(src)::value, rw.value, hb.value, m.value>),
                               dim3(ceil_div(P.n_units * AGG_SPLIT, WAVES)), dim3(BLOCK), 0, st, P, A, S);
          });
        },
        raw, d_base != nullptr);
  };
  if (compact)
    launch(std::integral_constant<int, AGG_COMPACT>{});
  else
    launch(std::integral_constant<int, AGG_ENTRIES>{});
  return launched();
}

int coalac_gather(const void* const* d_src, int n, int elem_bytes, void* d_out, void* stream) {
  if (n < 0 || (n > 0 && (!d_src || !d_out))) return fail(COALAC_EINVAL, "coalac_gather: bad arguments");
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
    return fail(COALAC_EINVAL, "coalac_gather: element size %d (1, 2, 4 or 8)", elem_bytes);
  if (reinterpret_cast<uintptr_t>(d_out) % (uintptr_t)elem_bytes)
    return fail(COALAC_EINVAL, "coalac_gather: output not aligned to the element size");
  if (n == 0) return COALAC_OK;
  hipLaunchKernelGGL(k_gather, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, static_cast<hipStream_t>(stream), d_src,
                     (uint32_t)n, (uint32_t)elem_bytes, d_out);
  return launched();
}

// The diagnostics read a finished encode's workspace back: the arrays' places come from the same walk as the encode's.
int coalac_workspace_fallbacks(coalac_plan_t plan, const void* d_ws, void* stream, int* out) {
  if (!plan || !d_ws || !out) return fail(COALAC_EINVAL, "coalac_workspace_fallbacks: NULL argument");
  *out = 0;
  if (plan->proto.nseg == 0 || plan->dense) return COALAC_OK;
  Params W = plan->proto;
  carve_workspace(W, false, const_cast<void*>(d_ws));
  std::vector<uint32_t> st(W.nseg);
  std::vector<uint32_t> large(W.n_large);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_CHECK(hipMemcpyAsync(st.data(), W.status, 4 * st.size(), hipMemcpyDeviceToHost, s));
  if (W.n_large) HIP_CHECK(hipMemcpyAsync(large.data(), W.large_list, 4 * large.size(), hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  int c = 0;
  for (uint32_t s2 : large) c += st[s2] == 1;
  *out = c;
  return COALAC_OK;
}

int coalac_debug_brackets(coalac_plan_t plan, const void* d_ws, void* stream, uint32_t* host_tlo, uint32_t* host_thi,
                          int n) {
  if (!plan || !d_ws || !host_tlo || !host_thi || n < 0) return fail(COALAC_EINVAL, "coalac_debug_brackets: bad argument");
  if (plan->dense) return 0;
  Params W = plan->proto;
  carve_workspace(W, false, const_cast<void*>(d_ws));
  const size_t cnt = std::min<size_t>((size_t)n, W.n_lunits);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (cnt) {
    HIP_CHECK(hipMemcpyAsync(host_tlo, W.tlo, 4 * cnt, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(host_thi, W.thi, 4 * cnt, hipMemcpyDeviceToHost, s));
  }
  HIP_CHECK(hipStreamSynchronize(s));
  return (int)cnt;
}

int coalac_debug_stamps(coalac_plan_t plan, const void* d_ws, void* stream, uint64_t* host, int n) {
  if (!plan || !d_ws || !host || n < 0) return fail(COALAC_EINVAL, "coalac_debug_stamps: bad argument");
  if (plan->dense) return 0;  // (a dense plan's workspace has no stamp rows)
  Params W = plan->proto;
  carve_workspace(W, false, const_cast<void*>(d_ws));
  const size_t cap = (size_t)NSTAMP * std::max<size_t>(W.nseg, 1);
  const size_t cnt = std::min<size_t>((size_t)n, cap);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HIP_CHECK(hipMemcpyAsync(host, W.stamps, 8 * cnt, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  return (int)cnt;
}

}  // extern "C"
