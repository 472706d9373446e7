// Host-side checks of coalac.hip that need no device, meant to be built with the host sanitizers
// (tests/test_host_sanitized.py builds and runs it): every plan-validation error, the NULL-argument cases of every
// entry point, every argument check of coalac_pack_dense / coalac_unpack_dense / coalac_decode_packed (on plans in host
// memory), and the workspace / plan-table walks against independently stated sizes — with real host buffers of
// exactly the walked size, every array written end to end, so an array the walk sized too small is an overrun the
// sanitizer reports. The codec source is included, not linked: the walks live in its anonymous namespace.
#include "../coala_amd/csrc/coalac.hip"

#include <cinttypes>

#include "host_check_common.h"

static void plan_validation() {
  struct Row {
    std::vector<coalac_seg_t> segs;  // {in_off, n, k, out_off}
    int bits, code;
    const char* msg;
  };
  const Row rows[] = {  // the rows of tests/test_abi.py::test_plan_validation
      {{{0, 10, 1, 0}}, 9, COALAC_EBITS, "bits"},
      {{{2, 10, 1, 0}}, 8, COALAC_EINVAL, "multiple of 4"},
      {{{0, 10, 0, 0}}, 8, COALAC_EINVAL, "k="},
      {{{0, 10, 11, 0}}, 8, COALAC_EINVAL, "k="},
      {{{0, 0, 1, 0}}, 8, COALAC_EINVAL, "k="},
      {{{0, 10, 2, 0}, {8, 10, 2, 2}}, 8, COALAC_EINVAL, "input ranges overlap"},
      {{{0, 10, 2, 0}, {16, 10, 2, 1}}, 8, COALAC_EINVAL, "output ranges overlap"},
      {{{0, 1ull << 31, 1, 0}}, 8, COALAC_EINVAL, ">= 2^31"},
      // the first invalid segment reports, after valid ones of every class were built
      {{{0, 300, 3, 0}, {4096, 70001, 700, 3}, {80000, 10, 11, 703}}, 8, COALAC_EINVAL, "segment 2: k="},
      {{{0, 10, 1, 0}, {16, 10, 1, 1ull << 47}}, 8, COALAC_EINVAL, "offset too large"},
  };
  for (const Row& r : rows) {
    coalac_plan_t h = reinterpret_cast<coalac_plan_t>(1);
    const int rc = coalac_plan_create(r.segs.data(), (int)r.segs.size(), r.bits, &h);
    CHECK(rc == r.code && says(r.msg) && h == nullptr);
  }
}

static void null_arguments() {
  coalac_plan_t h = nullptr;
  coalac_seg_t seg{0, 10, 1, 0};
  CHECK(coalac_plan_create(&seg, 1, 8, nullptr) == COALAC_EINVAL && says("out is NULL"));
  CHECK(coalac_plan_create(nullptr, 1, 8, &h) == COALAC_EINVAL && says("bad segment table"));
  CHECK(coalac_plan_create(&seg, -1, 8, &h) == COALAC_EINVAL && says("bad segment table"));
  CHECK(coalac_plan_destroy(nullptr) == COALAC_OK);
  CHECK(coalac_plan_query(nullptr, nullptr, nullptr, nullptr, nullptr) == COALAC_EINVAL && says("coalac_plan_query"));
  const auto N = nullptr;
  CHECK(coalac_encode(N, N, N, N, N, N, N, N, N, 0, 0, N) == COALAC_EINVAL && says("coalac_encode: plan is NULL"));
  CHECK(coalac_encode_ev(N, N, N, N, N, N, N, N, N, 0, 0, N, N) == COALAC_EINVAL && says("coalac_encode: plan is NULL"));
  CHECK(coalac_encode_segptr(N, N, N, N, N, N, N, N, N, 0, 0, N) == COALAC_EINVAL && says("coalac_encode: plan is NULL"));
  CHECK(coalac_decode(N, N, N, N, N, N, N, N, N) == COALAC_EINVAL && says("coalac_decode: plan is NULL"));
  CHECK(coalac_decode_ev(N, N, N, N, N, N, N, N, N, N) == COALAC_EINVAL && says("coalac_decode: plan is NULL"));
  CHECK(coalac_ef_accumulate(N, N, N, N, N, N) == COALAC_EINVAL && says("coalac_ef_accumulate: plan is NULL"));
  CHECK(coalac_ef_commit(N, N, N, N, N, N, N, N) == COALAC_EINVAL && says("coalac_ef_commit: plan is NULL"));
  CHECK(coalac_aggregate(N, 1, N, N, N, N, N, N, 1.0f, COALAC_AGG_DIV, N, N, N, N) == COALAC_EINVAL &&
        says("coalac_aggregate: plan is NULL"));
  CHECK(coalac_aggregate_ev(N, 1, N, N, N, N, N, N, 1.0f, COALAC_AGG_DIV, N, N, N, N, N) == COALAC_EINVAL &&
        says("coalac_aggregate: plan is NULL"));
  int out = 0;
  uint32_t lo = 0, hi = 0;
  uint64_t stamp = 0;
  CHECK(coalac_workspace_fallbacks(N, N, N, &out) == COALAC_EINVAL && says("coalac_workspace_fallbacks"));
  CHECK(coalac_debug_brackets(N, N, N, &lo, &hi, 1) == COALAC_EINVAL && says("coalac_debug_brackets"));
  CHECK(coalac_debug_stamps(N, N, N, &stamp, 1) == COALAC_EINVAL && says("coalac_debug_stamps"));
  CHECK(coalac_gather(N, -1, 4, N, N) == COALAC_EINVAL && says("bad arguments"));
  CHECK(coalac_gather(N, 1, 4, &out, N) == COALAC_EINVAL && says("bad arguments"));
  const void* src = &out;
  CHECK(coalac_gather(&src, 1, 3, &out, N) == COALAC_EINVAL && says("element size 3"));
  CHECK(coalac_gather(&src, 1, 8, reinterpret_cast<uint8_t*>(&stamp) + 4, N) == COALAC_EINVAL && says("not aligned"));
  CHECK(coalac_gather(N, 0, 4, N, N) == COALAC_OK);
  CHECK(coalac_version() == COALAC_ABI_VERSION);
}

// coalac_pack_dense, coalac_unpack_dense and coalac_decode_packed: every COALAC_EINVAL case, each ahead of the empty
// plan's COALAC_OK and of the first device call, on plans in host memory
static void dense_stream() {
  HostPlans p;
  alignas(16) static float x[64];
  alignas(16) static uint32_t out[64];
  const auto N = nullptr;
  float* r = reinterpret_cast<float*>(out);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(out);
  for (int empty = 0; empty < 2; ++empty) {  // (the second time on a plan without units: the same answers)
    if (empty) p.empty_dense();
    // coalac_pack_dense(plan, vals, packed, packed_bytes, stream) / coalac_unpack_dense(plan, packed, packed_bytes, vals, stream)
    CHECK(coalac_pack_dense(N, x, out, 32, N) == COALAC_EINVAL && says("coalac_pack_dense: plan is NULL"));
    CHECK(coalac_pack_dense(&p.dense, N, out, 32, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_pack_dense(&p.dense, x, N, 32, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_pack_dense(&p.sparse, x, out, 32, N) == COALAC_EINVAL && says("dense plan") && says("coalac_pack's"));
    CHECK(coalac_pack_dense(&p.raw, x, out, 32, N) == COALAC_EINVAL && says("bits == 32"));
    CHECK(coalac_pack_dense(&p.dense, x, out, 28, N) == COALAC_EINVAL && says("packed_bytes"));
    CHECK(coalac_pack_dense(&p.dense, bytes + 2, x, 32, N) == COALAC_EINVAL && says("4-byte"));
    CHECK(coalac_pack_dense(&p.dense, x, bytes + 1, 32, N) == COALAC_EINVAL && says("4-byte"));
    CHECK(coalac_unpack_dense(N, out, 32, x, N) == COALAC_EINVAL && says("coalac_unpack_dense: plan is NULL"));
    CHECK(coalac_unpack_dense(&p.dense, N, 32, x, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_unpack_dense(&p.dense, out, 32, N, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_unpack_dense(&p.sparse, out, 32, x, N) == COALAC_EINVAL && says("dense plan"));
    CHECK(coalac_unpack_dense(&p.raw, out, 32, x, N) == COALAC_EINVAL && says("bits == 32"));
    CHECK(coalac_unpack_dense(&p.dense, out, 28, x, N) == COALAC_EINVAL && says("packed_bytes"));
    CHECK(coalac_unpack_dense(&p.dense, bytes + 2, 32, x, N) == COALAC_EINVAL && says("4-byte"));
    CHECK(coalac_unpack_dense(&p.dense, out, 32, bytes + 3, N) == COALAC_EINVAL && says("4-byte"));
    // coalac_decode_packed(plan, packed, packed_bytes, mn, scale, base, out, stream)
    CHECK(coalac_decode_packed(N, out, 32, r, r, N, x, N) == COALAC_EINVAL && says("coalac_decode_packed: plan is NULL"));
    CHECK(coalac_decode_packed(&p.dense, N, 32, r, r, N, x, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_decode_packed(&p.dense, out, 32, N, r, N, x, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_decode_packed(&p.dense, out, 32, r, N, N, x, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_decode_packed(&p.dense, out, 32, r, r, N, N, N) == COALAC_EINVAL && says("NULL"));
    CHECK(coalac_decode_packed(&p.sparse, out, 32, r, r, N, x, N) == COALAC_EINVAL && says("dense plan"));
    CHECK(coalac_decode_packed(&p.raw, out, 32, r, r, N, x, N) == COALAC_EINVAL && says("bits == 32"));
    CHECK(coalac_decode_packed(&p.dense, out, 28, r, r, N, x, N) == COALAC_EINVAL && says("packed_bytes"));
    CHECK(coalac_decode_packed(&p.dense, bytes + 2, 32, r, r, N, x, N) == COALAC_EINVAL && says("4-byte"));
    CHECK(coalac_decode_packed(&p.dense, out, 32, r, r, N, x + 1, N) == COALAC_EINVAL && says("16-byte"));
    CHECK(coalac_decode_packed(&p.dense, out, 32, r, r, x + 2, x, N) == COALAC_EINVAL && says("16-byte"));
  }
  // the plan without units, otherwise: OK with nothing launched (a launch on this host-memory plan would fail)
  CHECK(coalac_pack_dense(&p.dense, x, out, 32, N) == COALAC_OK);
  CHECK(coalac_unpack_dense(&p.dense, out, 32, x, N) == COALAC_OK);
  CHECK(coalac_decode_packed(&p.dense, out, 32, r, r, N, x, N) == COALAC_OK);
  CHECK(coalac_decode_packed(&p.dense, out, 32, r, r, x, x, N) == COALAC_OK);
  for (int i = 0; i < 64; ++i) CHECK(x[i] == 0.0f && out[i] == 0u);  // nothing was written
}

static size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

template <typename T>
static void fill(T* p, size_t count, const uint8_t* lo, const uint8_t* hi) {
  CHECK(reinterpret_cast<uintptr_t>(p) % 256 == 0);
  CHECK(reinterpret_cast<uint8_t*>(p) >= lo && reinterpret_cast<uint8_t*>(p + count) <= hi);
  memset(p, 0x5A, sizeof(T) * count);  // past the allocation: an AddressSanitizer report
}

// the workspace walk for (segments, large units, groups, large segments, record slots): the size it measures is the sum
// of the arrays' padded sizes as Params documents them, and carved from a buffer of that size every array fits
static void workspace_walk() {
  const size_t shapes[][5] = {{1, 0, 0, 0, 512},        {7, 19, 3, 2, 512},      {7, 19, 3, 2, 2752},
                              {14, 38, 6, 4, 4096},     {2, 8201, 258, 1, 576},  {0, 0, 0, 0, 4096}};
  for (const auto& s : shapes) {
    const size_t S = s[0], LU = s[1], NG = s[2], NL = s[3], CC = s[4];
    Params P{};
    P.nseg = (uint32_t)S, P.n_lunits = (uint32_t)LU, P.n_groups = (uint32_t)NG, P.n_large = (uint32_t)NL;
    P.ccap = (uint32_t)CC;
    const size_t bytes = carve_workspace(P, false, nullptr);
    CHECK(P.status == nullptr && P.shhi == nullptr && P.stamps == nullptr);
    const size_t want = 3 * pad256(4 * S) + 10 * pad256(4 * LU) + pad256(16 * LU) + pad256(4 * CC * LU) +
                        pad256(2 * CC * LU) + pad256(8 * NSTAMP * std::max<size_t>(S, 1)) + pad256(4 * HB2 * NG) +
                        pad256(4 * NG) + pad256(8 * GCAP * NG) + pad256(8 * NG) + pad256(16 * NL) + pad256(4 * NL);
    CHECK(bytes == std::max<size_t>(want, 256));
    uint8_t* w = static_cast<uint8_t*>(aligned_alloc(256, bytes));
    CHECK(carve_workspace(P, false, w) == bytes);
    const uint8_t* e = w + bytes;
    CHECK(reinterpret_cast<uint8_t*>(P.status) == w && P.umm == nullptr);
    fill(P.status, S, w, e), fill(P.tstar, S, w, e), fill(P.rtie, S, w, e);
    fill(P.tlo, LU, w, e), fill(P.thi, LU, w, e), fill(P.cntA, LU, w, e), fill(P.cntC, LU, w, e);
    fill(P.cntZ, LU, w, e), fill(P.tsgn, LU, w, e), fill(P.gtC, LU, w, e), fill(P.eqC, LU, w, e);
    fill(P.eqpre, LU, w, e), fill(P.outoff, LU, w, e), fill(P.uemit, LU, w, e);
    fill(P.cval, CC * LU, w, e), fill(P.cpos, CC * LU, w, e);
    fill(P.stamps, NSTAMP * std::max<size_t>(S, 1), w, e);
    fill(P.ghist, HB2 * NG, w, e), fill(P.gcnt, NG, w, e), fill(P.glist, GCAP * NG, w, e), fill(P.gmm, 2 * NG, w, e);
    fill(P.sstate, NL, w, e), fill(P.shhi, NL, w, e);
    // in today's order: each array starts where the one before it ends, padded
    CHECK(reinterpret_cast<uint8_t*>(P.tstar) == w + pad256(4 * S));
    CHECK(reinterpret_cast<uint8_t*>(P.tlo) == w + 3 * pad256(4 * S));
    CHECK(reinterpret_cast<uint8_t*>(P.cval) == reinterpret_cast<uint8_t*>(P.uemit) + pad256(16 * LU));
    CHECK(reinterpret_cast<uint8_t*>(P.shhi) + pad256(4 * NL) == e || bytes == 256);
    free(w);
  }
  for (size_t U : {(size_t)0, (size_t)3, (size_t)8201}) {  // a dense plan: the per-unit min / max only
    Params P{};
    P.n_units = (uint32_t)U;
    const size_t bytes = carve_workspace(P, true, nullptr);
    CHECK(bytes == std::max<size_t>(pad256(8 * U), 256));
    uint8_t* w = static_cast<uint8_t*>(aligned_alloc(256, bytes));
    carve_workspace(P, true, w);
    CHECK(P.status == nullptr && P.stamps == nullptr);
    fill(P.umm, 2 * U, w, w + bytes);
    free(w);
  }
}

// the plan-table walk: the measured size, the packing into a staging buffer of exactly that size, and the device
// pointers (a made-up device base) at the same offsets
static void table_walk() {
  PlanTables T;
  T.segs.resize(5), T.units.resize(23), T.lunits.resize(19), T.small_list = {0, 3, 4}, T.large_list = {1, 2};
  T.lsegs.resize(2), T.ssegs.resize(3), T.groups.resize(2), T.gseg.resize(2);
  for (size_t i = 0; i < T.units.size(); ++i) T.units[i].start = (uint32_t)(100 + i);
  T.gseg[1] = make_uint4(1, 2, 3, 4);
  Params P{};
  const size_t bytes = place_tables(T, P, nullptr, nullptr);
  CHECK(P.segs == nullptr && P.gseg == nullptr);
  const size_t want = pad256(32 * 5) + pad256(32 * 23) + pad256(32 * 19) + pad256(4 * 3) + pad256(4 * 2) +
                      pad256(32 * 2) + pad256(32 * 3) + pad256(16 * 2) + pad256(16 * 2) + 256;
  CHECK(bytes == want);
  std::vector<uint8_t> host(bytes, 0);
  const uint8_t* dev = reinterpret_cast<const uint8_t*>(uintptr_t(1) << 40);
  CHECK(place_tables(T, P, host.data(), dev) == bytes);
  CHECK(reinterpret_cast<const uint8_t*>(P.segs) == dev);
  CHECK(reinterpret_cast<const uint8_t*>(P.units) == dev + pad256(32 * 5));
  CHECK(reinterpret_cast<const uint8_t*>(P.gseg) + pad256(16 * 2) + 256 == dev + bytes);
  const size_t o_units = reinterpret_cast<const uint8_t*>(P.units) - dev;
  CHECK(reinterpret_cast<const UnitDev*>(host.data() + o_units)[22].start == 122);
  const size_t o_small = reinterpret_cast<const uint8_t*>(P.small_list) - dev;
  CHECK(reinterpret_cast<const uint32_t*>(host.data() + o_small)[2] == 4);
  const size_t o_gseg = reinterpret_cast<const uint8_t*>(P.gseg) - dev;
  CHECK(reinterpret_cast<const uint4*>(host.data() + o_gseg)[1].w == 4);
  PlanTables E;  // an empty table: the pad alone
  CHECK(place_tables(E, P, nullptr, nullptr) == 256);
}

int main() {
  plan_validation();
  null_arguments();
  dense_stream();
  workspace_walk();
  table_walk();
  return report("host checks");
}
