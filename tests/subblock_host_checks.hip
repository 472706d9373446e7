// Host-side checks of the block-size entry points that need no device (tests/test_subblock_host.py
// builds and runs it, with the host sanitizers): every COALAC_EINVAL case of coalac_encode_block_g,
// coalac_decode_block_g, coalac_aggregate_dense_g and coalac_plan_block_count — and, through block = 4096, of
// coalac_encode_block, coalac_decode_block and coalac_aggregate_dense — each of which returns before the first device
// call, on plans built in host memory; the plan without units; and the block counts against hand-computed ones.
// The codec source is included, not linked: struct coalac_plan lives in it.
#include "../coala_amd/csrc/coalac.hip"

#include "host_check_common.h"

alignas(16) static float x[64];
alignas(16) static uint32_t out[64];
alignas(16) static const void* ptrs[4];

static void block_counts() {
  HostPlans hp;
  coalac_plan &p = hp.dense, &sparse = hp.sparse, &raw = hp.raw;
  // the counts a plan over segments of 0, 1, 255, 256, 257 and 4097 elements holds: 22 blocks of 256 (0 + 1 + 1 + 1 + 2
  // + 17), 9 of 1024 (0 + 1 + 1 + 1 + 1 + 5), 6 units (0 + 1 + 1 + 1 + 1 + 2)
  const uint32_t sizes[6] = {0, 1, 255, 256, 257, 4097};
  uint64_t nb[2] = {0, 0}, units = 0;
  for (uint32_t n : sizes) {
    for (int i = 0; i < 2; ++i) nb[i] += ceil_div(n, SUB_BLOCKS[i]);
    units += ceil_div(n, UNIT);
  }
  CHECK(nb[0] == 22 && nb[1] == 9 && units == 6);
  p.n_blocks[0] = nb[0], p.n_blocks[1] = nb[1], p.proto.n_units = (uint32_t)units;
  uint64_t n = 99;
  CHECK(coalac_plan_block_count(&p, 256, &n) == COALAC_OK && n == 22);
  CHECK(coalac_plan_block_count(&p, 1024, &n) == COALAC_OK && n == 9);
  CHECK(coalac_plan_block_count(&p, 4096, &n) == COALAC_OK && n == 6);
  n = 99;
  for (uint32_t bad : {0u, 1u, 64u, 512u, 2048u, 8192u, 4095u, 0xFFFFFFFFu})
    CHECK(coalac_plan_block_count(&p, bad, &n) == COALAC_EINVAL && says("need 256, 1024 or 4096") && n == 99);
  CHECK(coalac_plan_block_count(nullptr, 256, &n) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_plan_block_count(&p, 256, nullptr) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_plan_block_count(&sparse, 256, &n) == COALAC_EINVAL && says("dense plan"));
  CHECK(coalac_plan_block_count(&raw, 1024, &n) == COALAC_EINVAL && says("dense plan"));
  CHECK(n == 99);
}

static void encode_and_decode(uint32_t G) {
  HostPlans hp;
  coalac_plan &dense = hp.dense, &sparse = hp.sparse, &raw = hp.raw;
  const float* seg = x;
  const auto N = nullptr;
  float* r = reinterpret_cast<float*>(out);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(out);
  // coalac_encode_block_g(plan, block, in, seg_in, base, bmn, bscale, packed, packed_bytes, stream)
  CHECK(coalac_encode_block_g(N, G, x, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("plan is NULL"));
  CHECK(coalac_encode_block_g(&dense, G, x, &seg, N, r, r, out, 32, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_block_g(&dense, G, N, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_block_g(&sparse, G, x, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("dense plan"));
  CHECK(coalac_encode_block_g(&raw, G, x, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("bits == 32"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, N, r, out, 32, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, r, N, out, 32, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, r, r, N, 32, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, r, r, out, 28, N) == COALAC_EINVAL && says("packed_bytes"));
  CHECK(coalac_encode_block_g(&dense, G, x + 1, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, x + 2, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, reinterpret_cast<float*>(bytes + 2), r, out, 32, N) == COALAC_EINVAL &&
        says("4-byte"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, r, reinterpret_cast<float*>(bytes + 1), out, 32, N) == COALAC_EINVAL &&
        says("4-byte"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, r, r, bytes + 2, 32, N) == COALAC_EINVAL && says("4-byte"));
  // coalac_decode_block_g(plan, block, packed, packed_bytes, bmn, bscale, base, out, stream)
  CHECK(coalac_decode_block_g(N, G, out, 32, r, r, N, x, N) == COALAC_EINVAL && says("plan is NULL"));
  CHECK(coalac_decode_block_g(&sparse, G, out, 32, r, r, N, x, N) == COALAC_EINVAL && says("dense plan"));
  CHECK(coalac_decode_block_g(&raw, G, out, 32, r, r, N, x, N) == COALAC_EINVAL && says("bits == 32"));
  CHECK(coalac_decode_block_g(&dense, G, N, 32, r, r, N, x, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, N, r, N, x, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, r, N, N, x, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, r, r, N, N, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_decode_block_g(&dense, G, out, 28, r, r, N, x, N) == COALAC_EINVAL && says("packed_bytes"));
  CHECK(coalac_decode_block_g(&dense, G, bytes + 2, 32, r, r, N, x, N) == COALAC_EINVAL && says("4-byte"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, reinterpret_cast<float*>(bytes + 1), r, N, x, N) == COALAC_EINVAL &&
        says("4-byte"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, r, r, N, x + 1, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, r, r, x + 2, x, N) == COALAC_EINVAL && says("16-byte"));
  // a plan without units: the same checks, else OK with nothing launched (a launch on this host-memory plan would fail)
  hp.empty_dense();
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, N, r, out, 32, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, r, r, N, N, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_g(&dense, G, x + 1, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, r, r, bytes + 2, 32, N) == COALAC_EINVAL && says("4-byte"));
  CHECK(coalac_decode_block_g(&dense, G, bytes + 2, 32, r, r, N, x, N) == COALAC_EINVAL && says("4-byte"));
  CHECK(coalac_decode_block_g(&dense, G, out, 32, r, r, N, x + 1, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_g(&dense, G, x, N, N, r, r, out, 32, N) == COALAC_OK);
  CHECK(coalac_encode_block_g(&dense, G, N, &seg, x, r, r, out, 32, N) == COALAC_OK);
  CHECK(coalac_decode_block_g(&dense, G, out, 32, r, r, N, x, N) == COALAC_OK);
  for (int i = 0; i < 64; ++i) CHECK(x[i] == 0.0f && out[i] == 0u);  // nothing was written
}

static void aggregate(uint32_t G) {
  HostPlans hp;
  coalac_plan &dense = hp.dense, &sparse = hp.sparse, &raw = hp.raw;
  const auto N = nullptr;
  const void* const* cp = ptrs;
  const float* const* fp = reinterpret_cast<const float* const*>(ptrs);
  const float* w = x;
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(ptrs);
  const int DIV = COALAC_AGG_DIV;
  // coalac_aggregate_dense_g(plan, clients, block, codes, code_bytes, mn, scale, weights, total, mode, mask, base, out, stream)
  CHECK(coalac_aggregate_dense_g(N, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("plan is NULL"));
  CHECK(coalac_aggregate_dense_g(&sparse, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("dense plan"));
  CHECK(coalac_aggregate_dense_g(&raw, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("bits == 32"));
  CHECK(coalac_aggregate_dense_g(&dense, 0, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("clients"));
  CHECK(coalac_aggregate_dense_g(&dense, -3, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("clients"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, w, 1.0f, 3, N, N, x, N) == COALAC_EINVAL && says("bad mode"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, w, 1.0f, -1, N, N, x, N) == COALAC_EINVAL && says("bad mode"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, N, 32, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, N, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, N, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, N, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, N, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 28, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_EINVAL && says("code_bytes"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, x + 1, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, x + 2, x, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, reinterpret_cast<const void* const*>(bytes + 4), 32, fp, fp, w, 1.0f, DIV, N, N,
                                 x, N) == COALAC_EINVAL && says("8-byte"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, reinterpret_cast<const float*>(bytes + 2), 1.0f, DIV, N, N, x,
                                 N) == COALAC_EINVAL && says("4-byte"));
  hp.empty_dense();
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, N, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_aggregate_dense_g(&dense, 1, G, cp, 32, fp, fp, w, 1.0f, DIV, N, N, x, N) == COALAC_OK);
  CHECK(coalac_aggregate_dense_g(&dense, 2, G, cp, 32, fp, fp, w, 1.0f, COALAC_AGG_SUM, N, x, x, N) == COALAC_OK);
  for (int i = 0; i < 64; ++i) CHECK(x[i] == 0.0f);  // nothing was written
}

static void bad_block_sizes() {
  HostPlans hp;
  coalac_plan& dense = hp.dense;
  hp.empty_dense();  // (every other argument is acceptable: only the size is wrong)
  const auto N = nullptr;
  float* r = reinterpret_cast<float*>(out);
  const void* const* cp = ptrs;
  const float* const* fp = reinterpret_cast<const float* const*>(ptrs);
  for (uint32_t bad : {0u, 1u, 64u, 512u, 2048u, 8192u, 0xFFFFFFFFu}) {
    CHECK(coalac_encode_block_g(&dense, bad, x, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("need 256, 1024 or 4096"));
    CHECK(coalac_decode_block_g(&dense, bad, out, 32, r, r, N, x, N) == COALAC_EINVAL && says("need 256, 1024 or 4096"));
    CHECK(coalac_aggregate_dense_g(&dense, 1, bad, cp, 32, fp, fp, x, 1.0f, COALAC_AGG_DIV, N, N, x, N) == COALAC_EINVAL &&
          says("need 256, 1024 or 4096"));
    CHECK(coalac_encode_block_g(N, bad, x, N, N, r, r, out, 32, N) == COALAC_EINVAL);  // (also with nothing else right)
  }
}

int main() {
  block_counts();
  // (4096 forwards to the twins — coalac_encode_block, coalac_decode_block, coalac_aggregate_dense — which, like the
  // entry points above, check everything before their first device call, so their cases run here too)
  for (uint32_t G : {256u, 1024u, 4096u}) encode_and_decode(G), aggregate(G);
  bad_block_sizes();
  return report("subblock host checks");
}
