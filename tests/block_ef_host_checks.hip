// Host-side checks of coalac_encode_block_ef that need no device (tests/test_block_ef_host.py builds
// and runs it, with the host sanitizers): every COALAC_EINVAL case of the entry point, each of which returns before
// the first device call, on plans built in host memory, and the plan without units. The codec source is included, not
// linked: struct coalac_plan lives in it.
#include "../coala_amd/csrc/coalac.hip"

#include "host_check_common.h"

static void argument_checks() {
  HostPlans p;
  coalac_plan &dense = p.dense, &sparse = p.sparse, &raw = p.raw;
  alignas(16) static float x[64];
  alignas(16) static float res[64];
  alignas(16) static uint32_t out[64];
  const float* seg = x;
  const auto N = nullptr;
  float* r = reinterpret_cast<float*>(out);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(out);
  // coalac_encode_block_ef(plan, in, seg_in, base, resid, bmn, bscale, packed, packed_bytes, stream)
  CHECK(coalac_encode_block_ef(N, x, N, N, res, r, r, out, 32, N) == COALAC_EINVAL && says("coalac_encode_block_ef: plan is NULL"));
  // what coalac_encode_block rejects
  CHECK(coalac_encode_block_ef(&dense, x, &seg, N, res, r, r, out, 32, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_block_ef(&dense, N, N, N, res, r, r, out, 32, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_block_ef(&sparse, x, N, N, res, r, r, out, 32, N) == COALAC_EINVAL && says("dense plan"));
  CHECK(coalac_encode_block_ef(&raw, x, N, N, res, r, r, out, 32, N) == COALAC_EINVAL && says("bits == 32"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, N, r, out, 32, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, r, N, out, 32, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, r, r, N, 32, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, r, r, out, 28, N) == COALAC_EINVAL && says("packed_bytes"));
  CHECK(coalac_encode_block_ef(&dense, x + 1, N, N, res, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_ef(&dense, x, N, x + 2, res, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, reinterpret_cast<float*>(bytes + 2), r, out, 32, N) == COALAC_EINVAL &&
        says("4-byte"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, r, reinterpret_cast<float*>(bytes + 1), out, 32, N) == COALAC_EINVAL &&
        says("4-byte"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, r, r, bytes + 2, 32, N) == COALAC_EINVAL && says("4-byte"));
  // the residual's own
  CHECK(coalac_encode_block_ef(&dense, x, N, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("residual pointer is NULL"));
  CHECK(coalac_encode_block_ef(&dense, N, &seg, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("residual pointer is NULL"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res + 1, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_ef(&dense, x, N, x, res + 2, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_ef(&dense, N, &seg, N, res + 3, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  // the checks are the same for a plan without units ...
  p.empty_dense();
  CHECK(coalac_encode_block_ef(&dense, x, N, N, N, r, r, out, 32, N) == COALAC_EINVAL && says("residual pointer is NULL"));
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res + 1, r, r, out, 32, N) == COALAC_EINVAL && says("16-byte"));
  // ... which otherwise is OK and launches nothing (a launch on this host-memory plan would fail)
  CHECK(coalac_encode_block_ef(&dense, x, N, N, res, r, r, out, 32, N) == COALAC_OK);
  CHECK(coalac_encode_block_ef(&dense, N, &seg, x, res, r, r, out, 32, N) == COALAC_OK);
  for (int i = 0; i < 64; ++i) CHECK(res[i] == 0.0f && out[i] == 0u);  // nothing was written
}

int main() {
  argument_checks();
  return report("block ef host checks");
}
