// Host-side checks of the rotated block-wise entry points that need no device (tests/test_rot_host.py
// builds and runs it, with the host sanitizers): every COALAC_EINVAL case of coalac_encode_block_rot,
// coalac_encode_block_rot_sr and coalac_decode_block_rot, each of which returns before the first device call, on plans
// built in host memory; each once more on a plan without units, and that plan's COALAC_OK with nothing launched.
// The codec source is included, not linked: struct coalac_plan lives in it.
#include "../coala_amd/csrc/coalac.hip"

#include "host_check_common.h"

alignas(16) static float x[64];
alignas(16) static uint32_t out[64];

static const uint64_t ROT = 0x0123456789ABCDEFull, SR = 0xFEDCBA9876543210ull;

// coalac_encode_block_rot (sr false) or coalac_encode_block_rot_sr behind coalac_encode_block's arguments
static int enc(bool sr, coalac_plan_t plan, const float* in, const float* const* seg_in, const float* base, float* bmn,
               float* bscale, void* packed, uint64_t packed_bytes) {
  return sr ? coalac_encode_block_rot_sr(plan, in, seg_in, base, bmn, bscale, packed, packed_bytes, ROT, SR, nullptr)
            : coalac_encode_block_rot(plan, in, seg_in, base, bmn, bscale, packed, packed_bytes, ROT, nullptr);
}

static int dec(coalac_plan_t plan, const void* packed, uint64_t packed_bytes, const float* bmn, const float* bscale,
               const float* base, float* o) {
  return coalac_decode_block_rot(plan, packed, packed_bytes, bmn, bscale, ROT, base, o, nullptr);
}

static void encode(bool sr) {
  HostPlans hp;
  coalac_plan &dense = hp.dense, &sparse = hp.sparse, &raw = hp.raw;
  const float* seg = x;
  const auto N = nullptr;
  float* r = reinterpret_cast<float*>(out);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(out);
  CHECK(enc(sr, N, x, N, N, r, r, out, 32) == COALAC_EINVAL && says("plan is NULL"));
  CHECK(says(sr ? "coalac_encode_block_rot_sr" : "coalac_encode_block_rot:"));  // (the message names the entry point)
  CHECK(enc(sr, &dense, x, &seg, N, r, r, out, 32) == COALAC_EINVAL && says("exactly one"));
  CHECK(enc(sr, &dense, N, N, N, r, r, out, 32) == COALAC_EINVAL && says("exactly one"));
  CHECK(enc(sr, &sparse, x, N, N, r, r, out, 32) == COALAC_EINVAL && says("dense plan"));
  CHECK(enc(sr, &raw, x, N, N, r, r, out, 32) == COALAC_EINVAL && says("bits == 32"));
  CHECK(enc(sr, &dense, x, N, N, N, r, out, 32) == COALAC_EINVAL && says("NULL"));
  CHECK(enc(sr, &dense, x, N, N, r, N, out, 32) == COALAC_EINVAL && says("NULL"));
  CHECK(enc(sr, &dense, x, N, N, r, r, N, 32) == COALAC_EINVAL && says("NULL"));
  CHECK(enc(sr, &dense, x, N, N, r, r, out, 28) == COALAC_EINVAL && says("packed_bytes"));
  CHECK(enc(sr, &dense, x + 1, N, N, r, r, out, 32) == COALAC_EINVAL && says("16-byte"));
  CHECK(enc(sr, &dense, x, N, x + 2, r, r, out, 32) == COALAC_EINVAL && says("16-byte"));
  CHECK(enc(sr, &dense, x, N, N, reinterpret_cast<float*>(bytes + 2), r, out, 32) == COALAC_EINVAL && says("4-byte"));
  CHECK(enc(sr, &dense, x, N, N, r, reinterpret_cast<float*>(bytes + 1), out, 32) == COALAC_EINVAL && says("4-byte"));
  CHECK(enc(sr, &dense, x, N, N, r, r, bytes + 2, 32) == COALAC_EINVAL && says("4-byte"));
  // a plan without units: the same checks, else OK with nothing launched (a launch on this host-memory plan would fail)
  hp.empty_dense();
  CHECK(enc(sr, &dense, x, &seg, N, r, r, out, 32) == COALAC_EINVAL && says("exactly one"));
  CHECK(enc(sr, &dense, N, N, N, r, r, out, 32) == COALAC_EINVAL && says("exactly one"));
  CHECK(enc(sr, &dense, x, N, N, N, r, out, 32) == COALAC_EINVAL && says("NULL"));
  CHECK(enc(sr, &dense, x, N, N, r, N, out, 32) == COALAC_EINVAL && says("NULL"));
  CHECK(enc(sr, &dense, x, N, N, r, r, N, 32) == COALAC_EINVAL && says("NULL"));
  CHECK(enc(sr, &dense, x, N, N, r, r, out, 28) == COALAC_EINVAL && says("packed_bytes"));
  CHECK(enc(sr, &dense, x + 1, N, N, r, r, out, 32) == COALAC_EINVAL && says("16-byte"));
  CHECK(enc(sr, &dense, x, N, x + 2, r, r, out, 32) == COALAC_EINVAL && says("16-byte"));
  CHECK(enc(sr, &dense, x, N, N, reinterpret_cast<float*>(bytes + 2), r, out, 32) == COALAC_EINVAL && says("4-byte"));
  CHECK(enc(sr, &dense, x, N, N, r, reinterpret_cast<float*>(bytes + 1), out, 32) == COALAC_EINVAL && says("4-byte"));
  CHECK(enc(sr, &dense, x, N, N, r, r, bytes + 2, 32) == COALAC_EINVAL && says("4-byte"));
  hp.sparse.proto.nseg = hp.sparse.proto.n_units = 0, hp.raw.proto.nseg = hp.raw.proto.n_units = 0;
  CHECK(enc(sr, &sparse, x, N, N, r, r, out, 32) == COALAC_EINVAL && says("dense plan"));
  CHECK(enc(sr, &raw, x, N, N, r, r, out, 32) == COALAC_EINVAL && says("bits == 32"));
  CHECK(enc(sr, &dense, x, N, N, r, r, out, 32) == COALAC_OK);
  CHECK(enc(sr, &dense, N, &seg, x, r, r, out, 32) == COALAC_OK);
  for (int i = 0; i < 64; ++i) CHECK(x[i] == 0.0f && out[i] == 0u);  // nothing was written
}

static void decode() {
  HostPlans hp;
  coalac_plan &dense = hp.dense, &sparse = hp.sparse, &raw = hp.raw;
  const auto N = nullptr;
  float* r = reinterpret_cast<float*>(out);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(out);
  for (int pass = 0; pass < 2; ++pass) {  // (the second pass: every plan without units)
    CHECK(dec(N, out, 32, r, r, N, x) == COALAC_EINVAL && says("plan is NULL") && says("coalac_decode_block_rot"));
    CHECK(dec(&sparse, out, 32, r, r, N, x) == COALAC_EINVAL && says("dense plan"));
    CHECK(dec(&raw, out, 32, r, r, N, x) == COALAC_EINVAL && says("bits == 32"));
    CHECK(dec(&dense, N, 32, r, r, N, x) == COALAC_EINVAL && says("NULL"));
    CHECK(dec(&dense, out, 32, N, r, N, x) == COALAC_EINVAL && says("NULL"));
    CHECK(dec(&dense, out, 32, r, N, N, x) == COALAC_EINVAL && says("NULL"));
    CHECK(dec(&dense, out, 32, r, r, N, N) == COALAC_EINVAL && says("NULL"));
    CHECK(dec(&dense, out, 28, r, r, N, x) == COALAC_EINVAL && says("packed_bytes"));
    CHECK(dec(&dense, bytes + 2, 32, r, r, N, x) == COALAC_EINVAL && says("4-byte"));
    CHECK(dec(&dense, out, 32, reinterpret_cast<float*>(bytes + 1), r, N, x) == COALAC_EINVAL && says("4-byte"));
    CHECK(dec(&dense, out, 32, r, reinterpret_cast<float*>(bytes + 2), N, x) == COALAC_EINVAL && says("4-byte"));
    CHECK(dec(&dense, out, 32, r, r, N, x + 1) == COALAC_EINVAL && says("16-byte"));
    CHECK(dec(&dense, out, 32, r, r, x + 2, x) == COALAC_EINVAL && says("16-byte"));
    hp.empty_dense();
    hp.sparse.proto.nseg = hp.sparse.proto.n_units = 0, hp.raw.proto.nseg = hp.raw.proto.n_units = 0;
  }
  CHECK(dec(&dense, out, 32, r, r, N, x) == COALAC_OK);
  CHECK(dec(&dense, out, 32, r, r, x, x) == COALAC_OK);
  for (int i = 0; i < 64; ++i) CHECK(x[i] == 0.0f && out[i] == 0u);  // nothing was written
}

int main() {
  encode(false);
  encode(true);
  decode();
  return report("rot host checks");
}
