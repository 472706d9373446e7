// Host-side checks of the stochastic-rounding contract that need no device
// (tests/test_sr_host.py builds and runs it, with the host sanitizers): the __host__ side of sr_u24 / sr_code — the
// very functions the kernels call — over a table the Python test wrote from tests/sr_model.py, and the argument
// checks of coalac_encode_sr / coalac_encode_block_sr that return before any device call, on plans built in host
// memory. The codec source is included, not linked: struct coalac_plan lives in it.
//
// The table (argv[1]), one row per line, every number in hex:
//   u <seed> <c> <u24>                    sr_u24(seed, c) == u24
//   c <t bits> <u24> <levels> <code>      sr_code(t, u24, levels) == code
#include "../coala_amd/csrc/coalac.hip"

#include <cinttypes>

#include "host_check_common.h"

static void model_table(const char* path) {
  FILE* f = fopen(path, "r");
  CHECK(f != nullptr);
  if (!f) return;
  char kind;
  long rows_u = 0, rows_c = 0, bad = 0;
  while (fscanf(f, " %c", &kind) == 1) {
    if (kind == 'u') {
      uint64_t seed, c;
      uint32_t want;
      if (fscanf(f, "%" SCNx64 " %" SCNx64 " %" SCNx32, &seed, &c, &want) != 3) break;
      const uint32_t got = sr_u24(seed, c);
      if (got != want && bad++ < 5) printf("sr_u24(%" PRIx64 ", %" PRIx64 ") = %x, the model says %x\n", seed, c, got, want);
      ++rows_u;
    } else if (kind == 'c') {
      uint32_t tb, u24, levels, want;
      if (fscanf(f, "%" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32, &tb, &u24, &levels, &want) != 4) break;
      float t;
      memcpy(&t, &tb, 4);
      const uint32_t got = sr_code(t, u24, (float)levels);
      if (got != want && bad++ < 5) printf("sr_code(%a, %x, %u) = %u, the model says %u\n", t, u24, levels, got, want);
      ++rows_c;
    } else {
      break;
    }
  }
  fclose(f);
  CHECK(bad == 0);
  CHECK(rows_u >= 100 && rows_c >= 100);
  printf("model table: %ld draws, %ld codes\n", rows_u, rows_c);
}

// the issue's known-answer values, stated here once more
static void known_answers() {
  const uint32_t a[4] = {0x944fb5, 0xb2fcf0, 0xfdd0ca, 0x1ece84};
  for (uint64_t c = 0; c < 4; ++c) CHECK(sr_u24(0, c) == a[c]);
  const uint64_t s = 0xDEADBEEFCAFEF00Dull, cs[4] = {0, 1, 1ull << 32, (1ull << 32) + 1};
  const uint32_t b[4] = {0xb741a7, 0x05c4ca, 0x0f049b, 0xac3d96};
  for (int i = 0; i < 4; ++i) CHECK(sr_u24(s, cs[i]) == b[i]);
  CHECK(sr_code(3.0f, 0, 15.0f) == 3 && sr_code(3.0f, 0xFFFFFF, 15.0f) == 3);  // an integer t is kept
  CHECK(sr_code(3.5f, 0x7FFFFF, 15.0f) == 4 && sr_code(3.5f, 0x800000, 15.0f) == 3);
  CHECK(sr_code(15.0f, 0, 15.0f) == 15 && sr_code(1e30f, 0, 15.0f) == 15 && sr_code(INFINITY, 0, 15.0f) == 15);
  CHECK(sr_code(0.0f, 0, 15.0f) == 0 && sr_code(-1.0f, 0, 15.0f) == 0 && sr_code(NAN, 0, 15.0f) == 0);
  CHECK(sr_code(0x1p-30f, 0, 15.0f) == 1 && sr_code(0x1p-30f, 1, 15.0f) == 0);
}

static void argument_checks() {
  HostPlans p;
  coalac_plan &dense = p.dense, &sparse = p.sparse, &raw = p.raw;
  alignas(16) static float x[64];
  alignas(16) static uint32_t out[64];
  const float* seg = x;
  const auto N = nullptr;
  float* r = reinterpret_cast<float*>(out);
  void* ws = out;
  // coalac_encode_sr(plan, in, seg_in, base, vals, mn, scale, ws, ws_bytes, seed, flags, stream)
  CHECK(coalac_encode_sr(N, x, N, N, out, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("coalac_encode_sr: plan is NULL"));
  CHECK(coalac_encode_sr(&sparse, x, N, N, out, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("dense plan"));
  CHECK(coalac_encode_sr(&raw, x, N, N, out, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("bits == 32"));
  CHECK(coalac_encode_sr(&dense, x, &seg, N, out, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_sr(&dense, N, N, N, out, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_sr(&dense, x, N, N, out, N, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("mn/scale"));
  CHECK(coalac_encode_sr(&dense, x, N, N, out, r, N, ws, 256, 1, 0, N) == COALAC_EINVAL && says("mn/scale"));
  CHECK(coalac_encode_sr(&dense, x, N, N, N, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("vals"));
  CHECK(coalac_encode_sr(&dense, x + 1, N, N, out, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_sr(&dense, x, N, x + 2, out, r, r, ws, 256, 1, 0, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_sr(&dense, x, N, N, out, r, r, N, 256, 1, 0, N) == COALAC_EWORKSPACE && says("workspace"));
  CHECK(coalac_encode_sr(&dense, x, N, N, out, r, r, ws, 255, 1, 0, N) == COALAC_EWORKSPACE && says("workspace"));
  // coalac_encode_block_sr(plan, in, seg_in, base, bmn, bscale, packed, packed_bytes, seed, stream)
  CHECK(coalac_encode_block_sr(N, x, N, N, r, r, out, 32, 1, N) == COALAC_EINVAL && says("coalac_encode_block_sr: plan is NULL"));
  CHECK(coalac_encode_block_sr(&sparse, x, N, N, r, r, out, 32, 1, N) == COALAC_EINVAL && says("dense plan"));
  CHECK(coalac_encode_block_sr(&raw, x, N, N, r, r, out, 32, 1, N) == COALAC_EINVAL && says("bits == 32"));
  CHECK(coalac_encode_block_sr(&dense, x, &seg, N, r, r, out, 32, 1, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_block_sr(&dense, N, N, N, r, r, out, 32, 1, N) == COALAC_EINVAL && says("exactly one"));
  CHECK(coalac_encode_block_sr(&dense, x, N, N, N, r, out, 32, 1, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_sr(&dense, x, N, N, r, N, out, 32, 1, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_sr(&dense, x, N, N, r, r, N, 32, 1, N) == COALAC_EINVAL && says("NULL"));
  CHECK(coalac_encode_block_sr(&dense, x, N, N, r, r, out, 28, 1, N) == COALAC_EINVAL && says("packed_bytes"));
  CHECK(coalac_encode_block_sr(&dense, x + 1, N, N, r, r, out, 32, 1, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_block_sr(&dense, x, N, N, r, r, reinterpret_cast<uint8_t*>(out) + 2, 32, 1, N) == COALAC_EINVAL &&
        says("4-byte"));
  // a plan without segments / units: the block-wise checks are the same, else OK, nothing launched
  p.empty_dense();
  CHECK(coalac_encode_block_sr(&dense, x + 1, N, N, r, r, out, 32, 1, N) == COALAC_EINVAL && says("16-byte"));
  CHECK(coalac_encode_sr(&dense, x, N, N, out, r, r, ws, 256, 1, 0, N) == COALAC_OK);
  CHECK(coalac_encode_block_sr(&dense, x, N, N, r, r, out, 32, 1, N) == COALAC_OK);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: sr_host_checks TABLE\n");
    return 2;
  }
  model_table(argv[1]);
  known_answers();
  argument_checks();
  return report("sr host checks");
}
