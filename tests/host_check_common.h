// What the stand-alone host-check programs (tests/*_host_checks.hip, tests/host_checks.hip) share; each includes it
// after coalac.hip, whose struct coalac_plan and coalac_last_error it uses.
#pragma once

static int g_failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAILED %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, coalac_last_error()); \
      ++g_failures;                                                     \
    }                                                                   \
  } while (0)

static bool says(const char* part) { return strstr(coalac_last_error(), part) != nullptr; }

// Plans in host memory (every check under test returns before the first device call): a dense 4-bit plan of one
// 64-element segment — one unit, one block of either size, 8 stream words — a sparse one and one with bits == 32
struct HostPlans {
  coalac_plan dense, sparse, raw;
  HostPlans() {
    for (coalac_plan* p : {&dense, &sparse, &raw}) {
      p->dense = true, p->bits = 4, p->proto.nseg = 1, p->proto.n_units = 1, p->total_k = 64, p->span = 64;
      p->ws_bytes = 256, p->dense_words = 8;
      p->n_blocks[0] = 1, p->n_blocks[1] = 1;
    }
    sparse.dense = false;
    raw.bits = 32;
  }
  void empty_dense() { dense.proto.nseg = 0, dense.proto.n_units = 0; }  // a plan without segments / units
};

// the program's last line and exit status
static int report(const char* name) {
  if (g_failures)
    printf("%s: %d FAILED\n", name, g_failures);
  else
    printf("%s: ok\n", name);
  return g_failures ? 1 : 0;
}
