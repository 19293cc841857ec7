// What the host programs of the satellite libraries (zs_*_host_math.hip in this directory) share: the check counters, the
// long-double type of the restatements, one seeded generator (every program draws from the same stream, in its own order) and
// the closing lines of main.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

static long n_checks = 0;
static int n_fail = 0;
static void expect(bool ok, const char* what, double got, double want) {
  ++n_checks;
  if (!ok) {
    if (n_fail < 20) fprintf(stderr, "FAIL %s: got %.17g want %.17g\n", what, got, want);
    ++n_fail;
  }
}
typedef long double ld;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform01() {          // xorshift64*: strictly inside (0, 1)
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return ((double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) + 0.5) * ldexp(1.0, -53);
}
static double normal01() { return sqrt(-2.0 * log(uniform01())) * cos(6.283185307179586 * uniform01()); }

// the last statement of main: `return finish("nf host math ok");` prints "nf host math ok: N checks", or the failures' count
static int finish(const char* ok) {
  if (n_fail) {
    fprintf(stderr, "%d of %ld checks failed\n", n_fail, n_checks);
    return 1;
  }
  printf("%s: %ld checks\n", ok, n_checks);
  return 0;
}
