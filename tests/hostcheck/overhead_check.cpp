// Test-only host program (tests/test_gpu_solve_overhead.py): the slots of the branch-free transpose
// of L through the team scratch (bb_team16.h: ltr_slot, chol_solve_rows) against the packed
// triangle the predicated stores filled, on random rows.  Prints "ok" and returns 0, or says what
// differs.  Never shipped.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "bb_team16.h"

using namespace bb;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {  // xorshift64*, uniform in [-1, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return double((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / double(1ull << 52) - 1.0;
}
static bool same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// the sixteen lanes' stores column by column (one store instruction per column, all lanes), then
// lane tl's reads of column tl
static int check_transpose(int trials) {
  for (int t = 0; t < trials; t++) {
    double h[16][NV], scr[LTR_SLOTS + 8], old[LTR_SPARE];
    const double canary = 12345.678 + t;
    for (int i = 0; i < LTR_SLOTS + 8; i++) scr[i] = canary;
    for (int tl = 0; tl < 16; tl++)
      for (int k = 0; k < NV; k++) h[tl][k] = (t % 3 == 0 && k >= tl) ? NAN : rnd();  // upper part: anything
    for (int tl = 0; tl < NV; tl++)  // the predicated form
      for (int k = 0; k < NV - 1; k++)
        if (k < tl) old[tl * (tl - 1) / 2 + k] = h[tl][k];
    for (int k = 0; k < NV - 1; k++)
      for (int tl = 0; tl < 16; tl++) {
        const int s = ltr_slot(tl, k);
        if (s < 0 || s >= LTR_SLOTS) return printf("slot %d out of range: lane %d column %d\n", s, tl, k), 1;
        const bool valid = tl < NV && k < tl;
        if (valid && s != tl * (tl - 1) / 2 + k)
          return printf("lane %d column %d: slot %d, packed %d\n", tl, k, s, tl * (tl - 1) / 2 + k), 1;
        if (!valid && s != LTR_SPARE) return printf("lane %d column %d: slot %d is not the spare\n", tl, k, s), 1;
        scr[s] = h[tl][k];
      }
    for (int i = LTR_SLOTS; i < LTR_SLOTS + 8; i++)
      if (!same(scr[i], canary)) return printf("slot %d behind the scratch written\n", i), 1;
    for (int i = 0; i < LTR_SPARE; i++)
      if (!same(scr[i], old[i])) return printf("trial %d: packed slot %d differs from the predicated stores'\n", t, i), 1;
    for (int tl = 0; tl < 16; tl++)
      for (int i = 0; i < NV; i++) {
        const double got = i > tl ? scr[i * (i - 1) / 2 + tl] : 0.0;  // chol_solve_rows' read
        const double want = i > tl ? h[i][tl] : 0.0;
        if (!same(got, want)) return printf("trial %d: L[%d][%d] read back as %g, is %g\n", t, i, tl, got, want), 1;
      }
  }
  return 0;
}

// the gradient's wheel term as a selected operand (x - 0 for a row without a column) against the
// skipped subtraction, signed zeros included
static int check_selected_zero() {
  const double xs[] = {0.0, -0.0, 1.5, -2.25, 1e-310, -1e308};
  for (double x : xs) {
    const double t = rnd();
    for (int has = 0; has < 2; has++) {
      double o = x, n = x;
      if (has) o -= t;
      n -= has ? t : 0.0;
      if (!same(o, n)) return printf("x = %a: selected %a, skipped %a\n", x, n, o), 1;
    }
  }
  return 0;
}

int main() {
  if (check_transpose(300) || check_selected_zero()) return 1;
  printf("ok\n");
  return 0;
}
