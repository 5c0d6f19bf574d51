// Test-only host program (tests/test_host_lds_batch.py): the batched three-row product of a wheel
// contact's Jacobian (bb_solve.h: wheel_dot3, wheel_jar3) against three wheel_dot calls, bit for
// bit, on random J and x, all three wheels (the hinge entry is selected), floats and doubles.
// Prints "ok" and returns 0, or says what differs.  Never shipped.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "bb_solve.h"

using namespace bb;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double rnd() {  // xorshift64*, uniform in [-1, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return double((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / double(1ull << 52) - 1.0;
}
// magnitudes spread over many binades, so that the sums round differently in another order
static double wide() { return rnd() * exp2(floor(rnd() * 20.0)); }

template <typename T>
static bool same(T a, T b) { return memcmp(&a, &b, sizeof a) == 0; }

template <typename T>
static int check(const char* name, int trials) {
  for (int t = 0; t < trials; t++) {
    WheelCon<T> C;
    T x[NV];
    for (int r = 0; r < 3; r++) {
      for (int i = 0; i < 13; i++) C.J[r][i] = T(t % 4 == 1 ? rnd() : wide());
      C.aref[r] = T(wide());
      C.D[r] = T(rnd());
    }
    for (int i = 0; i < NV; i++) x[i] = T(t % 4 == 2 ? rnd() : wide());
    if (t % 7 == 3) {  // signed zeros and a column of zeros
      x[6] = x[7] = x[8] = T(-0.0);
      for (int r = 0; r < 3; r++) C.J[r][2] = T(0);
    }
    for (int w = 0; w < 3; w++) {
      T got[3], gjar[3];
      wheel_dot3(C, w, x, got);
      wheel_jar3(C, w, x, gjar);
      for (int r = 0; r < 3; r++) {
        const T want = wheel_dot(C, w, r, x);
        const T wjar = wheel_dot(C, w, r, x) - C.aref[r];
        if (!same(got[r], want))
          return printf("%s trial %d wheel %d row %d: batched %a, wheel_dot %a\n", name, t, w, r, double(got[r]),
                        double(want)), 1;
        if (!same(gjar[r], wjar))
          return printf("%s trial %d wheel %d row %d: batched jar %a, wheel_dot - aref %a\n", name, t, w, r,
                        double(gjar[r]), double(wjar)), 1;
      }
    }
  }
  return 0;
}

// the check must be able to fail: another summation order gives other bits on some of these inputs
template <typename T>
static int order_matters(int trials) {
  int differ = 0;
  for (int t = 0; t < trials; t++) {
    WheelCon<T> C;
    T x[NV];
    for (int r = 0; r < 3; r++)
      for (int i = 0; i < 13; i++) C.J[r][i] = T(wide());
    for (int i = 0; i < NV; i++) x[i] = T(wide());
    T acc = 0;
    for (int i = 0; i < 13; i++) acc += C.J[0][i] * x[wheel_col(i, 1)];  // plain column order
    differ += !same(acc, wheel_dot(C, 1, 0, x));
  }
  return differ == 0 ? printf("no input told the column order from wheel_dot's\n"), 1 : 0;
}

int main() {
  if (check<double>("double", 2000) || check<float>("float", 2000)) return 1;
  if (order_matters<double>(200) || order_matters<float>(200)) return 1;
  printf("ok\n");
  return 0;
}
