// Test-only host program (tests/test_host_pre_batch.py): the forward's batched-read forms
// (kPreBatchRk / kPreBatchDense: bb_physics.h, bb_step.h, bb_solve.h, bb_team16.h) against copies
// of the text they replace, bit for bit, in float and double.
//   * rk_sums_batch, first and later stages   vs  parent_rk_sums (rk4_step's loops, through the
//                                                 workspace's warm start as the kernels run them)
//   * Mass as an array at mass_entry_off(i, j), for every i >= j   vs  mass_entry(M, i, j);
//     tri_unpack_count vs tri_unpack for every packed index; and the packed matrix copied the way
//     mass_dense_team's batched form does it, for every team lane, vs the serial loop
// Inputs: seeded values scaled over many binades (2^-60 .. 2^60; floats 2^-30 .. 2^30), signed
// zeros, denormals, NaN, +-1e10.  Two NaNs count as equal whatever their payloads.  On the host
// the issue fence is empty: the program checks the operands, the operations and their order;
// tests/test_gpu_pre_batch.py checks the kernels.  bias_finish_half and ground_setup keep their
// text (no angular velocity or quaternion enters the forms above), so nothing of theirs is here.
// Prints "ok" and returns 0, or says what differs.  Never shipped.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "bb_model.h"
#include "bb_step.h"

using namespace bb;

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static double rnd() {  // xorshift64*, uniform in [-1, 1)
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return double((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / double(1ull << 52) - 1.0;
}

template <typename T>
static bool same(T a, T b) {
  if (a != a && b != b) return true;
  return memcmp(&a, &b, sizeof a) == 0;
}
template <typename T>
static int differ(const char* what, int cs, const T* a, const T* b, int n) {
  for (int i = 0; i < n; i++)
    if (!same(a[i], b[i])) {
      printf("%s (%s), case %d, entry %d: %.17g vs %.17g\n", what, sizeof(T) == 8 ? "double" : "float", cs, i,
             double(a[i]), double(b[i]));
      return 1;
    }
  return 0;
}

// a value for slot `i` of case `cs`: random over the case's binade, with the special values mixed in
template <typename T>
static T value(int cs, int i) {
  const T den = sizeof(T) == 8 ? T(5e-324) : T(1.4e-45);
  const int span = sizeof(T) == 8 ? 60 : 30;
  const T x = T(ldexp(rnd(), (cs % (2 * span + 1)) - span));
  if (cs % 7 == 3) {
    switch ((cs / 7 + i) % 9) {
      case 0: return T(0);
      case 1: return -T(0);
      case 2: return den;
      case 3: return -den;
      case 4: return T(1e10);
      case 5: return T(-1e10);
      case 6: return cs % 5 == 0 ? T(NAN) : x;
      default: return x;
    }
  }
  return x;
}

// ---- the text before the batching (bb_step.h: rk4_step after a stage's solve) ----
template <typename T>
static void parent_rk_sums(int stage, T b, const T* vi, const T* acc, T* warm, T* vs, T* as, T* k1) {
  for (int i = 0; i < NV; i++) warm[i] = acc[i];
  if (stage == 0) {
    for (int i = 0; i < NV; i++) { vs[i] = b * vi[i]; as[i] = b * warm[i]; k1[i] = warm[i]; }
  } else {
    for (int i = 0; i < NV; i++) { vs[i] += b * vi[i]; as[i] += b * warm[i]; }
  }
}

template <typename T>
static int check_rk() {
  const T bs[2] = {T(1.0 / 6), T(1.0 / 3)};
  for (int cs = 0; cs < 600; cs++) {
    T vi[NV], acc[NV], vs0[NV], as0[NV];
    for (int i = 0; i < NV; i++) {
      vi[i] = value<T>(cs, i);
      acc[i] = value<T>(cs + 2, i + 5);
      vs0[i] = value<T>(cs + 1, i + 1);
      as0[i] = value<T>(cs + 3, i + 2);
    }
    for (int stage = 0; stage < 4; stage++) {
      const T b = (stage == 0 || stage == 3) ? bs[0] : bs[1];
      T warm[NV], vs1[NV], as1[NV], k11[NV], vs2[NV], as2[NV], k12[NV];
      for (int i = 0; i < NV; i++) { vs1[i] = vs2[i] = vs0[i]; as1[i] = as2[i] = as0[i]; k11[i] = k12[i] = T(-7); }
      parent_rk_sums(stage, b, vi, acc, warm, vs1, as1, k11);
      rk_sums_batch(stage == 0, b, vi, acc, vs2, as2, k12);
      if (differ("rk vs", cs, vs2, vs1, NV) || differ("rk as", cs, as2, as1, NV) || differ("rk k1", cs, k12, k11, NV))
        return 1;
    }
  }
  return 0;
}

template <typename T>
static int check_dense() {
  constexpr int L = 16, R = (NH + L - 1) / L;
  for (int e = 0; e < NH; e++) {
    int i1, j1, i2, j2;
    tri_unpack(e, i1, j1);
    tri_unpack_count(e, i2, j2);
    if (i1 != i2 || j1 != j2) return printf("tri_unpack_count(%d) = (%d, %d), tri_unpack (%d, %d)\n", e, i2, j2, i1, j1), 1;
  }
  for (int cs = 0; cs < 300; cs++) {
    Mass<T> M;
    T* Mp = reinterpret_cast<T*>(&M);
    const int nm = int(sizeof M / sizeof(T));
    for (int i = 0; i < nm; i++) Mp[i] = value<T>(cs, i);
    T H1[NH], H2[NH];
    int seen = 0;
    for (int i = 0; i < NV; i++)
      for (int j = 0; j <= i; j++) {
        const int o = mass_entry_off<T>(i, j);
        if (o >= nm) return printf("mass_entry_off(%d, %d) = %d past the struct\n", i, j, o), 1;
        const T got = o < 0 ? T(0) : Mp[o], ref = mass_entry(M, i, j);
        if (differ("mass_entry_off", i * NV + j, &got, &ref, 1)) return 1;
        seen++;
      }
    if (seen != NH) return printf("%d entries, NH = %d\n", seen, NH), 1;
    // the team's copy: the serial loop, and the batched form's addressing lane by lane
    for (int tl = 0; tl < L; tl++)
      for (int e = tl; e < NH; e += L) {
        int i, j;
        tri_unpack(e, i, j);
        H1[e] = mass_entry(M, i, j);
      }
    for (int e = 0; e < NH; e++) H2[e] = T(-3);
    for (int tl = 0; tl < L; tl++) {
      int o[R];
      T x[R];
      for (int r = 0; r < R; r++) {
        const int e = tl + r * L;
        int i, j;
        tri_unpack_count(e < NH ? e : NH - 1, i, j);
        o[r] = mass_entry_off<T>(i, j);
        x[r] = Mp[o[r] < 0 ? 0 : o[r]];
      }
      for (int r = 0; r < R; r++) {
        const int e = tl + r * L;
        if (e < NH) H2[e] = o[r] < 0 ? T(0) : x[r];
      }
    }
    if (differ("dense mass", cs, H2, H1, NH)) return 1;
  }
  return 0;
}

template <typename T>
static int run() {
  return check_rk<T>() || check_dense<T>();
}

int main() {
  if (run<double>() || run<float>()) return 1;
  printf("ok\n");
  return 0;
}
