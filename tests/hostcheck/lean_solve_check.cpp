// Test-only host program (tests/test_host_lean_solve.py): the lean forms of the FUSE kernels'
// factorisation and sweeps (bb_team16.h: kLeanMax, kLeanFloor, kLeanDiag, kLeanLtr) against
// the text they replace, over sixteen emulated lanes, bit for bit, in float and double.  lane_pick,
// pivot_floor and ltr_lane_addr / ltr_lane_slot are the kernels' own functions.  A broadcast is
// the source lane's value; an FMA is fma(); the pivot's reciprocal square root is 1 / sqrt in both forms; v_max is modelled for quiet operands (a NaN gives the other
// operand), which is all the kernels' arithmetic produces.
//   * chol_rows: the floor formed once per lane from the diagonal that lane_pick's select tree
//     finds, the maximum taken on the lane's own entry and then broadcast, against the in-loop
//     floor of the broadcast diagonal; every entry of every lane's row, every diag[j] on every
//     lane, and down == diag[lane] (0 on lane 15)
//   * chol_solve_rows: the forward sweep on down, the transpose's stores through ltr_lane_slot,
//     the column read back out of the packed triangle, and (doubles) the backward sweep's s_i as bcast(z down) where it was bcast(z) diag[i]; every s[i] on every
//     lane and every sown
//   * the addresses: ltr_lane_slot == ltr_slot for every lane and entry, every entry that is not
//     below the diagonal in LTR_SPARE
// Inputs: seeded symmetric positive-definite matrices over many binades; matrices of rank 1 to 14
// and matrices with a zero or negative diagonal, whose pivots reach the floor; +-0, denormals,
// +-inf and NaN planted in the matrix, on its diagonal and in the right-hand side; the sweeps also
// on factors and inverse pivots that hold such values directly.  Two NaNs count as equal whatever
// their payloads.  Prints "ok" and returns 0, or says what differs.  Never shipped.
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
static int rint_below(int n) { return int((rnd() * 0.5 + 0.5) * n) % n; }

template <typename T>
static bool same(T a, T b) {
  if (a != a && b != b) return true;
  return memcmp(&a, &b, sizeof a) == 0;
}
template <typename T>
static const char* tname() { return sizeof(T) == 8 ? "double" : "float"; }

// v_max on quiet operands
template <typename T>
static T hw_max(T a, T b) {
  if (a != a) return b;
  if (b != b) return a;
  if (a == b) return signbit(a) ? b : a;
  return a > b ? a : b;
}
template <typename T>
static T rsq(T x) { return T(1) / sqrt(x); }

template <typename T>
struct Lanes16 {
  T h[16][NV];     // lane l: row min(l, NV - 1)
  T diag[16][NV];  // replicated inverse pivots, as each lane computed them
  T down[16];
};

static int n_floor = 0;  // pivots that took the floor

// the parent's chol_rows<true>: floor of the broadcast diagonal inside the column loop
template <typename T>
static void chol_parent(Lanes16<T>& t) {
  T hdi[16];
  for (int l = 0; l < 16; l++) {
    const int row = l < NV ? l : NV - 1;
    hdi[l] = 0;
    for (int k = 0; k < NV; k++) hdi[l] = row == k ? t.h[l][k] : hdi[l];
  }
  for (int j = 0; j < NV; j++) {
    T id[16];
    for (int l = 0; l < 16; l++) {
      T piv = t.h[j][j];
      const T hdj = hdi[j];
      const T fl = pivot_eps<T>() * maxT(hdj, T(1e-30));
      if (l == 0 && !(piv > fl)) n_floor++;
      piv = hw_max(piv, fl);
      id[l] = rsq(piv);
      t.diag[l][j] = id[l];
    }
    T c[16];
    for (int l = 0; l < 16; l++) c[l] = t.h[l][j] = t.h[l][j] * id[l];
    for (int k = j + 1; k < NV; k++)
      for (int l = 0; l < 16; l++) t.h[l][k] = fma(-c[k], c[l], t.h[l][k]);
  }
  for (int l = 0; l < 16; l++) t.down[l] = 0;
}

// the lean chol_rows<true>
template <typename T>
static void chol_lean(Lanes16<T>& t) {
  T flo[16];
  for (int l = 0; l < 16; l++) flo[l] = pivot_floor(lane_pick(t.h[l], t.h[l][NV - 1], l));
  for (int j = 0; j < NV; j++) {
    T m[16], id[16];
    for (int l = 0; l < 16; l++) m[l] = hw_max(t.h[l][j], flo[l]);
    for (int l = 0; l < 16; l++) {
      id[l] = rsq(m[j]);
      t.diag[l][j] = id[l];
    }
    T c[16];
    for (int l = 0; l < 16; l++) c[l] = t.h[l][j] = t.h[l][j] * id[l];
    for (int k = j + 1; k < NV; k++)
      for (int l = 0; l < 16; l++) t.h[l][k] = fma(-c[k], c[l], t.h[l][k]);
  }
  for (int l = 0; l < 16; l++) t.down[l] = lane_pick(t.diag[l], T(0), l);
}

template <typename T>
struct Sol {
  T s[16][NV], sown[16];
};

// the parent's chol_solve_rows<true, true>
template <typename T>
static void solve_parent(const Lanes16<T>& t, const T* g, Sol<T>& o) {
  T b[16], z[16], tt[16];
  for (int l = 0; l < 16; l++) { b[l] = l < NV ? -g[l] : T(0); z[l] = 0; }
  for (int j = 0; j < NV; j++) {
    for (int l = 0; l < 16; l++) { tt[l] = b[l] * t.diag[l][j]; z[l] = l == j ? tt[l] : z[l]; }
    for (int l = 0; l < 16; l++) b[l] = fma(-tt[j], t.h[l][j], b[l]);
  }
  T scr[LTR_SLOTS];
  for (int i = 0; i < LTR_SLOTS; i++) scr[i] = T(NAN);
  for (int k = 0; k < NV - 1; k++)
    for (int l = 0; l < 16; l++) scr[ltr_slot(l, k)] = t.h[l][k];
  T Lc[16][NV], own[16];
  for (int l = 0; l < 16; l++) {
    own[l] = 0;
    for (int i = 0; i < NV; i++) Lc[l][i] = i > l ? scr[i * (i - 1) / 2 + l] : T(0);
  }
  for (int i = NV - 1; i >= 0; i--) {
    T si[16];
    for (int l = 0; l < 16; l++) si[l] = z[i] * t.diag[l][i];
    for (int l = 0; l < 16; l++) {
      o.s[l][i] = si[l];
      z[l] = fma(-Lc[l][i], si[l], z[l]);  // z -= Lc si, contracted to one FMA in the kernel
      own[l] = l == i ? si[l] : own[l];
    }
  }
  for (int l = 0; l < 16; l++) o.sown[l] = own[l];
}

// the lean chol_solve_rows<true, true>; returns nonzero on an address out of place
template <typename T>
static int solve_lean(const Lanes16<T>& t, const T* g, Sol<T>& o) {
  T b[16], z[16], tt[16];
  for (int l = 0; l < 16; l++) { b[l] = l < NV ? -g[l] : T(0); z[l] = 0; }
  for (int j = 0; j < NV; j++) {
    for (int l = 0; l < 16; l++) { tt[l] = b[l] * t.down[l]; z[l] = l == j ? tt[l] : z[l]; }
    for (int l = 0; l < 16; l++) b[l] = fma(-tt[j], t.h[l][j], b[l]);
  }
  T scr[LTR_SLOTS];
  for (int i = 0; i < LTR_SLOTS; i++) scr[i] = T(NAN);
  for (int k = 0; k < NV - 1; k++)
    for (int l = 0; l < 16; l++) {
      const int slot = ltr_lane_slot(ltr_lane_base(l), ltr_rows(l), k);
      if (slot < 0 || slot >= LTR_SLOTS) return printf("store slot %d out of range\n", slot), 1;
      scr[slot] = t.h[l][k];
    }
  T Lc[16][NV], own[16];
  for (int l = 0; l < 16; l++) {
    own[l] = 0;
    for (int i = 0; i < NV; i++) Lc[l][i] = i > l ? scr[i * (i - 1) / 2 + l] : T(0);
  }
  for (int i = NV - 1; i >= 0; i--) {
    if (sizeof(T) == 8) {
      for (int l = 0; l < 16; l++) tt[l] = z[l] * t.down[l];  // lane i's is s_i, broadcast
      for (int l = 0; l < 16; l++) {
        o.s[l][i] = tt[i];
        z[l] = fma(-Lc[l][i], tt[i], z[l]);
        own[l] = l == i ? tt[i] : own[l];
      }
    } else {  // floats keep the parent's backward sweep
      T si[16];
      for (int l = 0; l < 16; l++) si[l] = z[i] * t.diag[l][i];
      for (int l = 0; l < 16; l++) {
        o.s[l][i] = si[l];
        z[l] = fma(-Lc[l][i], si[l], z[l]);
        own[l] = l == i ? si[l] : own[l];
      }
    }
  }
  for (int l = 0; l < 16; l++) o.sown[l] = own[l];
  return 0;
}

template <typename T>
static T special(int which) {
  const T den = sizeof(T) == 8 ? T(5e-324) : T(1.4e-45);
  switch (which % 8) {
    case 0: return T(0);
    case 1: return -T(0);
    case 2: return den;
    case 3: return -den;
    case 4: return T(INFINITY);
    case 5: return -T(INFINITY);
    case 6: return T(NAN);
    default: return den * T(1000);
  }
}

template <typename T>
static int compare(const char* what, int cs, const Lanes16<T>& a, const Lanes16<T>& b, const Sol<T>& sa, const Sol<T>& sb) {
  for (int l = 0; l < 16; l++) {
    for (int k = 0; k < NV; k++) {
      if (!same(a.h[l][k], b.h[l][k])) return printf("%s (%s) case %d: L lane %d entry %d\n", what, tname<T>(), cs, l, k), 1;
      if (!same(a.diag[l][k], b.diag[l][k])) return printf("%s (%s) case %d: diag lane %d entry %d\n", what, tname<T>(), cs, l, k), 1;
      if (!same(sa.s[l][k], sb.s[l][k]))
        return printf("%s (%s) case %d: s[%d] on lane %d: %.17g vs %.17g\n", what, tname<T>(), cs, k, l, double(sa.s[l][k]),
                      double(sb.s[l][k])), 1;
    }
    if (!same(b.down[l], l < NV ? a.diag[l][l] : T(0))) return printf("%s (%s) case %d: down on lane %d\n", what, tname<T>(), cs, l), 1;
    if (!same(sa.sown[l], sb.sown[l])) return printf("%s (%s) case %d: sown on lane %d\n", what, tname<T>(), cs, l), 1;
  }
  return 0;
}

template <typename T>
static int check_addresses() {
  for (int tl = 0; tl < 16; tl++)
    for (int k = 0; k < NV - 1; k++) {
      const int got = ltr_lane_slot(ltr_lane_base(tl), ltr_rows(tl), k), want = ltr_slot(tl, k);
      if (got != want) return printf("lane %d entry %d: slot %d, ltr_slot %d\n", tl, k, got, want), 1;
      const bool below = tl < NV && k < tl;
      if (!below && got != LTR_SPARE) return printf("lane %d entry %d: slot %d is not the spare\n", tl, k, got), 1;
      if (below && got != tl * (tl - 1) / 2 + k) return printf("lane %d entry %d: slot %d is not its packed place\n", tl, k, got), 1;
    }
  return 0;
}

template <typename T>
static int check_solve() {
  int n_spd = 0, n_nonfinite = 0;
  const int floor0 = n_floor;
  for (int cs = 0; cs < 1500; cs++) {
    const int kind = cs % 5;  // 0, 1 positive definite; 2 rank-deficient; 3 a bad diagonal; 4 specials planted
    double A[NV][NV];
    const int rank = kind == 2 ? 1 + cs / 5 % (NV - 1) : NV;
    double B[NV][NV];
    for (int i = 0; i < NV; i++)
      for (int k = 0; k < NV; k++) B[i][k] = k < rank ? rnd() : 0.0;
    const double scale = ldexp(1.0, (cs % 41 - 20) * (sizeof(T) == 8 ? 3 : 1));
    for (int i = 0; i < NV; i++)
      for (int k = 0; k <= i; k++) {
        double a = 0;
        for (int r = 0; r < NV; r++) a += B[i][r] * B[k][r];
        if (i == k && kind != 2) a += 0.5;
        A[i][k] = A[k][i] = a * scale;
      }
    if (kind == 3) {
      const int i = rint_below(NV);
      A[i][i] = cs % 2 ? 0.0 : -A[i][i];
    }
    T g[16];
    for (int l = 0; l < 16; l++) g[l] = T(ldexp(rnd(), cs % 30 - 15));
    if (kind == 4) {
      const int n = 1 + cs / 5 % 3;
      for (int r = 0; r < n; r++) {
        const int where = (cs / 15 + r) % 3, i = rint_below(NV), k = rint_below(NV);
        const double v = double(special<T>(cs / 5 + r));
        if (where == 0) A[i][k] = A[k][i] = v;
        else if (where == 1) A[i][i] = v;
        else g[i] = T(v);
      }
    }
    Lanes16<T> a, b;
    for (int l = 0; l < 16; l++) {
      const int row = l < NV ? l : NV - 1;
      for (int k = 0; k < NV; k++) a.h[l][k] = b.h[l][k] = T(A[row][k]);
    }
    g[15] = g[14];  // lane 15 is handed row 14's gradient and ignores it
    chol_parent(a);
    chol_lean(b);
    Sol<T> sa, sb;
    solve_parent(a, g, sa);
    if (solve_lean(b, g, sb)) return 1;
    if (compare("factorise and solve", cs, a, b, sa, sb)) return 1;
    bool fin = true;
    for (int k = 0; k < NV; k++) fin = fin && isfinite(sa.s[0][k]);
    if (fin && kind < 2) n_spd++;
    if (!fin) n_nonfinite++;
  }
  // the sweeps alone on factors, inverse pivots and right-hand sides that hold the special values
  for (int cs = 0; cs < 1500; cs++) {
    Lanes16<T> a;
    T g[16];
    T dg[NV];
    for (int k = 0; k < NV; k++) dg[k] = T(0.5 + 0.4 * rnd());
    if (cs % 3 == 1) dg[rint_below(NV)] = special<T>(cs);
    for (int l = 0; l < 16; l++) {
      for (int k = 0; k < NV; k++) {
        a.h[l][k] = T(rnd());
        a.diag[l][k] = dg[k];
      }
      a.down[l] = l < NV ? dg[l] : T(0);
      g[l] = T(rnd());
    }
    if (cs % 3 == 0) a.h[rint_below(NV)][rint_below(NV)] = special<T>(cs / 3);
    if (cs % 3 == 2) g[rint_below(NV)] = special<T>(cs / 3);
    Sol<T> sa, sb;
    solve_parent(a, g, sa);
    if (solve_lean(a, g, sb)) return 1;
    if (compare("sweeps", cs, a, a, sa, sb)) return 1;
  }
  if (!n_spd || !n_nonfinite || n_floor == floor0)
    return printf("(%s) a regime was not reached: %d finite, %d non-finite, %d floored pivots\n", tname<T>(), n_spd, n_nonfinite,
                  n_floor - floor0), 1;
  return 0;
}

int main() {
  if (check_addresses<double>() || check_solve<double>() || check_solve<float>()) return 1;
  printf("ok\n");
  return 0;
}
