// Test-only host program (tests/test_host_hrow.py): where the fast kernels' solve finds its
// operands (kHrowSquare, kGroundRecord: bb_solve.h; kSum3: bb_team16.h), against the forms they
// replace, bit for bit, in float and double.
//   * the dense mass matrix by rows: sixteen lanes read their rows out of the packed triangle
//     through hidx, all of them before the first store, and store them at hsq_row_off (the
//     addressing of t16::mass_rows_team); then element k of the row at hsq_row_off(i) equals the
//     triangle's entry hidx(i, k) for every (i, k), no two rows overlap, every row lies in W.H or
//     in the stored contacts' head of W.g, and no other byte of the workspace has changed.
//     Random symmetric matrices over many binades with +-0, denormals and NaN among the entries
//   * the stored ball-terrain contact: ground_contact's J[3][6], aref[3] and D written to the
//     record at grec_off(c) as t16::ground_setup does and read back as t16::ground_get does, for
//     every c below GC_LDS (contact 0, contact 12, both sides of the W.bc / mass-block boundary
//     GREC_BC); the records lie in W.bc and W.M, overlap neither each other nor a row, and the
//     parent's two regions (W.bc + 18 c, the mass blocks + 4 c) give the same values
//   * the three team sums behind the sweeps: sixteen lanes with the DPP row sums emulated stage by
//     stage (row_mirror, row_half_mirror, quad_perm [2,3,0,1], [1,0,3,2]); the parent's text (d0,
//     the finite / descent test, the diagonal fallback, then M s, sMs and gs) against the
//     product's (M s first, one interleaved three-value sum, the fallback summing again), on
//     random operands, on a non-finite s, on d0 >= 0 with a fallback that descends and with one
//     that does not (both leave the iteration: only that is compared then)
// Two NaNs count as equal whatever their payloads.  Prints "ok" and returns 0, or says what
// differs.  Never shipped.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bb_model.h"
#include "bb_step.h"

using namespace bb;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
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
static const char* tname() { return sizeof(T) == 8 ? "double" : "float"; }

template <typename T>
static T value(int cs, int i) {
  const T den = sizeof(T) == 8 ? T(5e-324) : T(1.4e-45);
  const int span = sizeof(T) == 8 ? 60 : 30;
  const T x = T(ldexp(rnd(), (cs % (2 * span + 1)) - span));
  if (cs % 5 == 2) {
    switch ((cs / 5 + i) % 8) {
      case 0: return T(0);
      case 1: return -T(0);
      case 2: return den;
      case 3: return -den;
      case 4: return cs % 3 == 0 ? T(NAN) : x;
      default: return x;
    }
  }
  return x;
}

// [lo, hi) in entries of T from the workspace's start
struct Span { int lo, hi; };
static bool overlap(Span a, Span b) { return a.lo < b.hi && b.lo < a.hi; }
template <typename T>
static Span member(size_t off, size_t bytes) { return Span{int(off / sizeof(T)), int((off + bytes) / sizeof(T))}; }
static bool inside(Span a, Span b) { return a.lo >= b.lo && a.hi <= b.hi; }

template <typename T>
static int check_rows() {
  typedef EnvWork<T> W_t;
  const Span Hs = member<T>(offsetof(W_t, H), sizeof(T) * (NH + HX));
  const Span Gs = member<T>(offsetof(W_t, g), sizeof(T) * GC_LDS * NGF);
  for (int i = 0; i < NV; i++) {
    const Span r{hsq_row_off<T>(i), hsq_row_off<T>(i) + HS};
    if (!inside(r, Hs) && !inside(r, Gs)) return printf("row %d (%s) outside W.H and the head of W.g\n", i, tname<T>()), 1;
    for (int j = 0; j < i; j++)
      if (overlap(r, Span{hsq_row_off<T>(j), hsq_row_off<T>(j) + HS})) return printf("rows %d and %d overlap\n", i, j), 1;
  }
  static W_t W, W0;
  for (int cs = 0; cs < 400; cs++) {
    unsigned char* wb = reinterpret_cast<unsigned char*>(&W);
    for (size_t b = 0; b < sizeof W; b++) wb[b] = (unsigned char)(0xA5 ^ (b * 7 + cs));
    T tri[NH];
    for (int e = 0; e < NH; e++) tri[e] = W.H[e] = value<T>(cs, e);
    memcpy(&W0, &W, sizeof W);
    // mass_rows_team, lane by lane: every lane's loads, then every lane's stores
    T x[16][NV];
    for (int tl = 0; tl < 16; tl++) {
      const int row = tl < NV ? tl : NV - 1;
      for (int k = 0; k < NV; k++) x[tl][k] = W.H[hidx(row, k)];
    }
    for (int tl = 0; tl < 16; tl++) {
      const int row = tl < NV ? tl : NV - 1;
      T* o = ws_at(W, hsq_row_off<T>(row));
      for (int k = 0; k < NV; k++) o[k] = x[tl][k];
    }
    for (int i = 0; i < NV; i++) {
      const T* hrow = ws_at(W, hsq_row_off<T>(i));
      for (int k = 0; k < NV; k++)
        if (!same(hrow[k], tri[hidx(i, k)]))
          return printf("square copy (%s), case %d, (%d, %d): %.17g vs %.17g\n", tname<T>(), cs, i, k, double(hrow[k]),
                        double(tri[hidx(i, k)])), 1;
    }
    // nothing but the rows has changed
    std::vector<bool> row_byte(sizeof W, false);
    for (int i = 0; i < NV; i++)
      for (size_t b = 0; b < HS * sizeof(T); b++) row_byte[hsq_row_off<T>(i) * sizeof(T) + b] = true;
    const unsigned char* w0 = reinterpret_cast<const unsigned char*>(&W0);
    for (size_t b = 0; b < sizeof W; b++)
      if (!row_byte[b] && wb[b] != w0[b]) return printf("byte %zu of the workspace changed (%s)\n", b, tname<T>()), 1;
  }
  return 0;
}

template <typename T>
static int check_records(const ModelT<T>& m) {
  typedef EnvWork<T> W_t;
  const Span Bs = member<T>(offsetof(W_t, bc), sizeof(T) * MAXB_LDS * NBF);
  const Span Ms = member<T>(offsetof(W_t, M), sizeof(Mass<T>));
  if (GREC_BC < 1 || GREC_BC >= GC_LDS) return printf("no W.bc / mass-block boundary below GC_LDS\n"), 1;
  for (int c = 0; c < GC_LDS; c++) {
    const Span r{grec_off<T>(c), grec_off<T>(c) + GREC};
    if (!inside(r, c < GREC_BC ? Bs : Ms)) return printf("record %d (%s) outside its region\n", c, tname<T>()), 1;
    for (int d = 0; d < c; d++)
      if (overlap(r, Span{grec_off<T>(d), grec_off<T>(d) + GREC})) return printf("records %d and %d overlap\n", c, d), 1;
    for (int i = 0; i < NV; i++)
      if (overlap(r, Span{hsq_row_off<T>(i), hsq_row_off<T>(i) + HS})) return printf("record %d overlaps row %d\n", c, i), 1;
  }
  static W_t W, Wp;
  for (int cs = 0; cs < 60; cs++) {
    // contacts: unit normals about +z, distances on both sides of 0; a ball pose and a stage velocity
    T RB[9], v[NV];
    {
      T qn[4] = {T(1 + 0.3 * rnd()), T(0.4 * rnd()), T(0.4 * rnd()), T(0.4 * rnd())};
      qnormalize(qn);
      q2mat(RB, qn);
    }
    for (int i = 0; i < NV; i++) v[i] = T(rnd() * (cs % 4 == 0 ? 0.0 : 2.0));
    for (int i = 0; i < 9; i++) W.P.RB[i] = Wp.P.RB[i] = RB[i];
    for (int i = 0; i < NV; i++) W.vi[i] = Wp.vi[i] = v[i];
    for (int c = 0; c < GC_LDS; c++) {
      T n[3] = {T(0.5 * rnd()), T(0.5 * rnd()), T(1)};
      const T inl = T(1) / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      for (int i = 0; i < 3; i++) W.g[c * NGF + GF_N + i] = Wp.g[c * NGF + GF_N + i] = n[i] * inl;
      W.g[c * NGF + GF_DIST] = Wp.g[c * NGF + GF_DIST] = T(0.01 * rnd());
    }
    T J[GC_LDS][3][6], ar[GC_LDS][3], D[GC_LDS];
    for (int c = 0; c < GC_LDS; c++) ground_contact(m, W.g + c * NGF, W.P.RB, W.vi, J[c], ar[c], D[c]);
    for (int c = 0; c < GC_LDS; c++) {  // ground_setup: the record, and the parent's two regions
      T* o = ws_at(W, grec_off<T>(c));
      for (int r = 0; r < 3; r++)
        for (int i = 0; i < 6; i++) o[6 * r + i] = J[c][r][i];
      for (int r = 0; r < 3; r++) o[GREC_AREF + r] = ar[c][r];
      o[GREC_D] = D[c];
      T* po = Wp.bc + c * 18;
      for (int r = 0; r < 3; r++)
        for (int i = 0; i < 6; i++) po[6 * r + i] = J[c][r][i];
      T* pa = reinterpret_cast<T*>(&Wp.M) + 4 * c;
      for (int r = 0; r < 3; r++) pa[r] = ar[c][r];
      pa[3] = D[c];
    }
    for (int c = 0; c < GC_LDS; c++) {  // ground_get, both ways
      const T* o = ws_at(W, grec_off<T>(c));
      const T* po = Wp.bc + c * 18;
      const T* pa = reinterpret_cast<const T*>(&Wp.M) + 4 * c;
      for (int r = 0; r < 3; r++) {
        for (int i = 0; i < 6; i++)
          if (!same(o[6 * r + i], J[c][r][i]) || !same(po[6 * r + i], J[c][r][i]))
            return printf("record %d (%s), case %d: J[%d][%d]\n", c, tname<T>(), cs, r, i), 1;
        if (!same(o[GREC_AREF + r], ar[c][r]) || !same(pa[r], ar[c][r]))
          return printf("record %d (%s), case %d: aref[%d]\n", c, tname<T>(), cs, r), 1;
      }
      if (!same(o[GREC_D], D[c]) || !same(pa[3], D[c])) return printf("record %d (%s), case %d: D\n", c, tname<T>(), cs), 1;
    }
  }
  return 0;
}

// ---- the team sums: sixteen lanes, the DPP stages of t16::tsum / tsum_n ----
template <typename T>
struct Lanes { T v[16]; };
template <typename T>
static void stage(Lanes<T>& x, int st) {
  Lanes<T> y = x;
  for (int i = 0; i < 16; i++) {
    const int src = st == 0 ? 15 - i : st == 1 ? (i & 8) | (7 - (i & 7)) : st == 2 ? i ^ 2 : i ^ 1;
    x.v[i] = y.v[i] + y.v[src];
  }
}
template <typename T>
static Lanes<T> tsum(Lanes<T> x) {
  for (int st = 0; st < 4; st++) stage(x, st);
  return x;
}
template <typename T>
static void tsum3(Lanes<T> (&x)[3]) {
  for (int st = 0; st < 4; st++)
    for (int j = 0; j < 3; j++) stage(x[j], st);
}

template <typename T>
struct SumsIn {
  T Hd[NV][NV];  // dense symmetric M
  T s[NV];       // the sweeps' s (replicated), sown = s[row] on the row lanes
  T gi[16], mq[16];
};
template <typename T>
struct SumsOut {
  bool left;  // the iteration ended in the fallback (`break`)
  T d0, sMs, gs, s[NV], sown[16], Ms[16];
};

template <bool SUM3, typename T>
static SumsOut<T> run_sums(const SumsIn<T>& in) {
  SumsOut<T> o;
  o.left = false;
  T s[NV];
  Lanes<T> sown, Ms, p[3];
  for (int k = 0; k < NV; k++) s[k] = in.s[k];
  for (int tl = 0; tl < 16; tl++) sown.v[tl] = tl < NV ? s[tl] : T(0);
  auto ms_of = [&]() {
    for (int tl = 0; tl < 16; tl++) {
      const int row = tl < NV ? tl : NV - 1;
      T a = 0;
      for (int k = 0; k < NV; k++) a += in.Hd[row][k] * s[k];
      Ms.v[tl] = a;
    }
  };
  auto prod = [&](const Lanes<T>& a, const T* b) {
    Lanes<T> r;
    for (int tl = 0; tl < 16; tl++) r.v[tl] = a.v[tl] * b[tl];
    return r;
  };
  T d0, sMs = 0, gs = 0;
  if (SUM3) {
    ms_of();
    p[0] = prod(sown, in.gi); p[1] = prod(sown, Ms.v); p[2] = prod(sown, in.mq);
    tsum3(p);
    d0 = p[0].v[0]; sMs = p[1].v[0]; gs = p[2].v[0];
    for (int j = 0; j < 3; j++)
      for (int tl = 1; tl < 16; tl++)
        if (!same(p[j].v[tl], p[j].v[0])) { o.left = true; o.d0 = T(-777); return o; }  // lanes disagree: flagged below
  } else {
    d0 = tsum(prod(sown, in.gi)).v[0];
  }
  bool fin = true;
  for (int i = 0; i < NV; i++) fin = fin && isfinite(s[i]);
  if (!fin || !(d0 < 0)) {
    for (int tl = 0; tl < 16; tl++) {
      const int row = tl < NV ? tl : NV - 1;
      sown.v[tl] = tl < NV ? -in.gi[tl] / maxT(in.Hd[row][row], T(1e-30)) : T(0);
    }
    for (int k = 0; k < NV; k++) s[k] = sown.v[k];
    d0 = tsum(prod(sown, in.gi)).v[0];
    if (!(d0 < 0)) { o.left = true; o.d0 = d0; return o; }
    if (SUM3) {
      ms_of();
      sMs = tsum(prod(sown, Ms.v)).v[0];
      gs = tsum(prod(sown, in.mq)).v[0];
    }
  }
  if (!SUM3) {
    ms_of();
    sMs = tsum(prod(sown, Ms.v)).v[0];
    gs = tsum(prod(sown, in.mq)).v[0];
  }
  o.d0 = d0; o.sMs = sMs; o.gs = gs;
  for (int k = 0; k < NV; k++) o.s[k] = s[k];
  for (int tl = 0; tl < 16; tl++) { o.sown[tl] = sown.v[tl]; o.Ms[tl] = Ms.v[tl]; }
  return o;
}

template <typename T>
static int check_sums() {
  int n_fallback = 0, n_left = 0, n_nonfinite = 0, n_plain = 0;
  for (int cs = 0; cs < 2000; cs++) {
    SumsIn<T> in;
    for (int i = 0; i < NV; i++)
      for (int k = 0; k <= i; k++) in.Hd[i][k] = in.Hd[k][i] = T(rnd() + (i == k ? 3.0 : 0.0));
    const int kind = cs % 8;  // 0-3 a descent direction; 4 a non-finite s; 5, 6 d0 >= 0; 7 d0 >= 0 and no descent after
    for (int tl = 0; tl < 16; tl++) {
      in.gi[tl] = tl < NV ? T(ldexp(rnd(), cs % 40 - 20)) : T(0);
      in.mq[tl] = tl < NV ? T(rnd()) : T(0);
    }
    for (int k = 0; k < NV; k++) in.s[k] = kind >= 5 ? in.gi[k] * T(0.5 + 0.4 * rnd()) : -in.gi[k] * T(0.5 + 0.4 * rnd());
    if (kind == 4) in.s[cs % NV] = (cs / 8) % 2 ? T(NAN) : T(INFINITY);
    if (kind == 7)
      for (int tl = 0; tl < NV; tl++) in.gi[tl] = T(0);  // the diagonal step is 0: d0 = 0, the iteration ends
    const SumsOut<T> a = run_sums<false>(in), b = run_sums<true>(in);
    if (b.left && b.d0 == T(-777)) return printf("sums (%s), case %d: the lanes of tsum_n disagree\n", tname<T>(), cs), 1;
    if (a.left != b.left) return printf("sums (%s), case %d: one form leaves the iteration\n", tname<T>(), cs), 1;
    if (!same(a.d0, b.d0)) return printf("sums (%s), case %d: d0 %.17g vs %.17g\n", tname<T>(), cs, double(a.d0), double(b.d0)), 1;
    if (a.left) { n_left++; continue; }
    if (!same(a.sMs, b.sMs) || !same(a.gs, b.gs))
      return printf("sums (%s), case %d: sMs %.17g vs %.17g, gs %.17g vs %.17g\n", tname<T>(), cs, double(a.sMs),
                    double(b.sMs), double(a.gs), double(b.gs)), 1;
    for (int k = 0; k < NV; k++)
      if (!same(a.s[k], b.s[k])) return printf("sums (%s), case %d: s[%d]\n", tname<T>(), cs, k), 1;
    for (int tl = 0; tl < 16; tl++)
      if (!same(a.sown[tl], b.sown[tl]) || !same(a.Ms[tl], b.Ms[tl])) return printf("sums (%s), case %d: lane %d\n", tname<T>(), cs, tl), 1;
    if (kind == 4) n_nonfinite++;
    if (kind >= 4) n_fallback++; else n_plain++;
  }
  if (!n_fallback || !n_left || !n_nonfinite || !n_plain)
    return printf("sums (%s): a branch was not reached (%d %d %d %d)\n", tname<T>(), n_fallback, n_left, n_nonfinite, n_plain), 1;
  return 0;
}

template <typename T>
static int run(const ModelT<T>& m) {
  return check_rows<T>() || check_records<T>(m) || check_sums<T>();
}

int main() {
  const ModelT<double> md = compile_model(default_solver(true));
  const ModelT<float> mf = cast_model<float>(compile_model(default_solver(false)));
  if (run<double>(md) || run<float>(mf)) return 1;
  printf("ok\n");
  return 0;
}
