// Test-only host program (tests/test_gpu_ls_select.py): the branch-free forms of the line search
// (bb_solve.h: LsTerm::prep_sel, LineSearch::crosses_sel, ls_advance) against copies, kept here, of
// the branching forms they stand in for: prep's `if (vv > 0)`, the short-circuit crosses, and the
// evaluation loop with its three breaks and its lazily summed dmag and d2.  Bit for bit, floats and
// doubles, random inputs across many binades and directed ones.  The fallback keeps its branching
// form in the kernels (a division in every iteration costs more than the rare branch); its
// division (lo == 0, hi > 0) is reached here through both loops.  Prints "ok" and returns 0, or
// says what differs.  Never shipped.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "bb_solve.h"

using namespace bb;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}
static double rnd() { return double(rnd64() >> 11) / double(1ull << 52) - 1.0; }  // [-1, 1)
static int rndi(int n) { return int(rnd64() % uint64_t(n)); }
// +-(1 + u) 2^e, e uniform in [-span, span]
template <typename T>
static T binade(int span) {
  const double m = 1.0 + 0.5 * (rnd() + 1.0);
  return T((rnd() < 0 ? -m : m) * ldexp(1.0, rndi(2 * span + 1) - span));
}
template <typename T>
static bool same(T a, T b) { return memcmp(&a, &b, sizeof a) == 0; }
template <typename T>
static const char* name() { return sizeof(T) == 8 ? "double" : "float"; }

// ---- the parent's branching forms ----------------------------------------------------------
template <typename T>
static void ref_prep(LsTerm<T>& t, const T* j0, const T* x, T mu_, T f1, T f2, const T* D, T Dm_) {
  t.mu = mu_;
  t.Dm = Dm_;
  t.u0[0] = t.mu * j0[0]; t.u0[1] = f1 * j0[1]; t.u0[2] = f2 * j0[2];
  t.du[0] = t.mu * x[0]; t.du[1] = f1 * x[1]; t.du[2] = f2 * x[2];
  t.b0 = D[0] * j0[0] * x[0] + D[1] * j0[1] * x[1] + D[2] * j0[2] * x[2];
  t.b1 = D[0] * x[0] * x[0] + D[1] * x[1] * x[1] + D[2] * x[2] * x[2];
  t.c0 = T(0.5) * (D[0] * j0[0] * j0[0] + D[1] * j0[1] * j0[1] + D[2] * j0[2] * j0[2]);
  t.vv = t.du[1] * t.du[1] + t.du[2] * t.du[2];
  t.kink = T(-1);
  if (t.vv > 0) {
    const T ak = -(t.u0[1] * t.du[1] + t.u0[2] * t.du[2]) / t.vv;
    const T N = t.u0[0] + ak * t.du[0], U1 = t.u0[1] + ak * t.du[1], U2 = t.u0[2] + ak * t.du[2];
    const T Tn = sqrt(U1 * U1 + U2 * U2);
    if (ak > 0 && N < t.mu * Tn && t.mu * N + Tn > 0) t.kink = ak;
  }
}
template <typename T>
static bool ref_crosses(const LineSearch<T>& l, T k) {
  const bool between = l.alpha > l.prev ? (k > l.prev && k < l.alpha) : (k < l.prev && k > l.alpha);
  return between && k > l.lo && (l.hi < 0 || k < l.hi);
}
// one trip of the branching loop: 0 went on, 1 left converged (ls_ok), 2 left on a NaN
template <typename T>
static int ref_step(LineSearch<T>& l, T s1, T s2, T sm, T gs, T sMs, T d0, T tol, const T* kinks, int nk) {
  const T alpha = l.alpha;
  const T d1 = gs + alpha * sMs + s1;
  if (fabs(d1) <= tol * fabs(d0)) return 1;
  const T dmag = fabs(gs) + fabs(alpha * sMs) + sm;
  if (fabs(d1) <= T(32) * eps_of<T>() * dmag) return 1;
  if (!(d1 == d1)) return 2;
  const T d2 = sMs + s2;
  l.update(d1, d2);
  const bool up = l.alpha > l.prev;
  const T big = T(1e30);
  T kv = big;
  for (int c = 0; c < nk; c++) kv = fmin(kv, ref_crosses(l, kinks[c]) ? (up ? kinks[c] : -kinks[c]) : big);
  const T ks = up ? kv : -kv;
  l.dx = kv < big ? fabs(ks - l.prev) : l.dx;
  l.alpha = kv < big ? ks : l.alpha;
  return 0;
}
template <typename T>
static void new_step(LineSearch<T>& l, bool& ok, bool& done, T s1, T s2, T sm, T gs, T sMs, T d0, T tol, const T* kinks,
                     int nk) {
  ls_advance(l, ok, done, s1, s2, sm, gs, sMs, d0, tol, [&](const LineSearch<T>& n, bool up) {
    T kv = T(1e30);
    for (int c = 0; c < nk; c++) kv = fmin(kv, n.crosses_sel(kinks[c]) ? (up ? kinks[c] : -kinks[c]) : T(1e30));
    return kv;
  });
}

template <typename T>
static bool same_term(const LsTerm<T>& a, const LsTerm<T>& b) {
  bool s = same(a.mu, b.mu) && same(a.Dm, b.Dm) && same(a.b0, b.b0) && same(a.b1, b.b1) && same(a.vv, b.vv) &&
           same(a.kink, b.kink) && same(a.c0, b.c0);
  for (int r = 0; r < 3; r++) s = s && same(a.u0[r], b.u0[r]) && same(a.du[r], b.du[r]);
  return s;
}
template <typename T>
static bool same_state(const LineSearch<T>& a, const LineSearch<T>& b) {
  return same(a.lo, b.lo) && same(a.dlo, b.dlo) && same(a.hi, b.hi) && same(a.dhi, b.dhi) && same(a.alpha, b.alpha) &&
         same(a.flo, b.flo) && same(a.fhi, b.fhi) && same(a.prev, b.prev) && same(a.dx, b.dx) && same(a.dxold, b.dxold) &&
         a.side == b.side && a.same == b.same;
}
// what a finished search hands on: alpha, the bracket and so the fallback
template <typename T>
static bool same_result(const LineSearch<T>& a, const LineSearch<T>& b) {
  return same(a.lo, b.lo) && same(a.dlo, b.dlo) && same(a.hi, b.hi) && same(a.dhi, b.dhi) && same(a.alpha, b.alpha) &&
         same(a.fallback(), b.fallback());
}

// ---- prep against prep_sel -----------------------------------------------------------------
template <typename T>
static int check_prep(int trials) {
  const int span = sizeof(T) == 8 ? 40 : 12;
  const T nan = T(NAN);
  for (int t = 0; t < trials; t++) {
    T j0[3], x[3], D[3];
    for (int r = 0; r < 3; r++) { j0[r] = binade<T>(span); x[r] = binade<T>(span); D[r] = fabs(binade<T>(10)); }
    T mu = T(rndi(2) ? 1.0 : 0.7), f1 = mu, f2 = T(rndi(2) ? 1.0 : 0.001);
    switch (t % 16) {  // directed: no tangential motion (vv == 0), signed zeros, a kink at the origin, NaNs
      case 1: x[1] = x[2] = T(0); break;
      case 2: x[1] = T(-0.0); x[2] = T(0); break;
      case 3: x[1] = x[2] = T(-0.0); j0[1] = T(-0.0); break;
      case 4: j0[1] = j0[2] = T(0); break;               // ak == 0: not a kink
      case 5: j0[1] = T(-0.0); j0[2] = T(0); x[0] = T(0); break;
      case 6: x[2] = nan; break;                         // vv NaN
      case 7: j0[0] = nan; break;
      case 8: x[0] = x[1] = x[2] = T(0); D[0] = D[1] = D[2] = T(0); mu = f1 = f2 = T(0); j0[0] = j0[1] = j0[2] = T(0); break;
      case 9: x[1] = T(ldexp(1.0, sizeof(T) == 8 ? -600 : -80)); x[2] = T(0); break;  // vv underflows to 0
      default: break;
    }
    LsTerm<T> a, b;
    ref_prep(a, j0, x, mu, f1, f2, D, D[0] * T(0.5));
    b.prep_sel(j0, x, mu, f1, f2, D, D[0] * T(0.5));
    if (!same_term(a, b)) return printf("%s prep trial %d: kink %a against %a\n", name<T>(), t, double(b.kink), double(a.kink)), 1;
    LsTerm<T> c;
    c.prep(j0, x, mu, f1, f2, D, D[0] * T(0.5));
    if (!same_term(a, c)) return printf("%s prep trial %d: the header's prep differs from the copy here\n", name<T>(), t), 1;
  }
  return 0;
}

// ---- an idle lane's inert term against LsTerm::none -------------------------------------------
template <typename T>
static int check_inert() {
  const T z[3] = {T(0), T(0), T(0)};
  LsTerm<T> idle, none;
  idle.prep_sel(z, z, T(0), T(0), T(0), z, T(0) * T(0.5));
  none.none();
  if (!same(idle.kink, T(-1))) return printf("%s: the inert term has a kink\n", name<T>()), 1;
  const T alphas[] = {T(0), T(-0.0), T(1), T(0.37), T(1e-30), T(1e30), T(-2)};
  const T starts[] = {T(0), T(-0.0), T(3.25), T(-1e-30), T(1e20)};
  for (T al : alphas)
    for (T st : starts) {
      T a1 = st, a2 = st, a3 = st, b1 = st, b2 = st, b3 = st;
      idle.eval(al, a1, a2, a3);
      none.eval(al, b1, b2, b3);
      if (!same(a1, b1) || !same(a2, b2) || !same(a3, b3) || !same(a1, st + T(0)))
        return printf("%s: the inert term adds %a to %a at alpha %a\n", name<T>(), double(a1), double(st), double(al)), 1;
      T ca = st, cb = st;
      ca += idle.cost(al) - idle.cost(T(0));
      cb += none.cost(al) - none.cost(T(0));
      if (!same(ca, cb)) return printf("%s: the inert term's cost differs at alpha %a\n", name<T>(), double(al)), 1;
    }
  LineSearch<T> l;
  l.init(T(-1));
  if (l.crosses_sel(idle.kink)) return printf("%s: the inert kink is crossed from the start\n", name<T>()), 1;
  return 0;
}

// ---- crosses against crosses_sel, a kink exactly at prev, alpha, lo and hi ---------------------
template <typename T>
static int check_crosses(int trials) {
  const T nan = T(NAN);
  for (int t = 0; t < trials; t++) {
    LineSearch<T> l;
    l.init(T(-1));
    T v[4];
    for (int i = 0; i < 4; i++) v[i] = fabs(binade<T>(6));
    l.prev = v[0]; l.alpha = v[1]; l.lo = rndi(4) ? fmin(v[0], v[1]) * T(rndi(2) ? 1.0 : 0.5) : T(0);
    l.hi = rndi(3) ? fmax(v[0], v[1]) * T(rndi(2) ? 1.0 : 2.0) : T(-1);
    if (t % 7 == 0) l.prev = l.alpha;
    const T ks[] = {l.prev, l.alpha, l.lo, l.hi, v[2], v[3], T(0.5) * (l.prev + l.alpha), T(-1), T(0), T(-0.0), nan,
                    nextafter(l.prev, l.alpha), nextafter(l.alpha, l.prev)};
    for (T k : ks)
      if (ref_crosses(l, k) != l.crosses_sel(k) || l.crosses(k) != l.crosses_sel(k))
        return printf("%s crosses: k %a prev %a alpha %a lo %a hi %a\n", name<T>(), double(k), double(l.prev), double(l.alpha),
                      double(l.lo), double(l.hi)), 1;
  }
  return 0;
}

// ---- one evaluation, synthetic sums: every exit, d2 <= 0, hi < 0, kinks on the bracket ---------
template <typename T>
static int check_step(int trials) {
  const int span = sizeof(T) == 8 ? 30 : 10;
  const T nan = T(NAN), tol = T(0.01);
  for (int t = 0; t < trials; t++) {
    // a state some way into a search: a few reference trips from init on random sums
    const T d0 = -fabs(binade<T>(span));
    LineSearch<T> l;
    l.init(d0);
    T gs = d0 * T(0.5 + 0.25 * rnd()), sMs = fabs(binade<T>(span));
    const int pre = rndi(5);
    for (int i = 0; i < pre; i++) {
      const T none_k = T(-1);
      if (ref_step(l, binade<T>(span), binade<T>(span), fabs(binade<T>(span)), gs, sMs, d0, tol, &none_k, 1)) break;
    }
    T s1 = binade<T>(span), s2 = binade<T>(span), sm = fabs(binade<T>(span));
    T kinks[4] = {T(-1), fabs(binade<T>(4)), T(-1), fabs(binade<T>(4))};
    switch (t % 16) {
      case 1: s1 = -(gs + l.alpha * sMs); break;                        // d1 == +-0: tolerance and roundoff together
      case 2: s1 = -(gs + l.alpha * sMs); sm = T(0); gs = T(0); break;
      case 3: s1 = nan; break;                                          // d1 NaN
      case 4: s1 = nan; sm = nan; break;
      case 5: s2 = -sMs; break;                                         // d2 == 0: the 1e-30 floor
      case 6: s2 = -T(4) * sMs; break;                                  // d2 < 0
      case 7: sm = T(INFINITY); break;                                  // roundoff exit alone
      case 8: s1 = fabs(s1) + fabs(gs) + fabs(l.alpha * sMs); break;    // d1 > 0: sets hi
      case 9: s1 = -fabs(s1) - fabs(l.alpha * sMs); break;              // d1 < 0: hi may stay < 0
      case 11: s2 = nan; break;
      case 12: gs = T(-0.0); s1 = T(0); sMs = T(0); break;              // signed zeros through d1
      default: break;
    }
    LineSearch<T> a = l, b = l;
    bool ok = false, done = false;
    const int r = ref_step(a, s1, s2, sm, gs, sMs, d0, tol, kinks, 4);
    if (t % 16 == 10) {  // kinks exactly on the updated state's prev, alpha, lo and hi
      LineSearch<T> u = l;
      const T none_k = T(-1);
      if (!ref_step(u, s1, s2, sm, gs, sMs, d0, tol, &none_k, 1)) {
        kinks[0] = u.alpha; kinks[1] = u.lo; kinks[2] = u.hi; kinks[3] = u.prev;
        a = l;
        ref_step(a, s1, s2, sm, gs, sMs, d0, tol, kinks, 4);
      }
    }
    new_step(b, ok, done, s1, s2, sm, gs, sMs, d0, tol, kinks, 4);
    if (ok != (r == 1) || done != (r != 0))
      return printf("%s step trial %d: exit %d, ls_ok %d done %d\n", name<T>(), t, r, int(ok), int(done)), 1;
    if (r == 0 ? !same_state(a, b) : !same_result(a, b))
      return printf("%s step trial %d (exit %d): alpha %a against %a\n", name<T>(), t, r, double(b.alpha), double(a.alpha)), 1;
    // a finished search that runs on with its wave keeps its result, whatever it is fed
    if (r != 0) {
      const bool ok0 = ok;
      for (int i = 0; i < 3; i++) new_step(b, ok, done, i == 1 ? nan : binade<T>(span), binade<T>(span), fabs(binade<T>(span)), gs,
                                           sMs, d0, tol, kinks, 4);
      if (ok != ok0 || !done || !same_result(a, b)) return printf("%s step trial %d: a finished search moved\n", name<T>(), t), 1;
    }
  }
  return 0;
}

// ---- whole searches over real terms, idle lanes included --------------------------------------
template <typename T>
static int check_search(int trials, long* evals, long* fallbacks, long* snaps) {
  const T tol = T(0.01);
  for (int t = 0; t < trials; t++) {
    const int nc = 1 + rndi(16), lanes = 16;
    LsTerm<T> ra[16], nb[16];
    T kinks[16];
    const int span = t % 3 == 0 ? 8 : 2;
    for (int c = 0; c < lanes; c++) {
      T j0[3], x[3], D[3];
      const bool wheel = c < 3, act = c < nc;
      for (int r = 0; r < 3; r++) { j0[r] = binade<T>(span); x[r] = binade<T>(span); D[r] = fabs(binade<T>(3)); }
      if (t % 5 == 1) j0[0] = -fabs(j0[0]);                            // pressed in: bottom and middle zones
      if (t % 11 == 2 && c == 0) { x[1] = x[2] = T(0); }               // vv == 0
      if (t % 11 == 3 && c == 1) { j0[1] = j0[2] = x[1] = x[2] = T(0); }  // t2 == 0 at every alpha, N of either sign
      const T mu = wheel ? T(0.7) : T(1), f2 = wheel ? T(0.001) : T(1);
      if (act) {
        ref_prep(ra[c], j0, x, mu, mu, f2, D, D[0] * T(0.5));
        nb[c].prep_sel(j0, x, mu, mu, f2, D, D[0] * T(0.5));
      } else {  // the idle lanes: none() there, zeroed operands here
        const T z[3] = {T(0), T(0), T(0)};
        ra[c].none();
        nb[c].prep_sel(z, z, T(0), T(0), T(0), z, T(0));
      }
      kinks[c] = nb[c].kink;
      if (!same(ra[c].kink, nb[c].kink)) return printf("%s search %d: kink of term %d\n", name<T>(), t, c), 1;
      if (ra[c].kink > 0) ++*snaps;
    }
    const T sMs = fabs(binade<T>(span)), d0 = -fabs(binade<T>(span));
    const T gs = t % 7 == 4 ? T(-0.0) : d0 * T(0.5 + 0.4 * rnd());
    const int maxit = t % 13 == 5 ? 2 : 50;  // short searches end unconverged: the fallback
    // the branching loop
    LineSearch<T> a;
    a.init(d0);
    bool aok = false;
    int na = 0;
    for (int ls = 1; ls <= maxit; ls++) {
      T p1 = 0, p2 = 0, pm = 0;
      for (int c = 0; c < lanes; c++) ra[c].eval(a.alpha, p1, p2, pm);
      na++;
      const int r = ref_step(a, p1, p2, pm, gs, sMs, d0, tol, kinks, lanes);
      if (r == 1) aok = true;
      if (r) break;
    }
    if (!aok) { a.alpha = a.fallback(); ++*fallbacks; }
    *evals += na;
    // ls_advance: leaving on done (extra == 0), or running on for the wave's sake
    for (int extra = 0; extra <= 3; extra += 3) {
      LineSearch<T> b;
      b.init(d0);
      bool bok = false, done = false;
      int nbv = 0, after = 0;
      for (int ls = 1; ls <= maxit; ls++) {
        if (done && after++ >= extra) break;
        T p1 = 0, p2 = 0, pm = 0;
        for (int c = 0; c < lanes; c++) nb[c].eval(b.alpha, p1, p2, pm);
        if (!done) nbv++;
        new_step(b, bok, done, p1, p2, pm, gs, sMs, d0, tol, kinks, lanes);
      }
      if (!bok) b.alpha = b.fallback();
      if (bok != aok || nbv != na || !same(a.alpha, b.alpha))
        return printf("%s search %d (extra %d): ok %d/%d evaluations %d/%d alpha %a against %a\n", name<T>(), t, extra, int(bok),
                      int(aok), nbv, na, double(b.alpha), double(a.alpha)), 1;
    }
  }
  return 0;
}

// the fallback's division: lo == 0 with hi > 0 after an unconverged search, through both loops
template <typename T>
static int check_fallback_division() {
  const T d0 = T(-1), gs = T(-1), sMs = T(0.25), tol = T(1e-6), none_k = T(-1);
  LineSearch<T> a, b;
  a.init(d0);
  b.init(d0);
  bool ok = false, done = false;
  const T s1 = T(3);  // d1 = -1 + 0.25 + 3 > 0 at alpha = 1: hi = 1, lo stays 0
  const int r = ref_step(a, s1, T(0), T(0), gs, sMs, d0, tol, &none_k, 1);
  new_step(b, ok, done, s1, T(0), T(0), gs, sMs, d0, tol, &none_k, 1);
  if (r != 0 || done || !(a.lo == 0) || !(a.hi > 0)) return printf("%s fallback: the directed state was not reached\n", name<T>()), 1;
  const T want = a.hi * a.dlo / (a.dlo - a.dhi);
  if (!same(a.fallback(), want) || !same(b.fallback(), want)) return printf("%s fallback: %a\n", name<T>(), double(b.fallback())), 1;
  return 0;
}

template <typename T>
static int check_all() {
  long evals = 0, fallbacks = 0, snaps = 0;
  if (check_prep<T>(40000) || check_inert<T>() || check_crosses<T>(20000) || check_step<T>(40000) ||
      check_search<T>(6000, &evals, &fallbacks, &snaps) || check_fallback_division<T>())
    return 1;
  // the random searches must reach what they are there for
  if (evals < 2 * 6000 || fallbacks < 50 || snaps < 500)
    return printf("%s: the searches reached too little: %ld evaluations, %ld fallbacks, %ld kinks\n", name<T>(), evals, fallbacks,
                  snaps), 1;
  return 0;
}

int main() {
  if (check_all<double>() || check_all<float>()) return 1;
  printf("ok\n");
  return 0;
}
