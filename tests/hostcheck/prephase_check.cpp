// Test-only host program (tests/test_host_prephase.py): the forward's twin forms and once-per-launch
// model terms (bb_physics.h) against the serial forms, bit for bit, in float and double.
//   * integrate_pos_lin + one integrate_quat_half per half   vs  integrate_pos
//   * kinematics_half for both halves                        vs  kinematics_base (and the stage
//     out's qnormalize of the base quaternion)
//   * bias_finish_half for both halves                       vs  bias_finish / bias_forces
//   * every field of ModelOnce vs the expression the forward held in place before (copied here),
//     and kinematics_wheel / mass_finish / bias_wheel / bias_finish / wheel_contact handed a
//     ModelOnce vs the same calls without one
// on seeded random states plus: zero and 1e-300 angular velocity (quat_integrate's other branch), a
// denormal, unnormalised quaternions, a negative w, a NaN state (which must also form no cell index
// in the ground collision) and velocities at +-1e10 (vec_bad's boundary).  Two NaNs count as equal
// whatever their payloads.  Prints "ok" and returns 0, or says what differs.  Never shipped.
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
static int differ(const char* what, int cs, const T* a, const T* b, int n) {
  for (int i = 0; i < n; i++)
    if (!same(a[i], b[i])) {
      printf("%s (%s), case %d, entry %d: %.17g vs %.17g\n", what, sizeof(T) == 8 ? "double" : "float", cs, i,
             double(a[i]), double(b[i]));
      return 1;
    }
  return 0;
}

template <typename T>
struct State {
  T q[NQ], v[NV];
};

template <typename T>
static std::vector<State<T>> states(const ModelT<T>& m) {
  std::vector<State<T>> out;
  auto base = [&](double qs, double vs) {
    State<T> s;
    for (int i = 0; i < NQ; i++) s.q[i] = m.qpos0[i] + T(0.3 * rnd());
    for (int i = 0; i < 4; i++) { s.q[3 + i] = T(qs * rnd()); s.q[13 + i] = T(qs * rnd()); }  // unnormalised
    for (int i = 0; i < NV; i++) s.v[i] = T(vs * rnd());
    return s;
  };
  for (int i = 0; i < 200; i++) out.push_back(base(i % 3 == 0 ? 2.0 : 1.0, i % 5 == 0 ? 30.0 : 1.0));
  State<T> s = base(1, 1);  // zero angular velocity: base, ball, both
  s.v[3] = s.v[4] = s.v[5] = 0; out.push_back(s);
  s.v[12] = s.v[13] = s.v[14] = 0; out.push_back(s);
  s = base(1, 1); s.v[12] = s.v[13] = s.v[14] = 0; out.push_back(s);
  s = base(1, 1);  // below quat_integrate's 1e-15 threshold
  for (int i = 0; i < 3; i++) { s.v[3 + i] = T(1e-300); s.v[12 + i] = T(-1e-30); }
  out.push_back(s);
  s = base(1, 1); s.v[3] = T(1e-300); s.v[4] = s.v[5] = 0; s.v[12] = T(3e-16); s.v[13] = s.v[14] = 0; out.push_back(s);
  const T den = sizeof(T) == 8 ? T(5e-324) : T(1.4e-45);
  s = base(1, 1); s.q[4] = den; s.q[14] = -den; s.v[3] = den; s.v[13] = den; s.v[0] = den; out.push_back(s);
  s = base(1, 1);  // quaternions of norm below qnormalize's 1e-15
  for (int i = 0; i < 4; i++) { s.q[3 + i] = den; s.q[13 + i] = T(1e-17); }
  out.push_back(s);
  s = base(7.5, 1); s.q[3] = T(-3.2); s.q[13] = T(-0.4); out.push_back(s);  // negative w, far from unit
  s = base(1, 1); s.q[3] = T(-1); s.q[4] = s.q[5] = s.q[6] = 0; out.push_back(s);
  s = base(1, 1); s.q[3] = T(NAN); out.push_back(s);  // NaN states
  s = base(1, 1); s.q[10] = T(NAN); s.q[15] = T(NAN); out.push_back(s);
  s = base(1, 1); s.v[4] = T(NAN); s.v[9] = T(NAN); out.push_back(s);
  s = base(1, 1); for (int i = 0; i < NQ; i++) s.q[i] = T(NAN); out.push_back(s);
  for (int sg = -1; sg <= 1; sg += 2) {  // vec_bad's boundary
    s = base(1, 1); for (int i = 0; i < NV; i++) s.v[i] = T(sg * 1e10); out.push_back(s);
    s = base(1, 1); s.v[3] = T(sg * 1e10); s.v[14] = T(-sg * 1e10); s.v[9] = T(sg * 1e10); out.push_back(s);
    s = base(1, 1); s.v[5] = T(sg * 1.0000001e10); s.v[12] = T(sg * 0.9999999e10); out.push_back(s);
  }
  return out;
}

template <typename T>
static int check_pos(const ModelT<T>& m, const std::vector<State<T>>& S) {
  const T hs[3] = {m.h, m.h * T(0.5), T(1)};
  for (size_t c = 0; c < S.size(); c++)
    for (int hk = 0; hk < 3; hk++) {
      const T h = hs[hk];
      T qs[NQ], qt[NQ];
      for (int i = 0; i < NQ; i++) { qs[i] = S[c].q[i]; qt[i] = S[c].q[i]; }
      integrate_pos(qs, S[c].v, h);
      integrate_pos_lin(qt, S[c].v, h);
      for (int hi = 0; hi < 2; hi++) {
        T qh[4];
        integrate_quat_half(S[c].q + half_quat(hi), S[c].v + half_vang(hi), h, qh);
        for (int i = 0; i < 4; i++) qt[half_quat(hi) + i] = qh[i];
      }
      if (differ("integrate_pos", int(c), qt, qs, NQ)) return 1;
    }
  return 0;
}

template <typename T>
static int check_kin(const ModelT<T>& m, const std::vector<State<T>>& S) {
  for (size_t c = 0; c < S.size(); c++) {
    Kin<T> k1, k2;
    memset(&k1, 0, sizeof k1);
    memset(&k2, 0, sizeof k2);
    kinematics_base(m, S[c].q, k1);
    T qn[2][4];
    kinematics_half(m, S[c].q, false, k2, qn[0]);
    kinematics_half(m, S[c].q, true, k2, qn[1]);
    if (differ("Rb", int(c), k2.Rb, k1.Rb, 9) || differ("RB", int(c), k2.RB, k1.RB, 9) ||
        differ("pb", int(c), k2.pb, k1.pb, 3) || differ("pB", int(c), k2.pB, k1.pB, 3) ||
        differ("c", int(c), k2.c, k1.c, 3))
      return 1;
    T qb[4] = {S[c].q[3], S[c].q[4], S[c].q[5], S[c].q[6]};  // the stage out (bb_step.h: forward)
    qnormalize(qb);
    if (differ("quat_b", int(c), qn[0], qb, 4)) return 1;
  }
  return 0;
}

template <typename T>
static int check_bias_and_once(const ModelT<T>& m, const std::vector<State<T>>& S) {
  ModelOnce<T> o;
  model_once(m, o);
  for (size_t c = 0; c < S.size(); c++) {
    const T* q = S[c].q;
    const T* v = S[c].v;
    Kin<T> k, ko;
    memset(&k, 0, sizeof k);
    memset(&ko, 0, sizeof ko);
    kinematics(m, q, k);
    kinematics_base(m, q, ko);
    for (int w = 0; w < 3; w++) kinematics_wheel(m, q, w, ko, &o);
    if (differ("kinematics_wheel wc", int(c), &ko.wc[0][0], &k.wc[0][0], 9) ||
        differ("kinematics_wheel Rw", int(c), &ko.Rw[0][0], &k.Rw[0][0], 27))
      return 1;
    // mass: the serial build against mass_finish with the staged terms
    Mass<T> M, Mo;
    memset(&M, 0, sizeof M);
    memset(&Mo, 0, sizeof Mo);
    T Iw[3][6], Iwo[3][6], mrw[3][3], IOw[3][6];
    build_mass(m, k, M, Iw);
    for (int w = 0; w < 3; w++) mass_wheel(m, k, w, Mo, Iwo[w], mrw[w], IOw[w]);
    mass_finish(m, k, Mo, mrw, IOw, &o);
    if (differ("mass", int(c), reinterpret_cast<const T*>(&Mo), reinterpret_cast<const T*>(&M), int(sizeof M / sizeof(T))))
      return 1;
    // bias: serial, serial with the staged terms, the halves with and without them
    T bias[NV], w0[3], vl[3], a0[3], fw[3][6], fwo[3][6], hinge[3], hingeo[3];
    bias_forces(m, k, Iw, v, bias);
    bias_base_motion(m, k, v, w0, vl, a0);
    for (int w = 0; w < 3; w++) {
      hinge[w] = bias_wheel(m, k, Iw[w], v, w, w0, vl, a0, fw[w], fw[w] + 3);
      hingeo[w] = bias_wheel(m, k, Iw[w], v, w, w0, vl, a0, fwo[w], fwo[w] + 3, &o);
    }
    if (differ("bias_wheel", int(c), hingeo, hinge, 3) || differ("bias_wheel f", int(c), &fwo[0][0], &fw[0][0], 18) ||
        differ("bias hinge", int(c), hinge, bias + 6, 3))
      return 1;
    T bo[NV];
    for (int i = 0; i < NV; i++) bo[i] = bias[i];
    bias_finish(m, k, v, fw, bo, &o);
    if (differ("bias_finish(once)", int(c), bo, bias, NV)) return 1;
    for (int withonce = 0; withonce < 2; withonce++) {
      T bt[NV];
      for (int i = 0; i < NV; i++) bt[i] = bias[i];
      bias_finish_half(m, k, v, fw, false, bt, withonce ? &o : nullptr);
      bias_finish_half(m, k, v, fw, true, bt + 9, withonce ? &o : nullptr);
      if (differ(withonce ? "bias_finish_half(once)" : "bias_finish_half", int(c), bt, bias, NV)) return 1;
    }
    // ball-wheel contacts
    for (int w = 0; w < 3; w++) {
      WheelCon<T> C0, C1;
      memset(&C0, 0, sizeof C0);
      memset(&C1, 0, sizeof C1);
      wheel_contact(m, k, v, w, C0);
      wheel_contact(m, k, v, w, C1, &o);
      if (differ("wheel_contact", int(c), reinterpret_cast<const T*>(&C1), reinterpret_cast<const T*>(&C0),
                 int(sizeof C0 / sizeof(T))))
        return 1;
    }
  }
  // the fields against the expressions the forward held in place
  {
    T c0[3] = {m.h0[0] / m.m0, m.h0[1] / m.m0, m.h0[2] / m.m0};
    T cc = dot3(c0, c0);
    T Ic[6] = {m.I0O[0] - m.m0 * (cc - c0[0] * c0[0]), m.I0O[1] - m.m0 * (cc - c0[1] * c0[1]),
               m.I0O[2] - m.m0 * (cc - c0[2] * c0[2]), m.I0O[3] + m.m0 * c0[0] * c0[1],
               m.I0O[4] + m.m0 * c0[0] * c0[2], m.I0O[5] + m.m0 * c0[1] * c0[2]};
    T cB[3] = {0, 0, m.dz};
    T IcB[6] = {m.IB, m.IB, m.IB, 0, 0, 0};
    if (differ("once c0", 0, o.bc[0], c0, 3) || differ("once Ic", 0, o.bI[0], Ic, 6) ||
        differ("once cB", 0, o.bc[1], cB, 3) || differ("once IcB", 0, o.bI[1], IcB, 6))
      return 1;
    const T bm[2] = {m.m0, m.mB};
    if (differ("once bm", 0, o.bm, bm, 2)) return 1;
    for (int w = 0; w < 3; w++) {
      T au[3];
      cross3(au, m.anchor, m.u[w]);
      if (differ("once au", w, o.au[w], au, 3)) return 1;
    }
    T d[3] = {m.cw[0] - m.jpos[0], m.cw[1] - m.jpos[1], m.cw[2] - m.jpos[2]};
    if (differ("once dcj", 0, o.dcj, d, 3)) return 1;
    const T dz = m.dz;
    const T ms[4] = {m.m0 + 3 * m.mw, m.mB * dz, m.IB + m.mB * dz * dz, m.IB};
    const T os[4] = {o.mt, o.sbd, o.MBrr[0], o.MBrr[1]};
    if (differ("once mass terms", 0, os, ms, 4)) return 1;
    const T nsb = -m.mB * dz, onsb = -o.sbd;
    if (differ("once -mB dz", 0, &onsb, &nsb, 1)) return 1;
    const T muw = m.fr_wheel[0];
    const T kdw = T(1) / (muw * muw * (1 + muw * muw));
    const T rr = m.fr_wheel[0] / m.fr_wheel[1];
    const T sx = m.hf_sx, sy = m.hf_sy;
    const int N1 = HF_N - 1;
    const T dx = 2 * sx / N1, dy = 2 * sy / N1;
    const T es[4] = {kdw, rr, dx, dy}, eo[4] = {o.kdw, o.rr, o.dx, o.dy};
    if (differ("once kdw rr dx dy", 0, eo, es, 4)) return 1;
  }
  return 0;
}

// a NaN pose forms no cell index: no contact, and no height is read outside the field
template <typename T>
static int check_nan_collision(const ModelT<T>& m) {
  static float hf[HF_N * HF_N];  // flat
  const int bad[4] = {10, 11, 12, 15};  // ball position and one quaternion entry
  for (int b = 0; b < 4; b++)
    for (int twin = 0; twin < 2; twin++) {
      T q[NQ], v[NV] = {0}, g[MAXG * NGF];
      for (int i = 0; i < NQ; i++) q[i] = m.qpos0[i];
      q[bad[b]] = T(NAN);
      Kin<T> k;
      memset(&k, 0, sizeof k);
      T qn[4];
      if (twin) { kinematics_half(m, q, false, k, qn); kinematics_half(m, q, true, k, qn); }
      else kinematics_base(m, q, k);
      int overflow = 0;
      const int ng = collide_ground(m, k, v, hf, T(1), GStore<T>{g, 1}, &overflow);
      if (ng != 0 || overflow) return printf("NaN qpos[%d]: %d ground contacts\n", bad[b], ng), 1;
    }
  return 0;
}

template <typename T>
static int run() {
  const ModelT<T> m = cast_model<T>(compile_model(default_solver(sizeof(T) == 8)));
  const std::vector<State<T>> S = states(m);
  return check_pos(m, S) || check_kin(m, S) || check_bias_and_once(m, S) || check_nan_collision(m);
}

int main() {
  if (run<double>() || run<float>()) return 1;
  printf("ok\n");
  return 0;
}
