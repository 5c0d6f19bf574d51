// Test-only host build: solve_team's carried jar and M a at solver exit, next to the same
// quantities recomputed from the final qacc (tests/test_host_solve_carry.py).  Never shipped.
#include <math.h>
#include "bb_model.h"
#include "bb_step.h"

using namespace bb;

// One fp64 forward at (q, v, ctrl) from the warm start acc (qacc out).  Returns the Newton
// iterations of the solve; out_n = {ng, iterations}.  Per contact row 3 c + r (c < 3 + ng):
// jar[0] carried, [1] J a - aref from the final a, [2] sum_k |J_rk| |a_k| + |aref_r|.  Per dof i:
// ma[0] carried (M a)_i, [1] recomputed, [2] sum_k |M_ik| |a_k|.
extern "C" int cc_solve_carry(const double* q, const double* v, const double* ctrl, double* acc, const float* hf,
                              double size_z, int* out_n, double (*jar)[3], double (*ma)[3]) {
  typedef double T;
  const ModelT<T> m = compile_model(default_solver(true));
  T warm[NV], a[NV];
  for (int i = 0; i < NV; i++) warm[i] = a[i] = acc[i];
  static EnvWork<T> W;
  StageOut<T> so;
  // the forward fills the workspace (contacts, poses, mass blocks, smooth force) and solves once
  const int it0 = forward(m, q, v, ctrl, a, TerrainRef<T>{hf, T(size_z), T(1e30)}, W, &so, Team{1, 0});
  // the same solve again from the same warm start, with the carry handed out
  for (int i = 0; i < NV; i++) a[i] = warm[i];
  SolveCarry<T> cy;
  const int it = solve_team(m, W, W.qfs, so.ng, a, Team{1, 0}, &cy);
  if (it != it0) return -1;
  out_n[0] = so.ng;
  out_n[1] = it;
  for (int c = 0; c < 3 + so.ng; c++)
    for (int r = 0; r < 3; r++) {
      T ref, mag;
      if (c < 3) {
        const WheelCon<T>& C = W.wc[c];
        ref = wheel_dot(C, c, r, a) - C.aref[r];
        mag = fabs(C.J[r][6]) * fabs(a[6 + c]) + fabs(C.aref[r]);
        for (int i = 0; i < 6; i++) mag += fabs(C.J[r][i]) * fabs(a[i]);
        for (int i = 7; i < 13; i++) mag += fabs(C.J[r][i]) * fabs(a[i + 2]);
      } else {
        T J[3][6], ar[3], D;
        ground_contact(m, W.g + (c - 3) * NGF, W.P.RB, W.vi, J, ar, D);
        ref = ground_dot(J, r, a) - ar[r];
        mag = fabs(ar[r]);
        for (int i = 0; i < 6; i++) mag += fabs(J[r][i]) * fabs(a[9 + i]);
      }
      jar[3 * c + r][0] = cy.jar[c][r];
      jar[3 * c + r][1] = ref;
      jar[3 * c + r][2] = mag;
    }
  T Ma[NV];
  mass_mul(W.M, a, Ma);
  for (int i = 0; i < NV; i++) {
    T mag = 0;
    for (int k = 0; k < NV; k++) mag += fabs(i >= k ? mass_entry(W.M, i, k) : mass_entry(W.M, k, i)) * fabs(a[k]);
    ma[i][0] = cy.Ma[i];
    ma[i][1] = Ma[i];
    ma[i][2] = mag;
  }
  for (int i = 0; i < NV; i++) acc[i] = a[i];
  return it;
}
