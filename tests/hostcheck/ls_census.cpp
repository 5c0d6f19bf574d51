// Test-only host library (tests/test_gpu_ls_select.py): one env step of the product's per-env
// templates (host path: a team of one lane, bb_solve.h:solve_team) built with BB_SOLVE_STATS,
// handing back what the step's line searches did, so that the test can pick states by it.
// Never shipped.
#include "bb_model.h"
#include "bb_step.h"

using namespace bb;

extern "C" {
// out[0..15]: converged searches by their number of evaluations (15: that many or more);
// out[16] evaluations, out[17] kink snaps, out[18] fallbacks, out[19] Newton iterations of the step
int lc_step(const EnvCfg* cfg, const double* q, const double* v, const double* w, const float* a, const float* hf,
            double size_z, long* out) {
  static const ModelT<double> m = compile_model(default_solver(true));
  static EnvWork<double> W;
  double qq[NQ], vv[NV], ww[NV];
  for (int i = 0; i < NQ; i++) qq[i] = q[i];
  for (int i = 0; i < NV; i++) { vv[i] = v[i]; ww[i] = w[i]; }
  long h0[16];
  for (int i = 0; i < 16; i++) h0[i] = g_ls_hist[i];
  const long e0 = g_ls_evals, s0 = g_ls_snaps, f0 = g_ls_fallbacks;
  float obs[15], rew = 0, p2[2];
  int it = 0, step = 0;
  const int fl = env_step(m, *cfg, qq, vv, ww, step, a, TerrainRef<double>{hf, size_z, 1e30}, W, obs, rew, p2, &it, Team{1, 0});
  for (int i = 0; i < 16; i++) out[i] = g_ls_hist[i] - h0[i];
  out[16] = g_ls_evals - e0;
  out[17] = g_ls_snaps - s0;
  out[18] = g_ls_fallbacks - f0;
  out[19] = it;
  return fl;
}
}
