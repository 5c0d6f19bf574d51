// Test-only device program: the collision passes of bb_team16.h as the step kernels run them, one
// 16-lane team per state, four teams per 64-lane workgroup, with everything they produce copied out:
//   ground_kernel  kinematics + t16::collide_team: ng, overflow and the team's g[MAXG * NGF]
//   body_kernel    kinematics + t16::body_candidates (the team-uniform bool) + t16::collide_body_team
//                  with a CAND_CAP int scratch per team in LDS and a spill block in global memory:
//                  nb, overflow and the NBF fields of every contact, from bc and from the spill
// tests/test_gpu_collide.py compares them with tests/collide_ref.py, the host build and the oracle.
//
// `rows` is a 4-bit mask of the live teams of every workgroup: lanes of the other rows return before
// the pass, the state of a wave whose other teams are elsewhere while this one ballots.
#include <hip/hip_runtime.h>

#include "bb_bodycon.h"
#include "bb_model.h"
#include "bb_team16.h"

using namespace bb;

// bb::t16 exists in the device pass only: the kernels' bodies are compiled there alone
constexpr int TL = 16;                               // lanes per team (t16::L)
constexpr int SPILL = (MAXB - MAXB_LDS) * NBF;       // a team's spill block
constexpr int CAND = 80;                             // t16::CAND_CAP

template <typename T>
__global__ __launch_bounds__(64) void ground_kernel(ModelT<T> mg, const double* qpos, int nteam, const float* hf,
                                                    double size_z, int rows, int* ng_out, int* ov_out, T* g_out) {
#ifdef __HIP_DEVICE_COMPILE__
  __shared__ ModelT<T> ms;
  __shared__ T g[4][MAXG * NGF];
  if (threadIdx.x == 0) ms = mg;
  __syncthreads();
  const ModelT<T>& m = ms;
  const int lane = threadIdx.x, row = lane / TL, tl = lane % TL, team = blockIdx.x * 4 + row;
  if (team >= nteam || !((rows >> row) & 1)) return;
  T q[NQ];
  for (int i = 0; i < NQ; i++) q[i] = T(qpos[team * NQ + i]);
  Kin<T> k;
  kinematics(m, q, k);
  int overflow = 0;
  const int ng = t16::collide_team(m, k, (const T*)nullptr, hf, T(size_z), g[row], &overflow, tl);
  team_sync();  // the team's stores to g are visible to its lanes
  for (int i = tl; i < ng * NGF; i += TL) g_out[team * (MAXG * NGF) + i] = g[row][i];
  if (tl == 0) { ng_out[team] = ng; ov_out[team] = overflow; }
#endif
}

template <typename T>
__global__ __launch_bounds__(64) void body_kernel(ModelT<T> mg, const double* qpos, int nteam, const float* hf,
                                                  double size_z, double hz, int rows, int* cand_out, int* nb_out,
                                                  int* ov_out, T* bc_out, T* spill) {
#ifdef __HIP_DEVICE_COMPILE__
  static_assert(CAND == t16::CAND_CAP, "candidate scratch size");
  __shared__ ModelT<T> ms;
  __shared__ T bc[4][MAXB_LDS * NBF];
  __shared__ int cand[4][CAND];
  if (threadIdx.x == 0) ms = mg;
  __syncthreads();
  const ModelT<T>& m = ms;
  const int lane = threadIdx.x, row = lane / TL, tl = lane % TL, team = blockIdx.x * 4 + row;
  if (team >= nteam || !((rows >> row) & 1)) return;
  T q[NQ];
  for (int i = 0; i < NQ; i++) q[i] = T(qpos[team * NQ + i]);
  Kin<T> k;
  kinematics(m, q, k);
  const bool any = t16::body_candidates(m, k, hf, T(size_z), T(hz), tl);
  int overflow = 0;
  const int nb = t16::collide_body_team(m, k, hf, T(size_z), T(hz), bc[row], spill + size_t(team) * SPILL, &overflow,
                                        tl, cand[row]);
  team_sync();  // the team's stores to bc are visible to its lanes
  const int nl = nb < MAXB_LDS ? nb : MAXB_LDS;  // the rest is in the spill block, which the host reads
  for (int i = tl; i < nl * NBF; i += TL) bc_out[team * (MAXB_LDS * NBF) + i] = bc[row][i];
  if (tl == 0) { cand_out[team] = any ? 1 : 0; nb_out[team] = nb; ov_out[team] = overflow; }
#endif
}

namespace {

struct Buf {  // a device copy of a host array, copied back and freed by done()
  void* d = nullptr;
  void* h;
  size_t bytes;
  Buf(const void* host, size_t n) : h(const_cast<void*>(host)), bytes(n) {
    if (hipMalloc(&d, n ? n : 1) != hipSuccess) d = nullptr;
    else (void)hipMemcpy(d, h, n, hipMemcpyHostToDevice);
  }
  void done(bool back) {
    if (d && back) (void)hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost);
    if (d) (void)hipFree(d);
  }
};

int finish() {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipGetLastError() != hipSuccess;
}

template <typename T>
ModelT<T> model_for() {
  const bool fp64 = sizeof(T) == 8;
  return cast_model<T>(compile_model(default_solver(fp64)));
}

template <typename T>
int ground_host(const double* qpos, int nteam, const float* hf, double size_z, int rows, int* ng, int* ov, T* g) {
  Buf q(qpos, sizeof(double) * NQ * nteam), h(hf, sizeof(float) * HF_N * HF_N), n(ng, sizeof(int) * nteam),
      o(ov, sizeof(int) * nteam), gg(g, sizeof(T) * MAXG * NGF * nteam);
  int rc = 1;
  if (q.d && h.d && n.d && o.d && gg.d) {
    ground_kernel<T><<<(nteam + 3) / 4, 64>>>(model_for<T>(), (const double*)q.d, nteam, (const float*)h.d, size_z,
                                              rows, (int*)n.d, (int*)o.d, (T*)gg.d);
    rc = finish();
  }
  q.done(false); h.done(false); n.done(rc == 0); o.done(rc == 0); gg.done(rc == 0);
  return rc;
}

template <typename T>
int body_host(const double* qpos, int nteam, const float* hf, double size_z, double hz, int rows, int* cand, int* nb,
              int* ov, T* bc, T* spill) {
  Buf q(qpos, sizeof(double) * NQ * nteam), h(hf, sizeof(float) * HF_N * HF_N), c(cand, sizeof(int) * nteam),
      n(nb, sizeof(int) * nteam), o(ov, sizeof(int) * nteam), b(bc, sizeof(T) * MAXB_LDS * NBF * nteam),
      s(spill, sizeof(T) * SPILL * nteam);
  int rc = 1;
  if (q.d && h.d && c.d && n.d && o.d && b.d && s.d) {
    body_kernel<T><<<(nteam + 3) / 4, 64>>>(model_for<T>(), (const double*)q.d, nteam, (const float*)h.d, size_z, hz,
                                            rows, (int*)c.d, (int*)n.d, (int*)o.d, (T*)b.d, (T*)s.d);
    rc = finish();
  }
  q.done(false); h.done(false); c.done(rc == 0); n.done(rc == 0); o.done(rc == 0); b.done(rc == 0); s.done(rc == 0);
  return rc;
}

}  // namespace

extern "C" {

// sizes the caller allocates by: MAXG, NGF, MAXB, MAXB_LDS, NBF
void cc_sizes(int* out) { out[0] = MAXG; out[1] = NGF; out[2] = MAXB; out[3] = MAXB_LDS; out[4] = NBF; }

// qpos [nteam][NQ], hf [HF_N * HF_N]; ng, ov [nteam]; g [nteam][MAXG * NGF].  The outputs keep what the
// caller put there wherever a team did not run or a slot was not filled.  Returns 0 on success.
int cc_ground_f64(const double* qpos, int nteam, const float* hf, double size_z, int rows, int* ng, int* ov,
                  double* g) {
  return ground_host<double>(qpos, nteam, hf, size_z, rows, ng, ov, g);
}
int cc_ground_f32(const double* qpos, int nteam, const float* hf, double size_z, int rows, int* ng, int* ov, float* g) {
  return ground_host<float>(qpos, nteam, hf, size_z, rows, ng, ov, g);
}

// hz: the terrain's top (max height x size_z); cand, nb, ov [nteam]; bc [nteam][MAXB_LDS * NBF] (the LDS
// slots); spill [nteam][(MAXB - MAXB_LDS) * NBF] (the rest, as the pass left it in global memory)
int cc_body_f64(const double* qpos, int nteam, const float* hf, double size_z, double hz, int rows, int* cand,
                int* nb, int* ov, double* bc, double* spill) {
  return body_host<double>(qpos, nteam, hf, size_z, hz, rows, cand, nb, ov, bc, spill);
}
int cc_body_f32(const double* qpos, int nteam, const float* hf, double size_z, double hz, int rows, int* cand, int* nb,
                int* ov, float* bc, float* spill) {
  return body_host<float>(qpos, nteam, hf, size_z, hz, rows, cand, nb, ov, bc, spill);
}

}  // extern "C"
