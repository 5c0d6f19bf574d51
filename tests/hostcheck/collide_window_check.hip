// Test-only device program (tests/test_gpu_collide_window.py): t16::collide_team with and without
// the bound on its cell window (prism_window, bb_physics.h), as the step kernels run it: one 16-lane
// team per state, four teams per 64-lane workgroup, ng, overflow and the team's g[MAXG * NGF]
// copied out.  `zbound` holds one bound per team (the caller forms it in the precision under test,
// as forward forms TerrainRef::hz); bounded == 0 calls the signature without it.
//
// `rows` is a 4-bit mask of the live teams of every workgroup: lanes of the other rows return before
// the pass, the state of a wave whose other teams are elsewhere while this one ballots.
#include <hip/hip_runtime.h>

#include "bb_model.h"
#include "bb_team16.h"

using namespace bb;

constexpr int TL = 16;  // lanes per team (t16::L)

template <typename T>
__global__ __launch_bounds__(64) void window_kernel(ModelT<T> mg, const double* qpos, int nteam, const float* hf,
                                                    double size_z, const double* zbound, int bounded, int rows,
                                                    int* ng_out, int* ov_out, T* g_out) {
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
  const int ng = bounded ? t16::collide_team(m, k, (const T*)nullptr, hf, T(size_z), g[row], &overflow, tl,
                                             (const ModelOnce<T>*)nullptr, T(zbound[team]))
                         : t16::collide_team(m, k, (const T*)nullptr, hf, T(size_z), g[row], &overflow, tl);
  team_sync();  // the team's stores to g are visible to its lanes
  for (int i = tl; i < ng * NGF; i += TL) g_out[team * (MAXG * NGF) + i] = g[row][i];
  if (tl == 0) { ng_out[team] = ng; ov_out[team] = overflow; }
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

template <typename T>
int window_host(const double* qpos, int nteam, const float* hf, double size_z, const double* zbound, int bounded,
                int rows, int* ng, int* ov, T* g) {
  if (nteam <= 0) return 1;
  Buf q(qpos, sizeof(double) * NQ * nteam), h(hf, sizeof(float) * HF_N * HF_N), z(zbound, sizeof(double) * nteam),
      n(ng, sizeof(int) * nteam), o(ov, sizeof(int) * nteam), gg(g, sizeof(T) * MAXG * NGF * nteam);
  int rc = 1;
  if (q.d && h.d && z.d && n.d && o.d && gg.d) {
    const ModelT<T> m = cast_model<T>(compile_model(default_solver(sizeof(T) == 8)));
    window_kernel<T><<<(nteam + 3) / 4, 64>>>(m, (const double*)q.d, nteam, (const float*)h.d, size_z,
                                              (const double*)z.d, bounded, rows, (int*)n.d, (int*)o.d, (T*)gg.d);
    rc = hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess;
  }
  q.done(false); h.done(false); z.done(false); n.done(rc == 0); o.done(rc == 0); gg.done(rc == 0);
  return rc;
}

}  // namespace

extern "C" {

// sizes the caller allocates by: MAXG, NGF; and 1 when the build has the window (no -DBB_NO_PRISM_WINDOW)
void cw_sizes(int* out) { out[0] = MAXG; out[1] = NGF; out[2] = kPrismWindow ? 1 : 0; }

// qpos [nteam][NQ], hf [HF_N * HF_N], zbound [nteam]; ng, ov [nteam]; g [nteam][MAXG * NGF].  The outputs
// keep what the caller put there wherever a team did not run or a slot was not filled.  Returns 0 on success.
int cw_ground_f64(const double* qpos, int nteam, const float* hf, double size_z, const double* zbound, int bounded,
                  int rows, int* ng, int* ov, double* g) {
  return window_host<double>(qpos, nteam, hf, size_z, zbound, bounded, rows, ng, ov, g);
}
int cw_ground_f32(const double* qpos, int nteam, const float* hf, double size_z, const double* zbound, int bounded,
                  int rows, int* ng, int* ov, float* g) {
  return window_host<float>(qpos, nteam, hf, size_z, zbound, bounded, rows, ng, ov, g);
}

}  // extern "C"
