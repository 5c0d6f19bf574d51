// Test-only program: the four base-tree contact primitives of bb_bodycon.h, one case per lane.
//   KIND 0 capsule_prism   1 cylinder_prism      in[n][18]: top triangle 9, bottom z, c 3, a 3, hh, r
//   KIND 2 sphere_cylinder 3 sphere_capsule      in[n][12]: sphere centre 3, sphere r, c 3, a 3, hh, r
// The inputs are doubles cast to T (the fp32 callers pass values a float holds exactly).  On a hit
// the lane writes hit[i] = 1 and out[i][7] = dist, n[3], pos[3]; on a miss it writes hit[i] = 0 and
// leaves out[i] as the caller filled it; the caller's buffers hold 64 more rows, which stay as they
// are.  The device entries launch 64-lane workgroups, so the primitives run under the partial exec
// masks the cases' routes make of a wave -- the state in which capsule_prism calls
// capsule_prism_apart_call; the host entries run the same templates in a plain loop.
// tests/bodycon_check.py compares both with tests/bodycon_ref.py.
#include <hip/hip_runtime.h>

#include "bb_bodycon.h"

using namespace bb;

namespace {

constexpr int NIN_PRISM = 18, NIN_SPHERE = 12, NOUT = 7, PAD = 64;

template <typename T, int KIND>
BB_HD void one_case(const double* in, int* hit, T* out) {
  T dist = 0, n[3] = {0, 0, 0}, pos[3] = {0, 0, 0};
  bool h;
  Seg<T> g;
  if (KIND <= 1) {
    const T Tp[3][3] = {{T(in[0]), T(in[1]), T(in[2])}, {T(in[3]), T(in[4]), T(in[5])}, {T(in[6]), T(in[7]), T(in[8])}};
    PrismG<T> P;
    prism_build(P, Tp, T(in[9]));
    for (int i = 0; i < 3; i++) { g.c[i] = T(in[10 + i]); g.a[i] = T(in[13 + i]); }
    g.hh = T(in[16]); g.r = T(in[17]);
    h = KIND == 0 ? capsule_prism(g, P, dist, n, pos) : cylinder_prism(g, P, dist, n, pos);
  } else {
    const T c[3] = {T(in[0]), T(in[1]), T(in[2])};
    for (int i = 0; i < 3; i++) { g.c[i] = T(in[4 + i]); g.a[i] = T(in[7 + i]); }
    g.hh = T(in[10]); g.r = T(in[11]);
    h = KIND == 2 ? sphere_cylinder(c, T(in[3]), g, dist, n, pos) : sphere_capsule(c, T(in[3]), g, dist, n, pos);
  }
  *hit = h ? 1 : 0;
  if (h) {
    out[0] = dist;
    for (int i = 0; i < 3; i++) { out[1 + i] = n[i]; out[4 + i] = pos[i]; }
  }
}

template <typename T, int KIND>
__global__ __launch_bounds__(64) void case_kernel(const double* in, int n, int* hit, T* out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  one_case<T, KIND>(in + size_t(i) * (KIND <= 1 ? NIN_PRISM : NIN_SPHERE), hit + i, out + size_t(i) * NOUT);
}

template <typename T, int KIND>
int run_device(const double* in, int n, int* hit, T* out) {
  if (n <= 0) return 0;
  // hit and out hold PAD rows past n, on the device too: a lane past n that wrote would show there
  const size_t bi = sizeof(double) * size_t(n) * (KIND <= 1 ? NIN_PRISM : NIN_SPHERE),
               bh = sizeof(int) * size_t(n + PAD), bo = sizeof(T) * size_t(n + PAD) * NOUT;
  void *di = nullptr, *dh = nullptr, *dout = nullptr;
  int rc = 1;
  if (hipMalloc(&di, bi) == hipSuccess && hipMalloc(&dh, bh) == hipSuccess && hipMalloc(&dout, bo) == hipSuccess &&
      hipMemcpy(di, in, bi, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dh, hit, bh, hipMemcpyHostToDevice) == hipSuccess &&
      hipMemcpy(dout, out, bo, hipMemcpyHostToDevice) == hipSuccess) {
    case_kernel<T, KIND><<<(n + 63) / 64, 64>>>((const double*)di, n, (int*)dh, (T*)dout);
    rc = hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess;
    if (rc == 0)
      rc = hipMemcpy(hit, dh, bh, hipMemcpyDeviceToHost) != hipSuccess ||
           hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost) != hipSuccess;
  }
  if (di) (void)hipFree(di);
  if (dh) (void)hipFree(dh);
  if (dout) (void)hipFree(dout);
  return rc;
}

template <typename T, int KIND>
int run_host(const double* in, int n, int* hit, T* out) {
  for (int i = 0; i < n; i++)
    one_case<T, KIND>(in + size_t(i) * (KIND <= 1 ? NIN_PRISM : NIN_SPHERE), hit + i, out + size_t(i) * NOUT);
  return 0;
}

template <typename T>
int run(int kind, int device, const double* in, int n, int* hit, T* out) {
  switch (kind * 2 + (device ? 1 : 0)) {
    case 0: return run_host<T, 0>(in, n, hit, out);
    case 1: return run_device<T, 0>(in, n, hit, out);
    case 2: return run_host<T, 1>(in, n, hit, out);
    case 3: return run_device<T, 1>(in, n, hit, out);
    case 4: return run_host<T, 2>(in, n, hit, out);
    case 5: return run_device<T, 2>(in, n, hit, out);
    case 6: return run_host<T, 3>(in, n, hit, out);
    case 7: return run_device<T, 3>(in, n, hit, out);
  }
  return 2;
}

}  // namespace

extern "C" {

// kind: 0 capsule_prism, 1 cylinder_prism, 2 sphere_cylinder, 3 sphere_capsule; device: 0 the host
// build of the templates, 1 the gfx950 kernel.  in [n][18 or 12], hit [n + 64], out [n + 64][7]: the
// 64 rows past n are copied to the device and back, and no lane may write them.  Returns 0 on success.
int bc_run_f64(int kind, int device, const double* in, int n, int* hit, double* out) {
  return run<double>(kind, device, in, n, hit, out);
}
int bc_run_f32(int kind, int device, const double* in, int n, int* hit, float* out) {
  return run<float>(kind, device, in, n, hit, out);
}

}  // extern "C"
