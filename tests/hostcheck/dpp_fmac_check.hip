// Test-only device program: the fused broadcast-FMA of bb_team16.h (fmac_bcast / fnmac_bcast) beside
// the plain move + FMA it replaces, and the register-row Cholesky and its two sweeps, on one
// workgroup of 64 lanes (four teams).  tests/test_gpu_dpp_fmac.py builds this file twice, with and
// without -DBB_NO_FMAC_DPP, and compares the two builds' outputs bit for bit.
//
// `rows` is a 4-bit mask of the live teams: lanes of the other rows return before any DPP
// instruction, the state of a wave whose teams left the Newton loop at different iterations.
#include <hip/hip_runtime.h>

#include "bb_team16.h"

using namespace bb;

// bb::t16 exists in the device pass only: the kernels' bodies are compiled there alone
constexpr int TL = 16;  // lanes per team (t16::L)

// out[(2 J + neg) * 64 + lane] for J = 0..15: acc (+|-)= bcast<J>(x) * own.
//   FUSED   fmac_bcast / fnmac_bcast        else   fma(+-bcast<J>(x), own, acc)
//   HAZARD  x is written by the VALU instruction right before each use: every x is a product
//           that depends on the previous result, so nothing can be scheduled between the two
template <bool FUSED, bool HAZARD>
__global__ void prim_kernel(const double* acc0, const double* x0, const double* own0, int rows, double* out) {
#ifdef __HIP_DEVICE_COMPILE__
  using namespace bb::t16;
  const int lane = threadIdx.x;
  if (!((rows >> (lane / TL)) & 1)) return;
  const double acc = acc0[lane], own = own0[lane];
  double x = x0[lane], prev = 1.0;
  static_for<2 * TL>([&](auto ic) {
    constexpr int J = decltype(ic)::value / 2;
    constexpr bool neg = decltype(ic)::value % 2;
    double xv = x;
    if constexpr (HAZARD) {
      // a finite, lane-dependent factor from the previous result (its low mantissa bits)
      const double f = 1.0 + double(__double_as_longlong(prev) & 0xFF) * 0.00390625;
      xv = x * f;
      x = xv;
    }
    double r = acc;
    if constexpr (FUSED) {
      if constexpr (neg) fnmac_bcast<J>(r, xv, own); else fmac_bcast<J>(r, xv, own);
    } else {
      r = neg ? fma(-bcast<J>(xv), own, r) : fma(bcast<J>(xv), own, r);
    }
    prev = r;
    out[decltype(ic)::value * 64 + lane] = r;
  });
#endif
}

// H: 4 x NV x NV (row-major, one SPD matrix per team), g: 4 x NV.  Lane tl of team t holds row
// min(tl, NV - 1), as in solve16.  Outputs per lane: the factor's row (NV), diag (NV), s (NV), sown.
template <typename T>
__global__ void solve_kernel(const T* H, const T* g, int rows, T* out) {
#ifdef __HIP_DEVICE_COMPILE__
  using namespace bb::t16;
  __shared__ T scr[4][NV * (NV - 1) / 2];
  const int lane = threadIdx.x, team = lane / TL, tl = lane % TL;
  if (!((rows >> team) & 1)) return;
  const int row = tl < NV ? tl : NV - 1;
  T h[NV], diag[NV], s[NV], sown;
#pragma unroll
  for (int k = 0; k < NV; k++) h[k] = H[(team * NV + row) * NV + k];
  T hdi = 0;
#pragma unroll
  for (int k = 0; k < NV; k++) hdi = row == k ? h[k] : hdi;
  const T gi = tl < NV ? g[team * NV + row] : T(0);
  chol_rows<true>(h, hdi, diag, tl);  // FUSE: the fused forms, unless -DBB_NO_FMAC_DPP
  chol_solve_rows<true>(h, diag, gi, s, sown, tl, scr[team]);
  T* o = out + lane * (3 * NV + 1);
#pragma unroll
  for (int k = 0; k < NV; k++) {
    o[k] = k < row ? h[k] : T(0);  // the strictly lower part: the rest of the row is never read
    o[NV + k] = diag[k];
    o[2 * NV + k] = s[k];
  }
  o[3 * NV] = sown;
#endif
}

static int finish() {
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  return hipGetLastError() != hipSuccess;
}

template <typename T>
static int solve_host(const T* H, const T* g, int rows, T* out) {
  T *d_H, *d_g, *d_out;
  const size_t nH = 4 * NV * NV, ng = 4 * NV, nout = 64 * (3 * NV + 1);
  if (hipMalloc(&d_H, nH * sizeof(T)) != hipSuccess) return 1;
  if (hipMalloc(&d_g, ng * sizeof(T)) != hipSuccess) return 1;
  if (hipMalloc(&d_out, nout * sizeof(T)) != hipSuccess) return 1;
  (void)hipMemcpy(d_H, H, nH * sizeof(T), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_g, g, ng * sizeof(T), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_out, out, nout * sizeof(T), hipMemcpyHostToDevice);
  solve_kernel<T><<<1, 64>>>(d_H, d_g, rows, d_out);
  int rc = finish();
  (void)hipMemcpy(out, d_out, nout * sizeof(T), hipMemcpyDeviceToHost);
  (void)hipFree(d_H);
  (void)hipFree(d_g);
  (void)hipFree(d_out);
  return rc;
}

extern "C" {

// 1 when this build fuses (no -DBB_NO_FMAC_DPP)
int dc_fused_build() {
#ifdef BB_NO_FMAC_DPP
  return 0;
#else
  return 1;
#endif
}

// host arrays: acc, x, own [64]; out [32 * 64], left untouched in the lanes of exited rows
int dc_prim(const double* acc, const double* x, const double* own, int rows, int fused, int hazard, double* out) {
  double *d_in, *d_out;
  const size_t nout = 2 * TL * 64;
  if (hipMalloc(&d_in, 3 * 64 * sizeof(double)) != hipSuccess) return 1;
  if (hipMalloc(&d_out, nout * sizeof(double)) != hipSuccess) return 1;
  (void)hipMemcpy(d_in, acc, 64 * sizeof(double), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_in + 64, x, 64 * sizeof(double), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_in + 128, own, 64 * sizeof(double), hipMemcpyHostToDevice);
  (void)hipMemcpy(d_out, out, nout * sizeof(double), hipMemcpyHostToDevice);
  if (fused && hazard) prim_kernel<true, true><<<1, 64>>>(d_in, d_in + 64, d_in + 128, rows, d_out);
  else if (fused) prim_kernel<true, false><<<1, 64>>>(d_in, d_in + 64, d_in + 128, rows, d_out);
  else if (hazard) prim_kernel<false, true><<<1, 64>>>(d_in, d_in + 64, d_in + 128, rows, d_out);
  else prim_kernel<false, false><<<1, 64>>>(d_in, d_in + 64, d_in + 128, rows, d_out);
  int rc = finish();
  (void)hipMemcpy(out, d_out, nout * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return rc;
}

int dc_solve_f64(const double* H, const double* g, int rows, double* out) { return solve_host(H, g, rows, out); }
int dc_solve_f32(const float* H, const float* g, int rows, float* out) { return solve_host(H, g, rows, out); }

}  // extern "C"
