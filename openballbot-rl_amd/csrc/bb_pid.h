// bb_pid.h -- the balance controller's row function (ballbot_gym/controllers/pid.py:61-101 of the
// reference), shared by the kernel (bb_pid.hip), the C-ABI (bb_pid_act) and the host build of
// tests/hostcheck/pid_check.cpp.  No HIP header is needed: a plain C++ compiler takes this file.
//
// Angles.  Only the third row of R enters: roll = atan2(R21, R22), pitch = atan2(-R20,
// sqrt(R21^2 + R22^2)), tilt = acos(R22).  The row is a float row (given, or Rodrigues in double from
// the float rotation vector and rounded once, as the reference's script rounds its float64 matrix
// with .float()); the angles are then taken in double and rounded once to float, so each is within
// half an ulp of the exact angle of that float row, whatever a single-precision atan2f would give.
// The recurrence that follows is the reference's float32 chain, in its order, without fused
// multiply-adds.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BB_PID_HD __host__ __device__ inline
#else
#define BB_PID_HD inline
#endif
// The double-precision angle code below is compiled for the GPU under bb_pid.hip's contraction mode
// (the compiler's default) in every unit that inlines it, whatever file-level pragma that unit sets
// (bb_kernels.hip: contract(on)), so that pid_rollout_kernel's angles are bb_pid_act's bit for bit.
#if defined(__HIP_DEVICE_COMPILE__)
#define BB_PID_DEVICE_CONTRACT _Pragma("clang fp contract(fast)")
#else
#define BB_PID_DEVICE_CONTRACT
#endif

namespace bb {

constexpr int PID_ROTVEC = 0, PID_ROTMAT = 1;   // BB_PID_ROTVEC / BB_PID_ROTMAT
constexpr int PID_MOTOR = 0, PID_PITCH_ROLL = 1;  // BB_PID_MOTOR / BB_PID_PITCH_ROLL

// bb_pid_cfg (include/ballbot_mi355x.h), field for field
struct PidCfg {
  float dt, k_p, k_i, k_d, limit;
  int32_t orient_kind, space;
};

// third row of R as floats: read (ROTMAT: o[6..8]) or computed in double from the rotation vector
// o[0..2], R = I + sin(th) K + (1 - cos(th)) K^2 with identity below 1e-14 rad.  Scalar reads only:
// a row inside an observation is float-aligned.
BB_PID_HD void pid_third_row(const float* o, int kind, float r[3]) {
  BB_PID_DEVICE_CONTRACT
  if (kind == PID_ROTMAT) {
    r[0] = o[6]; r[1] = o[7]; r[2] = o[8];
    return;
  }
  const double x = o[0], y = o[1], z = o[2];
  const double th = sqrt(x * x + y * y + z * z);
  if (th < 1e-14) {
    r[0] = 0.f; r[1] = 0.f; r[2] = 1.f;
    return;
  }
  const double kx = x / th, ky = y / th, kz = z / th;
  const double s = sin(th), c1 = 1.0 - cos(th);
  // row 2 of K is (-ky, kx, 0), row 2 of K^2 is (kx kz, ky kz, -(kx^2 + ky^2))
  r[0] = float(-s * ky + c1 * (kx * kz));
  r[1] = float(s * kx + c1 * (ky * kz));
  r[2] = float(1.0 - c1 * (kx * kx + ky * ky));
}

// One env's PID.act.  orient: the env's orientation row; sp: its (pitch, roll) setpoint or nullptr
// (zero); st: its state row, integral (pitch, roll) then prev_err (pitch, roll), read and written;
// clear: start from a zero state; out: 3 motor commands clamped to +-limit, or u (pitch, roll)
// unclamped; angle_deg: the tilt in degrees, or nullptr.  A NaN in the row gives NaN outputs (a
// clamp written with comparisons passes it on, as torch.clamp does).
BB_PID_HD void pid_row(const PidCfg& cfg, const float* orient, const float* sp, bool clear, float* st, float* out,
                       float* angle_deg) {
  BB_PID_DEVICE_CONTRACT
  float r[3];
  pid_third_row(orient, cfg.orient_kind, r);
  const double r0 = r[0], r1 = r[1], r2 = r[2];
  const float roll = float(atan2(r1, r2));
  const float pitch = float(atan2(-r0, sqrt(r1 * r1 + r2 * r2)));
  if (angle_deg) {
    const double c = r2 < -1.0 ? -1.0 : (r2 > 1.0 ? 1.0 : r2);
    *angle_deg = float(acos(c) * (180.0 / 3.14159265358979323846));
  }
  float integ[2] = {st[0], st[1]}, prev[2] = {st[2], st[3]};
  if (clear) integ[0] = integ[1] = prev[0] = prev[1] = 0.f;
  const float set[2] = {sp ? sp[0] : 0.f, sp ? sp[1] : 0.f};
  const float ang[2] = {pitch, roll};
  float u[2];
  {
    // torch's float32 chain (pid.py:74-82): no fused multiply-add anywhere
#pragma clang fp contract(off)
    for (int i = 0; i < 2; i++) {
      const float e = set[i] - ang[i];
      integ[i] = integ[i] + e * cfg.dt;
      const float d = (e - prev[i]) / cfg.dt;
      u[i] = (cfg.k_p * e + cfg.k_i * integ[i]) + cfg.k_d * d;
      prev[i] = e;
    }
    st[0] = integ[0]; st[1] = integ[1]; st[2] = prev[0]; st[3] = prev[1];
    if (cfg.space == PID_PITCH_ROLL) {
      out[0] = u[0]; out[1] = u[1];
      return;
    }
    // float(cos / sin(deg2rad(0, 120, 240))) of the double values (pid.py:96-98)
    const float ck[3] = {1.f, -0.5f, -0.5f};
    const float sk[3] = {0.f, 0.8660253882408142f, -0.8660253882408142f};
    for (int k = 0; k < 3; k++) {
      const float c = u[1] * ck[k] + u[0] * sk[k];
      out[k] = c < -cfg.limit ? -cfg.limit : (c > cfg.limit ? cfg.limit : c);
    }
  }
}

// balance()'s per-env accumulators (controllers/pid.py: balance, the loop of the reference's
// scripts/test_pid.py:38-65), one env's row of bb_pid_rollout's summary buffers
struct PidSummary {
  uint8_t alive, failed;  // 0 / 1
  int64_t steps;
  float max_angle;
  double g_tau;
  float pos[2];
};

// One step of balance()'s accumulation for one env, in its order: deg is the tilt the controller saw
// before the step, r / flags / p2 the step's reward, BB_DONE_* bits and base position, w = gamma^t
// (from the host: no pow here, so G_tau does not depend on a device's pow).  max_angle follows
// torch.maximum (a NaN propagates); the product and the sum of G_tau are two roundings, never one
// fused multiply-add.
BB_PID_HD void pid_summary_step(PidSummary& s, float deg, float r, int flags, const float* p2, double w) {
  const bool alive = s.alive != 0, term = (flags & 1) != 0, failure = (flags & 2) != 0;  // BB_DONE_TERMINATED, _FAILURE
  if (alive) s.max_angle = deg != deg ? deg : (s.max_angle != s.max_angle || s.max_angle > deg ? s.max_angle : deg);
  s.steps += alive;
  {
    // the product rounded, then the sum rounded, as torch's separate mul and add kernels.  Written as
    // plain operators under contract(off) on the host and the device alike: HIP's __dmul_rn /
    // __dadd_rn are the plain operators too, and written with them the device build still fused the
    // two into one v_fma_f64 (1 ulp off in G_tau after 120 steps, measured against balance()).
#pragma clang fp contract(off)
    const double prod = double(r) * w;
    s.g_tau = s.g_tau + (alive ? prod : 0.0);
  }
  if (alive) { s.pos[0] = p2[0]; s.pos[1] = p2[1]; }
  s.failed |= uint8_t(alive && term && failure);
  s.alive = uint8_t(alive && !term);
}

#if defined(__HIPCC__)
// one launch on s: row e of n reads orient + e * stride, sp + 2 e, reset[e] & reset_mask, and
// reads/writes state + 4 e, out + (3 | 2) e, angle_deg + e (bb_pid_act, include/ballbot_mi355x.h)
int launch_pid_act(const PidCfg& cfg, const float* orient, long long stride, const float* sp, const uint8_t* reset,
                   int reset_mask, float* state, int n, float* out, float* angle_deg, hipStream_t s);
#endif

}  // namespace bb
