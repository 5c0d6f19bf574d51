// bb_pid.hip -- the batched PID balance controller (bb_pid_act, include/ballbot_mi355x.h): the
// reference's PID.act (ballbot_gym/controllers/pid.py:61-101) for n envs in one launch, next to
// bb_ppo_mlp_act in a step loop.  The arithmetic is pid_row's (bb_pid.h).
//
// One thread per env, nothing shared between threads.  Per env the launch reads 12 B (a rotation
// vector inside a 60-B observation row) or 36 B (a matrix), 8 B of setpoint, one flag byte and 16 B
// of state, and writes 16 B of state, 12 B of commands and 4 B of tilt: at 4096 envs under 300 KB,
// so the launch itself is the cost and the double-precision angles are free.  All accesses are
// scalar: an orientation row inside an observation (obs + 9, stride 15) is only float-aligned.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_pid.h"

namespace bb {
namespace {

constexpr int PID_THREADS = 256;

__global__ __launch_bounds__(PID_THREADS) void pid_act_kernel(PidCfg cfg, const float* __restrict__ orient,
                                                              long long stride, const float* __restrict__ sp,
                                                              const uint8_t* __restrict__ reset, int reset_mask,
                                                              float* __restrict__ state, int n,
                                                              float* __restrict__ out, float* __restrict__ angle_deg) {
  const int e = int(blockIdx.x) * PID_THREADS + int(threadIdx.x);
  if (e >= n) return;
  const size_t r = size_t(e);
  const int width = cfg.space == PID_PITCH_ROLL ? 2 : 3;
  const bool clear = reset && (reset[r] & reset_mask) != 0;
  pid_row(cfg, orient + (long long)e * stride, sp ? sp + 2 * r : nullptr, clear, state + 4 * r, out + width * r,
          angle_deg ? angle_deg + r : nullptr);
}

}  // namespace

int launch_pid_act(const PidCfg& cfg, const float* orient, long long stride, const float* sp, const uint8_t* reset,
                   int reset_mask, float* state, int n, float* out, float* angle_deg, hipStream_t s) {
  const dim3 grid((n + PID_THREADS - 1) / PID_THREADS);
  hipLaunchKernelGGL(pid_act_kernel, grid, dim3(PID_THREADS), 0, s, cfg, orient, stride, sp, reset, reset_mask, state,
                     n, out, angle_deg);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bb
