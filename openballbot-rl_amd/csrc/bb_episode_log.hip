// bb_episode_log.hip -- the recorder behind the reference's per-episode logs.
//
// The reference env appends two floats per step to reward_term_1_hist /
// reward_term_2_hist (ballbot_env.py:929-937) and _save_logs writes them when an
// episode ends (:673-699).  The step kernels add the two terms into one float
// (bb_step.h) and an auto-reset overwrites the terminal observation, so the terms
// are recomputed here from the step's post-step observation row -- the clipped
// action (obs[0:3]) and "vel" (obs[12:15]) are exactly the floats the step's
// reward read -- with the step's own float32 operation order and no FMA
// contraction: the results are the step's own floats (tests/test_gpu_episode_logs.py
// checks fl32(fl32(t1 + t2) + bonus) == reward bit for bit).
//
// HBM bound: per env-step reads 5 floats of a 60-B observation row and one flag byte
// (61 B of lines touched) and writes 8 B.  One launch: the [k][n] rows are spread
// over a (n / 256, k) grid; the blocks of step row 0 also walk their envs' k flag
// bytes for the episode bookkeeping.  The device-side step counter that places the
// block of rows in the history is read by every workgroup and advanced by the
// last one to finish (a ticket), so a captured graph replays consecutive blocks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_episode_log.h"

namespace bb {
namespace {

constexpr int LOG_THREADS = 256;
constexpr int LOG_MAX_ROWS = 1024;  // gridDim.y; more step rows than this are strided over

__global__ __launch_bounds__(LOG_THREADS) void reward_terms_kernel(RewardTermsCfg cfg, const float* __restrict__ obs,
                                                                   const uint8_t* __restrict__ flags, int K, int n,
                                                                   float* __restrict__ terms, long long terms_rows,
                                                                   long long* __restrict__ book) {
  const int e = int(blockIdx.x) * LOG_THREADS + int(threadIdx.x);
  if (e < n) {
    const long long base = book[2 * size_t(n)];  // steps recorded before this launch
    for (int j = int(blockIdx.y); j < K; j += int(gridDim.y)) {
      const size_t row = size_t(j) * size_t(n) + size_t(e);
      const float* o = obs + 15 * row;
      const float a0 = o[0], a1 = o[1], a2 = o[2], v0 = o[12], v1 = o[13];
      float t1, t2;
      {
        // bb_step.h's reward chain (numpy float32, no fused multiply-add)
#pragma clang fp contract(off)
        t1 = (v0 * cfg.target[0] + v1 * cfg.target[1]) * cfg.reward_scale;
        const float nrm = sqrtf(a0 * a0 + a1 * a1 + a2 * a2);
        t2 = cfg.action_reg_coef * (nrm * nrm);
      }
      const long long g = base + j;
      if (g >= 0 && g < terms_rows)
        *reinterpret_cast<float2*>(terms + 2 * (size_t(g) * size_t(n) + size_t(e))) = make_float2(t1, t2);
    }
    if (blockIdx.y == 0) {  // episode bookkeeping: this env's terminal rows of the block
      long long last = 0;
      int ended = 0;
      for (int j = 0; j < K; j++) {
        if (flags[size_t(j) * size_t(n) + size_t(e)] & 1) {  // BB_DONE_TERMINATED
          last = base + j + 1;
          ended++;
        }
      }
      if (ended) {
        book[e] = last;
        book[size_t(n) + size_t(e)] += ended;
      }
    }
  }
  // the last workgroup to get here advances the step counter: every workgroup has read it by then
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* ticket = reinterpret_cast<unsigned long long*>(book + 2 * size_t(n) + 1);
    const unsigned long long nwg = (unsigned long long)gridDim.x * gridDim.y;
    if (atomicAdd(ticket, 1ull) == nwg - 1) {
      book[2 * size_t(n)] += K;
      *ticket = 0ull;
    }
  }
}

}  // namespace

int launch_reward_terms(const RewardTermsCfg& cfg, const float* obs, const uint8_t* flags, int k, int n, float* terms,
                        long long terms_rows, long long* book, hipStream_t s) {
  const dim3 grid((n + LOG_THREADS - 1) / LOG_THREADS, k < LOG_MAX_ROWS ? k : LOG_MAX_ROWS);
  hipLaunchKernelGGL(reward_terms_kernel, grid, dim3(LOG_THREADS), 0, s, cfg, obs, flags, k, n, terms, terms_rows, book);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bb
