// bb_eval.hip -- one evaluation step's episode accounting and the policy's per-step staging in ONE
// launch (bb_eval_track, include/ballbot_mi355x.h).  The arithmetic is eval_account's and the staging
// eval_stage's (bb_eval.h); this file only places the listed episodes.
//
// Launch shape: workgroup 0 does the accounting alone, workgroups 1.. stage 1024 envs each.  The two
// halves share nothing (the accounting reads reward / flags / targets, the staging reads obs /
// rel_ts), so they need no order between them, and a grid keeps the staging's 136 B per env off one
// CU's load/store path at 32768 envs.  The episode table's order (env order within a step, steps in
// order) needs ranks over all n envs, so the accounting stays in one workgroup and no atomic is used:
// 16 waves walk n in chunks of 1024 envs; in a chunk each lane decides whether its env lists an
// episode, a wave ballot gives the lane its rank within the wave (the count of set bits below it,
// mbcnt), the 16 wave totals go through LDS and every thread adds those of the waves before its own.
// The running base is the same value in every thread, so no broadcast is needed between chunks.
// Thread 0 alone writes book[], after the last chunk.  All stores are ordinary vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bb_eval.h"

namespace bb {
namespace {

constexpr int EVAL_THREADS = 1024;
constexpr int EVAL_WAVES = EVAL_THREADS / 64;

__global__ __launch_bounds__(EVAL_THREADS) void eval_track_kernel(EvalArgs a, int acct_blocks) {
  const int t = int(threadIdx.x);
  if (int(blockIdx.x) >= acct_blocks) {  // staging: one env per thread
    const long long e = (long long)(int(blockIdx.x) - acct_blocks) * EVAL_THREADS + t;
    if (e < a.n) eval_stage(a, int(e));
    return;
  }
  __shared__ int wave_total[EVAL_WAVES];
  const int lane = t & 63, w = t >> 6;
  const long long listed0 = a.book[0];  // read by every thread before thread 0 writes it (barriers below)
  const long long step = a.book[2] + 1;
  long long base = listed0;
  for (long long c0 = 0; c0 < a.n; c0 += EVAL_THREADS) {
    const long long e = c0 + t;
    bool listed = false;
    double r = 0.0;
    int64_t l = 0;
    if (e < a.n) {
      double ret = a.ep_ret[e];
      int64_t len = a.ep_len[e];
      int32_t cnt = a.counts[e];
      listed = eval_account(a.reward[e], a.flags[e], a.targets[e], ret, len, cnt, r, l);
      a.ep_ret[e] = ret;
      a.ep_len[e] = len;
      if (listed) a.counts[e] = cnt;
    }
    const unsigned long long m = __ballot(listed);
    const int below = int(__builtin_amdgcn_mbcnt_hi(unsigned(m >> 32), __builtin_amdgcn_mbcnt_lo(unsigned(m), 0u)));
    if (lane == 0) wave_total[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < EVAL_WAVES; i++) {
      const int v = wave_total[i];
      before += i < w ? v : 0;
      total += v;
    }
    if (listed) {
      const long long pos = base + before + below;
      if (pos < a.cap) {
        a.tab_ret[pos] = r;
        a.tab_len[pos] = l;
        a.tab_env[pos] = int32_t(e);
        a.tab_step[pos] = step;
      }
    }
    base += total;
    __syncthreads();  // wave_total is rewritten by the next chunk
  }
  if (t == 0) {
    a.book[0] = base;
    a.book[1] -= base - listed0;
    a.book[2] = step;
    if (base > a.cap && base > listed0) a.book[3] = 1;
  }
}

}  // namespace

int launch_eval_track(const EvalArgs& a, hipStream_t s) {
  const int acct = a.flags ? 1 : 0;
  const int stage = (a.feats || a.fresh) ? (a.n + EVAL_THREADS - 1) / EVAL_THREADS : 0;
  if (acct + stage == 0) return 0;
  hipLaunchKernelGGL(eval_track_kernel, dim3(acct + stage), dim3(EVAL_THREADS), 0, s, a, acct);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace bb
