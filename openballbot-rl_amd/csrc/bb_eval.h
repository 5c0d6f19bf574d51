// bb_eval.h -- the episode accounting of evaluate_policy (ballbot_rl/evaluation/evaluate.py; SB3
// evaluate_policy over a Monitor-wrapped VecEnv, as the reference's EvalCallback calls it), stated
// once: eval_account is one env's share of one step, eval_track_serial the whole call in env order.
// The kernel (bb_eval.hip) runs eval_account per env and places the listed episodes by a stable
// compaction; the host build of tests/hostcheck/eval_track_check.cpp runs eval_track_serial.  No HIP
// header is needed: a plain C++ compiler takes this file.
//
// Per step and env: ep_ret += double(reward) (Monitor's float64 sum of the float32 rewards), ep_len
// += 1.  An env whose flags carry BB_DONE_TERMINATED finishes an episode: it is listed while the env
// still owes episodes (counts < targets; counts then goes up), dropped otherwise, and the env's sums
// restart either way.  The episodes of one step are listed in env order after those of every earlier
// step (the row order of EvalCallback's evaluations.npz).  book = {episodes listed, episodes still
// wanted, steps tracked, overflow}: a listing at or past cap is counted in book[0] and taken off
// book[1] but not written, and sets book[3].  tab_step holds the number of steps tracked when the
// episode ended (1 for an episode that ends in the first step).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BB_EVAL_HD __host__ __device__ inline
#else
#define BB_EVAL_HD inline
#endif

namespace bb {

constexpr int EVAL_FEATS = 56;  // proprio 15 + relative_image_timestamp + 2 x 20 camera features
constexpr int EVAL_CAM0 = 13;   // first camera feature column; EVAL_CAM0 + 40 = 53 starts obs[12:15]

// bb_eval_args (include/ballbot_mi355x.h), field for field
struct EvalArgs {
  int32_t n, cap;
  const float* reward;
  const uint8_t* flags;
  const float* obs;
  const float* rel_ts;
  const int32_t* targets;
  double* ep_ret;
  int64_t* ep_len;
  int32_t* counts;
  double* tab_ret;
  int64_t* tab_len;
  int32_t* tab_env;
  int64_t* tab_step;
  int64_t* book;
  float* feats;
  int64_t* fresh;
};

// One env's step.  ret / len / count: its running sums and listed-episode count, read and written.
// -> true when the step lists an episode; its return and length are then in out_ret / out_len.
BB_EVAL_HD bool eval_account(float reward, int flags, int32_t target, double& ret, int64_t& len, int32_t& count,
                             double& out_ret, int64_t& out_len) {
  ret += double(reward);
  len += 1;
  if (!(flags & 1)) return false;  // BB_DONE_TERMINATED
  const bool listed = count < target;
  if (listed) {
    out_ret = ret;
    out_len = len;
    count += 1;
  }
  ret = 0.0;
  len = 0;
  return listed;
}

// One env's staging row: the proprio columns of the policy's feature row and the encoder's index.
// rel_ts == nullptr (no cameras): column 12 is left alone and the env is never fresh.
BB_EVAL_HD void eval_stage(const EvalArgs& a, int e) {
  const float* o = a.obs + size_t(e) * 15;
  const bool cam = a.rel_ts != nullptr;
  const float ts = cam ? a.rel_ts[e] : 1.f;
  if (a.feats) {
    float* f = a.feats + size_t(e) * EVAL_FEATS;
    for (int k = 0; k < 12; k++) f[k] = o[k];
    if (cam) f[12] = ts;
    for (int k = 0; k < 3; k++) f[EVAL_CAM0 + 40 + k] = o[12 + k];
  }
  if (a.fresh) a.fresh[e] = (cam && ts == 0.f) ? int64_t(e) : int64_t(-1);
}

// The whole call, one env after the other: what the kernel must leave behind.
inline void eval_track_serial(const EvalArgs& a) {
  if (a.flags) {
    int64_t listed = a.book[0];
    const int64_t step = a.book[2] + 1;
    for (int e = 0; e < a.n; e++) {
      double r = 0.0;
      int64_t l = 0;
      if (!eval_account(a.reward[e], a.flags[e], a.targets[e], a.ep_ret[e], a.ep_len[e], a.counts[e], r, l)) continue;
      if (listed < a.cap) {
        a.tab_ret[listed] = r;
        a.tab_len[listed] = l;
        a.tab_env[listed] = e;
        a.tab_step[listed] = step;
      } else {
        a.book[3] = 1;
      }
      listed += 1;
      a.book[1] -= 1;
    }
    a.book[0] = listed;
    a.book[2] = step;
  }
  if (a.feats || a.fresh)
    for (int e = 0; e < a.n; e++) eval_stage(a, e);
}

#if defined(__HIPCC__)
// one launch on s (bb_eval_track, include/ballbot_mi355x.h); the arguments are already checked
int launch_eval_track(const EvalArgs& a, hipStream_t s);
#endif

}  // namespace bb
