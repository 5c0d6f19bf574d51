// bb_episode_log.h -- the per-episode log recorder (bb_episode_log.hip), shared with the C-ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bb {

// the directional reward's settings (EnvCfg's, bb_step.h) as bb_reward_terms needs them
struct RewardTermsCfg {
  float target[2];
  float reward_scale;
  float action_reg_coef;
};

// reward terms of k steps' post-step observation rows + per-env episode bookkeeping
// (bb_reward_terms, include/ballbot_mi355x.h); book: long long[2 n + 2]
int launch_reward_terms(const RewardTermsCfg& cfg, const float* obs, const uint8_t* flags, int k, int n, float* terms,
                        long long terms_rows, long long* book, hipStream_t s);

}  // namespace bb
