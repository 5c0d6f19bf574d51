"""A numpy restatement of evaluate_policy's bookkeeping (ballbot_rl/evaluation/evaluate.py), one
step per call on arrays, with the layout bb_eval_track keeps (include/ballbot_mi355x.h) -- and the
random reward / flag streams the host and GPU tests of bb_eval_track share."""
import numpy as np

SENTINEL = -777.0


def targets_for(E, n):
    """SB3 evaluate_policy: env i owes (E + i) // n episodes."""
    return np.array([(E + i) // n for i in range(n)], np.int32)


class TrackRef:
    """evaluate_policy's loop body: ret += r.double(); length += 1; the done envs in env order are
    listed while counts < targets; their sums restart."""

    def __init__(self, n, targets, cap):
        self.n, self.cap = n, cap
        self.targets = np.asarray(targets, np.int32)
        self.ep_ret = np.zeros(n, np.float64)
        self.ep_len = np.zeros(n, np.int64)
        self.counts = np.zeros(n, np.int32)
        self.tab_ret = np.full(cap, SENTINEL, np.float64)
        self.tab_len = np.full(cap, -7, np.int64)
        self.tab_env = np.full(cap, -7, np.int32)
        self.tab_step = np.full(cap, -7, np.int64)
        self.book = np.array([0, int(self.targets.sum()), 0, 0], np.int64)

    def step(self, reward, flags):
        self.ep_ret += reward.astype(np.float64)
        self.ep_len += 1
        self.book[2] += 1
        for i in np.nonzero(flags & 1)[0]:
            if self.counts[i] < self.targets[i]:
                k = int(self.book[0])
                if k < self.cap:
                    self.tab_ret[k], self.tab_len[k] = self.ep_ret[i], self.ep_len[i]
                    self.tab_env[k], self.tab_step[k] = i, self.book[2]
                else:
                    self.book[3] = 1
                self.book[0] += 1
                self.book[1] -= 1
                self.counts[i] += 1
            self.ep_ret[i] = 0.0
            self.ep_len[i] = 0


def stage_ref(obs, rel_ts, feats, fresh):
    """The staging half: proprio columns of the feature rows and the encoder's index (in place)."""
    feats[:, 0:12] = obs[:, 0:12]
    feats[:, 53:56] = obs[:, 12:15]
    if rel_ts is None:
        fresh[:] = -1
        return
    feats[:, 12] = rel_ts
    fresh[:] = np.where(rel_ts == 0, np.arange(len(rel_ts)), -1)


def streams(n, T=50, p_done=0.2, seed=0):
    """Random inputs of T steps: reward f32[T, n], flags u8[T, n] (TERMINATED with p_done, other
    BB_DONE_* bits at random: only bit 0 may matter), obs f32[T, n, 15], rel_ts f32[T, n] (zero for
    about a third of the rows)."""
    rng = np.random.default_rng(1000 * seed + n)
    reward = rng.normal(0.02, 0.01, (T, n)).astype(np.float32)
    flags = (rng.random((T, n)) < p_done).astype(np.uint8) | (rng.integers(0, 8, (T, n)).astype(np.uint8) << 1)
    obs = rng.normal(0, 1, (T, n, 15)).astype(np.float32)
    rel_ts = (rng.integers(0, 3, (T, n)) * 0.002).astype(np.float32)
    return reward, flags, obs, rel_ts
