"""Deterministic policy evaluation on the batched env, with SB3's semantics.

Restates stable-baselines3 2.6.0 `evaluate_policy` as the reference's
EvalCallback calls it (ballbot_rl/training/callbacks.py:607-617: deterministic,
`evaluation.n_episodes` episodes, the eval VecEnv of train.py:90-97 wrapped in
Monitor, training/utils.py:81-83):
* the VecEnv is reset at the start (every env draws its next terrain from its
  own generator, np_random(seed + N_ENVS + i));
* env i must finish (n_eval_episodes + i) // n_envs episodes; all envs step
  together until every env has -- envs that are done or have no episode to
  count keep stepping and auto-resetting (their generators advance, exactly as
  in the reference, so the next evaluation starts on the same terrains);
* an episode's return is Monitor's: the float64 sum of the float32 step
  rewards since the env's last reset, rounded to 6 decimals; its length the
  step count; episodes are listed in the order they finish (env order within a
  step), which is the row order of EvalCallback's evaluations.npz.

Two forms.  evaluate_policy(fused=False) is the eager loop: the policy's torch modules, env.step
and a host check per step.  fused=True (DeviceEvaluator) replays ONE captured graph per step --
both cameras' encoders masked to the envs whose cameras re-rendered, bb_ppo_mlp_act, the env's
step launch, bb_eval_track -- and reads eight bytes every `poll` steps.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List

import numpy as np
import torch


def _policy_obs(env, obs):
    from ballbot_rl.training.ppo import env_images, policy_obs

    return policy_obs(obs, env_images(env), env.rel_ts) if getattr(env, "cameras", False) else obs


def _summary(rewards, lengths) -> Dict[str, object]:
    return {"mean_reward": float(np.mean(rewards)) if rewards else float("nan"),
            "std_reward": float(np.std(rewards)) if rewards else float("nan"),
            "mean_ep_length": float(np.mean(lengths)) if lengths else float("nan"),
            "episode_rewards": rewards, "episode_lengths": lengths}


def episode_targets(n_eval_episodes: int, n: int) -> np.ndarray:
    """SB3 evaluate_policy: env i owes (n_eval_episodes + i) // n_envs episodes."""
    return np.array([(n_eval_episodes + i) // n for i in range(n)], dtype=np.int64)


@torch.no_grad()
def evaluate_policy(policy, env, n_eval_episodes: int = 8, deterministic: bool = True,
                    max_steps: int = 1_000_000, return_episode_rewards: bool = False, fused: bool = False,
                    poll: int = 1) -> Dict[str, object]:
    """SB3 evaluate_policy on a BallbotVecEnv (auto-reset on).  -> {"mean_reward",
    "std_reward", "mean_ep_length", "episode_rewards", "episode_lengths"}.
    fused=True runs the captured device-side form (a DeviceEvaluator built for this call; keep one
    yourself to evaluate repeatedly) and adds "episode_envs" and "episode_steps"; `poll` is its host
    check interval in steps (1: stops at the eager loop's step)."""
    if fused:
        return DeviceEvaluator(policy, env).evaluate(n_eval_episodes, deterministic=deterministic,
                                                     max_steps=max_steps, poll=poll)
    n = int(env.num_envs)
    targets = episode_targets(n_eval_episodes, n)
    counts = np.zeros(n, dtype=np.int64)
    was_training = getattr(policy, "training", False)
    if hasattr(policy, "eval"):
        policy.eval()  # SB3 predict: set_training_mode(False) (BatchNorm running statistics)
    rewards: List[float] = []
    lengths: List[int] = []
    obs, _ = env.reset()
    dev = obs.device
    ret = torch.zeros(n, dtype=torch.float64, device=dev)
    length = torch.zeros(n, dtype=torch.int64, device=dev)
    try:
        for _ in range(max_steps):
            a = policy.predict(_policy_obs(env, obs), deterministic=deterministic)
            obs, r, term, trunc, info = env.step(a)
            flags = info.get("done_flags") if isinstance(info, dict) else None
            done = (term | trunc) if flags is None else ((flags & 1) != 0) | trunc
            ret += r.double()  # Monitor: float64 sum of the float32 rewards
            length += 1
            if bool(done.any()):
                d = done.cpu().numpy()
                rr, ll = ret.cpu().numpy(), length.cpu().numpy()
                for i in np.nonzero(d)[0]:
                    if counts[i] < targets[i]:
                        rewards.append(round(float(rr[i]), 6))
                        lengths.append(int(ll[i]))
                        counts[i] += 1
                ret.masked_fill_(done, 0.0)
                length.masked_fill_(done, 0)
                if not (counts < targets).any():
                    break
    finally:
        if hasattr(policy, "train"):
            policy.train(was_training)
    return _summary(rewards, lengths)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class DeviceEvaluator:
    """evaluate_policy with the whole step on the device: one captured graph per evaluation step.

    The graph, in order (camera policy): bb_depth_encoder (depth frames) or bb_rgbd_encoder (RGB-D
    frames, camera.disable_rgb: false, with 4-channel encoders) of camera 0 and of camera 1, each masked
    by `fresh` (the envs whose cameras rendered in the step before) and writing its 20 columns of
    the feature buffer in place; bb_ppo_mlp_act without noise (the mean, clipped to [-1, 1]); the
    env's step launch (bb_step and the cameras' cadence); bb_eval_track (the episode accounting, the
    proprio columns of the next step's features and the next `fresh`).  A proprio policy's graph is
    bb_ppo_mlp_act on env.obs, the step launch and bb_eval_track.  Every buffer the graph touches
    belongs to this object or is one of the env's fixed buffers (or the encoders' own tensors); the
    state is zeroed with tensor ops before a replay, so the graph holds kernel nodes only.

    The object keeps the graph across evaluations (EvalCallback builds one); the policy's trunk and
    head parameters are copied into a flat buffer at the start of every evaluation, the encoders'
    tensors are read in place.  A different n_eval_episodes captures a new graph.

    Refused, with a ValueError: a policy that is not the reference's MLP (pi = vf = [128]*4
    LeakyReLU(0.01), 15 or 56 features), camera encoders the fused kernels do not compute, encoders
    that read another channel count than the env renders (a depth policy on RGB-D frames or the
    reverse), a host reward plugin, an env that records per-episode logs, an env without
    auto-reset, a sampled (non-deterministic) evaluation."""

    def __init__(self, policy, env):
        from ballbot_gym import _native as N
        from ballbot_rl.training.ppo import pack_mlp_params, reference_mlp_tensors

        if "bb_eval_track" not in N.EXPORTS:
            raise RuntimeError("this build has no bb_eval_track")
        dev = torch.device(env.device)
        if dev.type != "cuda":
            raise ValueError(f"the fused evaluator runs on a GPU env (got {dev})")
        self.policy, self.env, self.device = policy, env, dev
        self.n = n = int(env.num_envs)
        self.cameras = bool(getattr(env, "cameras", False))
        if not getattr(env, "auto_reset", True):
            raise ValueError("the fused evaluator needs an env with auto_reset on (SB3's VecEnv)")
        if getattr(env, "_host_reward", None) is not None:
            raise ValueError("the fused evaluator needs a built-in reward: this env's reward is a host plugin, "
                             "evaluated per step() (use fused=False)")
        if getattr(env, "_reward_error", None):
            raise ValueError(env._reward_error)
        if getattr(env, "_log_on", False):
            raise ValueError("the fused evaluator does not step an env that records per-episode logs (log_options): "
                             "the reference's eval env writes none (use fused=False)")
        self.channels = int(getattr(env, "cam_channels", 1)) if self.cameras else 0
        if self.cameras and (env.cam_h, env.cam_w) != (64, 64):
            raise ValueError(f"the fused evaluator needs 64x64 camera frames (got {env.cam_h}x{env.cam_w})")
        ext = getattr(policy, "features_extractor", None)
        fd = int(getattr(ext, "features_dim", -1))
        if fd != (56 if self.cameras else 15):
            raise ValueError(f"the policy reads {fd} features, this env gives {56 if self.cameras else 15} "
                             f"(cameras {'on' if self.cameras else 'off'})")
        self.encs = ()
        if self.cameras:
            from ballbot_rl.encoders.models import fusable_encoder

            mods = getattr(ext, "extractors", {})
            for key in ("rgbd_0", "rgbd_1"):
                if key not in mods or not fusable_encoder(mods[key]):
                    raise ValueError(f"the fused evaluator needs frozen encoders of the reference's layout "
                                     f"(fusable_encoder): features_extractor.extractors.{key} is not one")
            self.encs = (mods["rgbd_0"], mods["rgbd_1"])
            for key, enc in zip(("rgbd_0", "rgbd_1"), self.encs):
                want = int(enc[0].in_channels)
                if want != self.channels:
                    kind = {1: "depth-only", 4: "RGB-D"}
                    raise ValueError(f"features_extractor.extractors.{key} reads {want}-channel ({kind[want]}) images, "
                                     f"this env renders {self.channels}-channel ({kind.get(self.channels, '?')}) frames "
                                     f"(camera.disable_rgb: {'false' if self.channels == 4 else 'true'}): RGB-D frames "
                                     "need encoders pretrained on RGB-D frames (pretrain --rgbd), depth frames depth "
                                     "encoders")
        self.tensors = reference_mlp_tensors(policy, self.cameras)
        if self.tensors is None:
            raise ValueError("the fused evaluator runs the reference's MLP policy (pi = vf = [128]*4 LeakyReLU(0.01), "
                             "a 3-d action head): this policy is not one (use fused=False)")
        self.flat, offsets = pack_mlp_params(self.tensors, dev)
        self.offsets = offsets
        self.offs = (C.c_int32 * 21)(*offsets)
        f32 = dict(dtype=torch.float32, device=dev)
        self.actions = torch.zeros(n, 3, **f32)
        self.clipped = torch.zeros(n, 3, **f32)
        self.values = torch.zeros(n, **f32)
        self.log_prob = torch.zeros(n, **f32)
        self.feats = torch.zeros(n, 56, **f32) if self.cameras else None
        self.fresh = torch.full((n,), -1, dtype=torch.int64, device=dev) if self.cameras else None
        self.ws = None
        if self.cameras:
            from ballbot_rl.encoders.models import encoder_workspace_bytes

            # one scratch: the two encoders run in turn
            self.ws = torch.empty(encoder_workspace_bytes(n, self.channels) // 4 + 4, **f32)
        self.ep_ret = torch.zeros(n, dtype=torch.float64, device=dev)
        self.ep_len = torch.zeros(n, dtype=torch.int64, device=dev)
        self.counts = torch.zeros(n, dtype=torch.int32, device=dev)
        self.targets = torch.zeros(n, dtype=torch.int32, device=dev)
        self.book = torch.zeros(4, dtype=torch.int64, device=dev)
        self.book_host = torch.zeros(4, dtype=torch.int64).pin_memory()
        self.event = torch.cuda.Event()
        self.cap = -1  # rows of the episode table (n_eval_episodes of the captured graph)
        self.tab_ret = self.tab_len = self.tab_env = self.tab_step = None
        self.graph = None
        self.steps = 0  # env.steps of the last evaluation

    # ------------------------------------------------------------------ pieces
    def _track_args(self, step: bool):
        from ballbot_gym import _native as N

        env = self.env
        return N.EvalArgs(self.n, max(self.cap, 0), _ptr(env.reward), _ptr(env.done) if step else None, _ptr(env.obs),
                          _ptr(env.rel_ts) if self.cameras else None, _ptr(self.targets), _ptr(self.ep_ret),
                          _ptr(self.ep_len), _ptr(self.counts), _ptr(self.tab_ret), _ptr(self.tab_len),
                          _ptr(self.tab_env), _ptr(self.tab_step), _ptr(self.book), _ptr(self.feats),
                          _ptr(self.fresh))

    def _track(self, step: bool) -> None:
        from ballbot_gym import _native as N

        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        args = self._track_args(step)
        N.check(N.lib().bb_eval_track(C.byref(args), stream), "bb_eval_track")

    def _encode(self, masked: bool) -> None:
        from ballbot_rl.encoders.models import fused_encoder_forward
        from ballbot_rl.training.ppo import camera_images, env_images

        frames = env_images(self.env)
        for c, enc in enumerate(self.encs):
            fused_encoder_forward(enc, camera_images(frames, c), index=self.fresh if masked else None,
                                  out=self.feats[:, 13 + 20 * c:33 + 20 * c], out_stride=56, workspace=self.ws)

    def _act(self) -> None:
        from ballbot_gym import _native as N

        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        obs = self.feats if self.cameras else self.env.obs
        N.check(N.lib().bb_ppo_mlp_act(_ptr(self.flat), self.offs, int(self.flat.numel()), _ptr(obs),
                                       int(obs.shape[1]), None, self.n, None, _ptr(self.actions), _ptr(self.clipped),
                                       _ptr(self.values), _ptr(self.log_prob), stream), "bb_ppo_mlp_act")

    def _step_nodes(self) -> None:
        if self.cameras:
            self._encode(masked=True)
        self._act()
        self.env._step_launch(self.clipped)
        self._track(step=True)

    def _capture(self) -> None:
        env, dev = self.env, self.device
        fixed = [env.obs.data_ptr(), env.reward.data_ptr(), env.done.data_ptr()]
        torch.cuda.synchronize(dev)
        env.note_graph_capture()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._step_nodes()
        torch.cuda.synchronize(dev)
        if fixed != [env.obs.data_ptr(), env.reward.data_ptr(), env.done.data_ptr()]:
            raise RuntimeError("the env's observation / reward / flag buffers moved during the capture")

    # --------------------------------------------------------------------- api
    @torch.no_grad()
    def evaluate(self, n_eval_episodes: int = 8, deterministic: bool = True, max_steps: int = 1_000_000,
                 poll: int = 1) -> Dict[str, object]:
        from ballbot_rl.training.ppo import refill_mlp_params

        if not deterministic:
            raise ValueError("the fused evaluator is deterministic (bb_ppo_mlp_act without noise): use fused=False "
                             "to sample actions")
        poll, E, n, dev = int(poll), int(n_eval_episodes), self.n, self.device
        if poll < 1 or E < 1:
            raise ValueError(f"poll and n_eval_episodes must be >= 1 (got {poll}, {E})")
        policy, env = self.policy, self.env
        was_training = bool(getattr(policy, "training", False))
        policy.eval()  # the encoders' BatchNorms normalise with their running statistics
        try:
            if E != self.cap:  # the table's size is a kernel argument: a new graph
                self.cap, self.graph = E, None
                self.tab_ret = torch.zeros(E, dtype=torch.float64, device=dev)
                self.tab_len = torch.zeros(E, dtype=torch.int64, device=dev)
                self.tab_env = torch.zeros(E, dtype=torch.int32, device=dev)
                self.tab_step = torch.zeros(E, dtype=torch.int64, device=dev)
            refill_mlp_params(self.flat, self.offsets, self.tensors)
            targets = episode_targets(E, n)
            self.targets.copy_(torch.from_numpy(targets.astype(np.int32)))
            self.ep_ret.zero_()
            self.ep_len.zero_()
            self.counts.zero_()
            self.book.copy_(torch.tensor([0, int(targets.sum()), 0, 0], dtype=torch.int64))
            env.reset()  # renders: every env's relative_image_timestamp is 0
            self._track(step=False)  # priming: the first step's proprio columns (and fresh = identity)
            if self.cameras:
                self._encode(masked=False)
            if self.graph is None:
                self._capture()  # the capture launches nothing
            steps, wanted = 0, int(targets.sum())
            while steps < max_steps and wanted > 0:
                self.graph.replay()
                steps += 1
                if steps % poll == 0 or steps == max_steps:
                    self.book_host[1:2].copy_(self.book[1:2], non_blocking=True)  # 8 bytes to pinned memory
                    self.event.record()
                    self.event.synchronize()
                    wanted = int(self.book_host[1])
            self.steps = steps
            self.book_host.copy_(self.book)
            listed, _, tracked, overflow = (int(v) for v in self.book_host)
            if overflow or listed > E:
                raise RuntimeError(f"bb_eval_track listed {listed} episodes into a table of {E} rows")
            if tracked != steps:
                raise RuntimeError(f"bb_eval_track counted {tracked} steps, the loop replayed {steps}")
            rets = self.tab_ret[:listed].cpu().numpy()
            out = _summary([round(float(v), 6) for v in rets], [int(v) for v in self.tab_len[:listed].cpu().numpy()])
            out["episode_envs"] = [int(v) for v in self.tab_env[:listed].cpu().numpy()]
            out["episode_steps"] = [int(v) for v in self.tab_step[:listed].cpu().numpy()]
            return out
        finally:
            policy.train(was_training)
