"""SB3 EvalCallback as the reference configures it (ballbot_rl/training/callbacks.py:607-617).

Every `eval_freq` vec-env steps of the training VecEnv, `n_eval_episodes`
deterministic episodes on the eval VecEnv (evaluation.evaluate_policy, SB3's
semantics), with the parameters the training rollout ran with at that step
(SB3 calls EvalCallback._on_step inside collect_rollouts; BatchedPPO.learn
calls this with the rollout's vec-step range before the update).  Per
evaluation, as SB3 writes them:
* progress.csv gets a row with eval/mean_reward, eval/mean_ep_length,
  time/total_timesteps (and the train/* values recorded by the last update,
  which SB3's logger dumps with it);
* log_path/evaluations.npz holds timesteps [n_evals], results and ep_lengths
  [n_evals][n_eval_episodes] (np.savez, loadable with allow_pickle=False);
* a new best mean reward saves best_model.safetensors and calls `callback_on_new_best(model)`
  when one is given (the reference hangs its VideoRecorderOnBestCallback there, :94-293, 616).

VideoRecorder is this build's recorder of the reference's best-model videos: one deterministic
episode of the current policy on a dedicated one-env BallbotVecEnv, every `frame_skip`-th step
rendered by the HIP world-view renderer (BallbotVecEnv.render_view) straight into a preallocated
device stack, one device-to-host copy, an animated PNG written through PIL.  The reference records
on its eval env through VecVideoRecorder, which shifts that env's terrain stream; here the eval
env is never touched, so a run's evaluations are the same with videos on or off.
"""
from __future__ import annotations

from pathlib import Path
from typing import List, Optional

import numpy as np


class EvalCallback:
    def __init__(self, eval_env, n_eval_episodes: int = 8, eval_freq: int = 5000, n_total_envs: int = 1,
                 log_path: Optional[Path] = None, best_model_save_path: Optional[Path] = None,
                 deterministic: bool = True, callback_on_new_best=None, callback_after_eval=None,
                 fused: bool = False):
        self.eval_env = eval_env
        # fused: the device-side evaluator (one captured graph per step, kept across evaluations;
        # poll = 1, so every evaluation leaves the eval env where the eager loop would)
        self.fused = bool(fused)
        self._evaluator = None
        # called with the model: after a new best is saved / after every evaluation (None: nothing)
        self.callback_on_new_best, self.callback_after_eval = callback_on_new_best, callback_after_eval
        self.n_eval_episodes, self.eval_freq = int(n_eval_episodes), int(eval_freq)
        self.n_total_envs = int(n_total_envs)
        self.log_path = None if log_path is None else Path(log_path)
        self.best_path = None if best_model_save_path is None else Path(best_model_save_path)
        self.deterministic = deterministic
        self.best_mean_reward = -np.inf
        self.timesteps: List[int] = []
        self.results: List[List[float]] = []
        self.ep_lengths: List[List[int]] = []

    def due(self, first: int, last: int) -> List[int]:
        """Every multiple of eval_freq in vec-env steps [first, last]: SB3 calls _on_step at
        every vec-env step, so with eval_freq < n_steps one rollout holds several evaluations."""
        k0 = max(1, -(-first // self.eval_freq))
        return [k * self.eval_freq for k in range(k0, last // self.eval_freq + 1)]

    def __call__(self, model, first: int, last: int) -> None:
        for step in self.due(first, last):  # the rollout's fixed parameters, one evaluation per multiple
            self._evaluate(model, step)

    def _evaluate(self, model, step: int) -> None:
        from ballbot_rl.evaluation import evaluate_policy

        if self.fused:
            from ballbot_rl.evaluation import DeviceEvaluator

            if self._evaluator is None or self._evaluator.policy is not model.policy:
                self._evaluator = DeviceEvaluator(model.policy, self.eval_env)
            r = self._evaluator.evaluate(self.n_eval_episodes, deterministic=self.deterministic, poll=1)
        else:
            r = evaluate_policy(model.policy, self.eval_env, n_eval_episodes=self.n_eval_episodes,
                                deterministic=self.deterministic)
        ts = step * self.n_total_envs  # SB3's num_timesteps at that step
        self.timesteps.append(ts)
        self.results.append(r["episode_rewards"])
        self.ep_lengths.append(r["episode_lengths"])
        if self.log_path is not None:
            self.log_path.mkdir(parents=True, exist_ok=True)
            np.savez(self.log_path / "evaluations.npz", timesteps=np.array(self.timesteps),
                     results=np.array(self.results), ep_lengths=np.array(self.ep_lengths))
        L = model.logger
        L.record("eval/mean_reward", float(r["mean_reward"]))
        L.record("eval/mean_ep_length", float(r["mean_ep_length"]))
        L.record("time/total_timesteps", ts)
        L.dump(step=ts)
        if r["mean_reward"] > self.best_mean_reward:
            self.best_mean_reward = r["mean_reward"]
            if self.best_path is not None:
                model.save(str(self.best_path / "best_model.safetensors"))
            if self.callback_on_new_best is not None:
                self.callback_on_new_best(model)
        if self.callback_after_eval is not None:
            self.callback_after_eval(model)


def write_apng(path, frames: np.ndarray, fps: float = 30.0) -> None:
    """uint8 frames [F, H, W, 3] -> an animated PNG (lossless: the frames read back bit for bit).
    PIL encodes every frame; the APNG container (acTL, one fcTL per frame, IDAT / fdAT) is put
    together here, because PIL's own APNG writer merges consecutive identical frames into one."""
    import io
    import struct
    import zlib

    from PIL import Image

    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    if frames.ndim != 4 or frames.shape[-1] != 3 or frames.shape[0] < 1:
        raise ValueError(f"write_apng: need frames [F >= 1, H, W, 3], got {frames.shape}")
    n, h, w, _ = frames.shape

    def chunk(tag: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)

    out, seq = [b"\x89PNG\r\n\x1a\n"], 0
    for k in range(n):
        buf = io.BytesIO()
        Image.fromarray(frames[k], "RGB").save(buf, format="PNG")
        png, pos, idat, ihdr = buf.getvalue(), 8, [], b""
        while pos < len(png):
            (size,), tag = struct.unpack(">I", png[pos:pos + 4]), png[pos + 4:pos + 8]
            if tag == b"IDAT":
                idat.append(png[pos + 8:pos + 8 + size])
            elif tag == b"IHDR":
                ihdr = png[pos + 8:pos + 8 + size]
            pos += 12 + size
        if k == 0:
            out += [chunk(b"IHDR", ihdr), chunk(b"acTL", struct.pack(">II", n, 0))]
        # whole frame at (0, 0), delay 1000 / fps ms, dispose none, blend source: every frame stands alone
        out.append(chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, int(round(1000.0 / fps)), 1000, 0, 0)))
        seq += 1
        for body in idat:
            if k == 0:
                out.append(chunk(b"IDAT", body))
            else:
                out.append(chunk(b"fdAT", struct.pack(">I", seq) + body))
                seq += 1
    out.append(chunk(b"IEND", b""))
    with open(str(path), "wb") as f:
        f.write(b"".join(out))


def read_apng(path) -> np.ndarray:
    """The frames uint8 [F, H, W, 3] of a file written by write_apng."""
    from PIL import Image

    with Image.open(str(path)) as im:
        out = []
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            out.append(np.asarray(im.convert("RGB")).copy())
    return np.stack(out)


class VideoRecorder:
    """Records `<folder>/<name_prefix>_episode_<k>.png` (k = 1, 2, ...), one file per call.

    `video_env` is a one-env BallbotVecEnv of the recorder's own (train.make_env with the run's
    config): it is reset, stepped with the policy's deterministic action until the episode ends or
    `video_length` steps, and rendered after the reset and after every `frame_skip`-th step
    (`frame_steps`).  frame_skip 17 plays in real time at 30 frames per second with dt = 2 ms.
    `size` is (height, width), as the reference unpacks _video_renderer_size.  With `async_write`
    only the encode and the file write run in a background thread; close() joins it."""

    def __init__(self, video_env, folder, video_length: int = 4000, frame_skip: int = 17, size=(640, 480),
                 name_prefix: str = "best_model", async_write: bool = True, episodes: int = 1, fps: float = 30.0):
        if int(video_env.num_envs) != 1:
            raise ValueError(f"VideoRecorder needs a one-env video env of its own, got {video_env.num_envs} envs")
        if int(frame_skip) < 1 or int(video_length) < 1 or int(episodes) < 1:
            raise ValueError("VideoRecorder: video_length, frame_skip and episodes must be >= 1")
        self.env, self.folder = video_env, Path(folder)
        self.video_length, self.frame_skip, self.episodes = int(video_length), int(frame_skip), int(episodes)
        self.height, self.width = int(size[0]), int(size[1])
        self.name_prefix, self.async_write, self.fps = name_prefix, bool(async_write), float(fps)
        self.count = 0
        self.paths: List[Path] = []
        self.stack = None   # device frames [F_max, H, W, 3], allocated at the first recording
        self._threads: list = []

    @staticmethod
    def frame_steps(n_steps: int, frame_skip: int) -> List[int]:
        """The step counts after which a frame is rendered in an episode of n_steps steps:
        0 (the reset state) and every multiple of frame_skip up to n_steps."""
        return list(range(0, int(n_steps) + 1, int(frame_skip)))

    def __call__(self, model) -> Path:
        return self.record(model)

    def record(self, model) -> Path:
        import torch

        from ballbot_rl.evaluation.evaluate import _policy_obs

        env, policy = self.env, getattr(model, "policy", model)
        per_episode = self.video_length // self.frame_skip + 1
        if self.stack is None:
            self.stack = torch.zeros(per_episode * self.episodes, self.height, self.width, 3, dtype=torch.uint8,
                                     device=env.device)
        was_training = getattr(policy, "training", False)
        if hasattr(policy, "eval"):
            policy.eval()
        f = 0
        try:
            with torch.no_grad():
                for _ in range(self.episodes):
                    obs, _ = env.reset()
                    env.render_view(None, self.height, self.width, out=self.stack[f:f + 1])
                    f += 1
                    for t in range(1, self.video_length + 1):
                        a = policy.predict(_policy_obs(env, obs), deterministic=True)
                        obs, _, term, trunc, info = env.step(a)
                        flags = info.get("done_flags") if isinstance(info, dict) else None
                        done = (term | trunc) if flags is None else ((flags & 1) != 0) | trunc
                        if bool(done.any()):  # the env has auto-reset: the state is the next episode's
                            break
                        if t % self.frame_skip == 0:
                            env.render_view(None, self.height, self.width, out=self.stack[f:f + 1])
                            f += 1
        finally:
            if hasattr(policy, "train"):
                policy.train(was_training)
        frames = self.stack[:f].cpu().numpy()  # the one device-to-host copy
        self.count += 1
        self.folder.mkdir(parents=True, exist_ok=True)
        path = self.folder / f"{self.name_prefix}_episode_{self.count}.png"
        self.paths.append(path)
        if self.async_write:
            import threading

            th = threading.Thread(target=write_apng, args=(path, frames, self.fps), daemon=False)
            th.start()
            self._threads.append(th)
        else:
            write_apng(path, frames, self.fps)
        return path

    def close(self) -> None:
        """Join the writer threads and close the video env."""
        for th in self._threads:
            th.join()
        self._threads = []
        if self.env is not None:
            self.env.close()
            self.env = None


def video_options(config) -> Optional[dict]:
    """The reference's `visualization` section (configs/train/ppo_directional.yaml:181-197) ->
    the recorder's options, or None when nothing is to be recorded (no section, or record_videos
    false).  video_freq: "on_new_best" | "every_eval" | int N (every N-th evaluation)."""
    viz = config.get("visualization")
    if not viz or not viz.get("record_videos", False):
        return None
    freq = viz.get("video_freq", "on_new_best")
    if not (freq in ("on_new_best", "every_eval") or (isinstance(freq, int) and not isinstance(freq, bool) and freq >= 1)):
        raise ValueError(f'visualization.video_freq must be "on_new_best", "every_eval" or an integer >= 1, got {freq!r}')
    size = viz.get("video_size", (640, 480))
    max_ep = int((config.get("env", {}) or {}).get("max_ep_steps", 4000))
    return {"video_freq": freq, "episodes": int(viz.get("video_episodes", 1)),
            "async_write": bool(viz.get("async_video_recording", True)),
            "video_length": int(viz.get("video_length", max_ep)), "frame_skip": int(viz.get("video_frame_skip", 17)),
            "size": (int(size[0]), int(size[1])),
            "name_prefix": "best_model" if freq == "on_new_best" else "eval"}


class EveryNth:
    """Calls `fn(model)` at every n-th call (the reference's integer video_freq)."""

    def __init__(self, fn, n: int):
        self.fn, self.n, self.calls = fn, int(n), 0

    def __call__(self, model) -> None:
        self.calls += 1
        if self.calls % self.n == 0:
            self.fn(model)
