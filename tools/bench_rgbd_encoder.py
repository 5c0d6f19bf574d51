"""The frozen RGB-D encoder's cost, alone and inside PPO (profiles/rgbd_encoder.json).

    python tools/bench_rgbd_encoder.py encoder [--reps 20]
    python tools/bench_rgbd_encoder.py ppo [--root OTHER_CHECKOUT] [--envs 4096 --n-steps 64 --iters 4]

One JSON line per call; run each variant in its own process, alternating, at least three times.

encoder: one frozen encoder (random weights), per call the mean time of `--reps` forwards after 3
warm-ups, for the 4-channel encoder through bb_rgbd_encoder ("fused4"), the same module through
torch ("torch4": what BB_FUSED_ENCODER=0 runs) and the 1-channel encoder through bb_depth_encoder
("fused1"), at two shapes: eval mode over n = 4096 frames (a rollout step) and train mode gathering
B = 8192 rows of camera 1 from a 4096 x 64 rollout buffer (a PPO minibatch).

ppo: BatchedPPO on an RGB-D env (camera.disable_rgb: false, flat) with a random frozen 4-channel
encoder of the Extractor's layout, `--iters` iterations after warm_up(): env-steps/s with the rollout
/ update split.  --root names another checkout of this project (built) whose package is imported
instead of this one's: the commit before bb_rgbd_encoder sends the same encoder through its torch
modules and the autograd update, which is the yardstick.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def frozen_encoder(channels: int, seed: int = 0):
    import torch

    from ballbot_rl.policies.mlp_policy import depth_cnn

    torch.manual_seed(seed)
    enc = depth_cnn(channels, 64, 64)  # the encoder's layout, for any channel count on either checkout
    for p in enc.parameters():
        p.requires_grad = False
    return enc


def _time(fn, reps):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def bench_encoder(a):
    import torch

    from ballbot_rl.encoders.models import fused_encoder_forward

    dev = "cuda:0"
    out = {"mode": "encoder", "reps": a.reps, "us": {}}
    rows = a.envs * a.n_steps
    idx = torch.randperm(rows, device=dev, generator=torch.Generator(device=dev).manual_seed(1))[:a.batch]
    for name, ch in (("fused4", 4), ("torch4", 4), ("fused1", 1)):
        enc = frozen_encoder(ch).to(dev)
        frames = torch.empty(a.envs, 2, *((4,) if ch == 4 else ()), 64, 64, device=dev).uniform_()
        cam = frames[:, 1] if ch == 4 else frames[:, 1:2]
        enc.eval()
        with torch.no_grad():
            fn = (lambda: enc(cam)) if name == "torch4" else (lambda: fused_encoder_forward(enc, cam))
            out["us"][f"{name}_eval_n{a.envs}"] = _time(fn, a.reps)
        del frames, cam
        buf = torch.empty(rows, 2, *((4,) if ch == 4 else ()), 64, 64, device=dev).uniform_()
        cam = buf[:, 1] if ch == 4 else buf[:, 1:2]
        enc.train()
        with torch.no_grad():
            fn = (lambda: enc(cam[idx])) if name == "torch4" else (lambda: fused_encoder_forward(enc, cam, index=idx))
            out["us"][f"{name}_train_gather_B{a.batch}"] = _time(fn, a.reps)
        del buf, cam
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def bench_ppo(a):
    import torch

    from ballbot_gym.envs import BallbotVecEnv
    from ballbot_rl.training.logger import CSVLogger
    from ballbot_rl.training.ppo import BatchedPPO
    from ballbot_rl.training.schedules import lr_schedule

    env = BallbotVecEnv(a.envs, device="cuda:0", seed=10, terrain_config={"type": "flat", "config": {}},
                        disable_cameras=False, env_config={"camera": {"disable_rgb": False}})
    m = BatchedPPO(env, n_steps=a.n_steps, batch_size=a.batch, n_epochs=5, ent_coef=0.001, clip_range=0.015,
                   vf_coef=2.0, target_kl=0.3, learning_rate=lr_schedule, normalize_advantage=False, weight_decay=0.01,
                   seed=10, logger=CSVLogger(None, stdout=False), frozen_encoder=frozen_encoder(4))
    t = time.perf_counter()
    m.warm_up()
    setup_s = time.perf_counter() - t
    times = {"rollout": [], "update": []}
    collect, train = m.collect_rollouts, m.train

    def timed(fn, key):
        def run():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn(); torch.cuda.synchronize(); times[key].append(time.perf_counter() - t0)
        return run

    m.collect_rollouts, m.train = timed(collect, "rollout"), timed(train, "update")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.learn(total_timesteps=a.envs * a.n_steps * a.iters)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    g = m._graphs
    print(json.dumps({"mode": "ppo", "root": str(a.root), "env_steps_per_s": m.num_timesteps / el, "wall_s": el,
                      "setup_s": setup_s, "rollout_s": [round(x, 4) for x in times["rollout"]],
                      "update_s": [round(x, 4) for x in times["update"]],
                      "fused_rollout": bool(m._act_slots), "fused_update": bool(g is not None and g.fused),
                      "envs": a.envs, "n_steps": a.n_steps, "batch": a.batch, "iters": a.iters,
                      "kl_stops": getattr(m, "kl_stops", None)}), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("mode", choices=["encoder", "ppo"])
    ap.add_argument("--root", default=str(ROOT), help="the checkout whose package runs (default: this one)")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--n-steps", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.root, "openballbot-rl_amd"))
    (bench_encoder if a.mode == "encoder" else bench_ppo)(a)


if __name__ == "__main__":
    main()
