"""Evaluate a checkpoint on the batched env and print the result as one JSON line.

    python -m ballbot_rl.evaluation --model best_model.zip --config run/config.yaml
    python -m ballbot_rl.evaluation --model final_model.safetensors --terrain perlin --n-envs 64 --n-episodes 64

--model: a Stable-Baselines3 .zip (policy.pth alone is read, weights only) or this project's
.safetensors.  The env is the eval env train.py builds: from --config (a run's config.yaml, or a
training YAML that names its env_config) N = evaluation.num_envs or num_envs envs, env i drawing its
terrains from np_random(seed + num_envs + i); or, without a config, from the flags (directional
reward, cameras on when the policy reads 56 features, RGB-D frames when its encoders read 4 channels).  --n-envs, --n-episodes, --terrain and
--seed override the config.  The fused device-side evaluator runs unless --eager is given; --poll P is
its host check interval.  Also: --max-steps (the evaluation's step limit), --precision fp32|fp64 (the
env's arithmetic, fp64 as train.py's default), --device (cuda:0), --out FILE (the JSON line, also written there).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch


def _load_config(path: str):
    from ballbot_gym.core.config import load_config, load_training_config

    cfg = load_config(path)
    return load_training_config(str(Path(path).resolve())) if cfg.get("env_config") else cfg


def _load_policy(path: str, device):
    """-> (policy, meta).  safetensors: the policy's width is read from its first trunk layer."""
    if path.lower().endswith(".zip"):
        from ballbot_rl.evaluation.sb3_zip import load_sb3_policy

        return load_sb3_policy(path, device)
    from safetensors.torch import load_file

    from ballbot_rl.evaluation.sb3_zip import _empty_policy, encoder_channels

    state = load_file(path, device="cpu")
    w0 = state.get("policy_net.0.weight")
    if w0 is None or w0.dim() != 2 or int(w0.shape[1]) not in (15, 56):
        raise ValueError(f"{path}: no 15- or 56-wide policy_net.0.weight: not a policy this tool evaluates")
    policy = _empty_policy(int(w0.shape[1]), encoder_channels(state) if int(w0.shape[1]) == 56 else 1)
    policy.load_state_dict(state)
    for m in policy.features_extractor.extractors.values():
        m.eval()
    meta = {}
    side = Path(path + ".json")
    if side.exists():
        meta = json.loads(side.read_text())
    return policy.to(device), meta


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ballbot_rl.evaluation", description=__doc__.split("\n")[0])
    ap.add_argument("--model", required=True, help="SB3 .zip or .safetensors checkpoint")
    ap.add_argument("--config", default=None, help="a run's config.yaml or a training YAML")
    ap.add_argument("--terrain", default=None, help="terrain type (overrides the config; default flat)")
    ap.add_argument("--n-envs", type=int, default=None)
    ap.add_argument("--n-episodes", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--eager", action="store_true", help="the eager loop (torch modules, a host check per step)")
    ap.add_argument("--poll", type=int, default=1, help="fused: host check every POLL steps")
    ap.add_argument("--max-steps", type=int, default=1_000_000)
    ap.add_argument("--precision", default="fp64", choices=["fp32", "fp64"])
    ap.add_argument("--device", default="cuda:0", help="the GPU the env and the policy live on")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args(argv)

    from ballbot_rl.evaluation import evaluate_policy
    from ballbot_rl.training.train import make_env
    from ballbot_gym.distributed import shard_stream_seeds

    dev = torch.device(a.device)
    policy, meta = _load_policy(a.model, dev)
    cameras = policy.features_extractor.features_dim == 56
    cfg = _load_config(a.config) if a.config else {}
    cfg = dict(cfg)
    problem = dict(cfg.get("problem", {}) or {})
    if a.terrain is not None or not (problem.get("terrain") or cfg.get("terrain")):
        problem["terrain"] = {"type": a.terrain or "flat", "config": {}}
        cfg.pop("terrain", None)
    if not (problem.get("reward") or cfg.get("reward")):
        problem["reward"] = {"type": "directional", "config": {"target_direction": [0.0, 1.0]}}
    cfg["problem"] = problem
    if cameras and not cfg.get("camera"):
        rgbd = int(policy.features_extractor.extractors["rgbd_0"][0].in_channels) == 4
        cfg["camera"] = {"height": 64, "width": 64, "frame_rate": 90, "disable_rgb": not rgbd}
    if not cameras:
        cfg["disable_cameras"] = True
    ev = cfg.get("evaluation", {}) or {}
    seed = int(a.seed if a.seed is not None else cfg.get("seed", 0))
    n_total = int(cfg.get("num_envs", a.n_envs or 8))
    n_envs = int(a.n_envs if a.n_envs is not None else ev.get("num_envs", n_total))
    n_episodes = int(a.n_episodes if a.n_episodes is not None else ev.get("n_episodes", 8))
    # train.py's eval env: env i on np_random(seed + N_ENVS + i)
    env = make_env(cfg, n_envs, dev, seed + n_total, a.precision,
                   shard_stream_seeds(seed + n_total, 0, n_envs, per_env=True))
    try:
        r = evaluate_policy(policy, env, n_eval_episodes=n_episodes, max_steps=a.max_steps, fused=not a.eager,
                            poll=a.poll)
    finally:
        env.close()
    r.update({"model": str(a.model), "fused": not a.eager, "poll": int(a.poll), "n_envs": n_envs,
              "n_eval_episodes": n_episodes, "seed": seed,
              "terrain": (cfg.get("problem", {}).get("terrain") or {}).get("type"),
              "num_timesteps": meta.get("num_timesteps")})
    line = json.dumps(r)
    print(line, flush=True)
    if a.out:
        Path(a.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
