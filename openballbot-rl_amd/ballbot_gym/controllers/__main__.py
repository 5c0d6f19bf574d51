"""The reference's install check (scripts/test_pid.py:15-65) on this build:

    python -m ballbot_gym.controllers [pitch_deg roll_deg] [--num-envs 1] [--steps 25000] [--video PATH | --fused]

Flat terrain, max_ep_steps = steps, gains 20/15/2 ("better for 500hz, but not optimal"), the optional
setpoints in degrees.  Prints the reference's lines per env and exits with status 0 when no env failed.
--video writes env 0's world view, every 10th step, as an animated PNG: it stands in for GUI=True.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

GAINS = (20, 15, 2)
FRAME_EVERY = 10


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m ballbot_gym.controllers", description=__doc__.split("\n")[0])
    ap.add_argument("setpoints", nargs="*", type=float, metavar="DEG", help="pitch and roll setpoints in degrees")
    ap.add_argument("--num-envs", type=int, default=1)
    ap.add_argument("--steps", type=int, default=25000)
    ap.add_argument("--video", default=None, metavar="PATH", help="animated PNG of env 0's world view")
    ap.add_argument("--fused", action="store_true",
                    help="run the loop inside the launch (bb_pid_rollout, 500 steps per launch)")
    args = ap.parse_args(argv)
    if len(args.setpoints) not in (0, 2):
        ap.error("give both setpoints (pitch_deg roll_deg) or neither")
    if args.fused and args.video:
        ap.error("--video renders frames between steps: it cannot be combined with --fused")
    setpoint_p, setpoint_r = (np.deg2rad(args.setpoints) if args.setpoints else (0.0, 0.0))

    from ballbot_gym.envs import BallbotVecEnv

    from .pid import BatchedPID, balance

    env = BallbotVecEnv(args.num_envs, terrain_config={"type": "flat", "config": {}}, max_ep_steps=args.steps)
    try:
        pid = BatchedPID(env, *GAINS)
        frames = []

        def grab(t, e):
            if t % FRAME_EVERY == 0:
                frames.append(e.render_view([0], 320, 240)[0])

        out = balance(env, pid, args.steps, setpoint_r=float(setpoint_r), setpoint_p=float(setpoint_p),
                      callback=grab if args.video else None, fused=args.fused)
        if args.video:
            import torch

            from ballbot_rl.training.callbacks import write_apng

            write_apng(args.video, torch.stack(frames).cpu().numpy(), fps=1.0 / (FRAME_EVERY * env.opt_timestep))
    finally:
        env.close()
    for e in range(args.num_envs):
        tag = f"env {e}: " if args.num_envs > 1 else ""
        if out["failed"][e]:
            print(f"{tag}failed!")
        else:  # the reference prints the index of the last step
            print(f"{tag}successfuly balanced robot for {int(out['steps'][e]) - 1} steps")
        print(f"{tag}G_tau== {out['G_tau'][e]}")
    return 1 if out["failed"].any() else 0


if __name__ == "__main__":
    sys.exit(main())
