"""Cost of the onboard cameras' two renderers on the same states (diagnostic, GPU box).

4096 envs at 64x64 on flat ground and on perlin (n_terrains 64), states after 200 random-action
steps.  A forced bb_render_depth and a forced bb_render_rgbd (every env, both cameras) are timed
with device events: warm-up, then 20 alternating repeats of each in one process.  The depth kernel
in the same call is the yardstick; the ratio is reported, there is no pass mark.  The env renders
every 6th step, so the per-step amortised cost is 1/6 of a forced render.

  python tools/camera_cost.py [--envs 4096] [--size 64] [--repeats 20] [--out profiles/rgbd_camera_cost.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "openballbot-rl_amd"))

import torch  # noqa: E402

from ballbot_gym import _native as N  # noqa: E402
from ballbot_gym.envs import BallbotVecEnv  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    s = sorted(ms)
    return {"median_ms": statistics.median(s), "min_ms": s[0], "max_ms": s[-1],
            "per_step_amortised_ms": statistics.median(s) / 6}


def measure(terrain, n, size, repeats, steps, seed):
    kw = {"n_terrains": 64} if terrain == "perlin" else {}
    env = BallbotVecEnv(n, device="cuda:0", terrain_config={"type": terrain, "config": {}}, seed=seed, **kw)
    g = torch.Generator(device=env.device).manual_seed(seed)
    for _ in range(steps):
        env.step(torch.rand(n, 3, generator=g, device=env.device) * 2 - 1)
    depth = torch.empty(n, 2, size, size, device=env.device)
    rgbd = torch.empty(n, 2, 4, size, size, device=env.device)
    L, p, s = N.lib(), (lambda t: C.c_void_p(t.data_ptr())), env._stream()

    def run_depth():
        N.check(L.bb_render_depth(env._h, p(depth), None, size, size, 6, 1, s), "bb_render_depth")

    def run_rgbd():
        N.check(L.bb_render_rgbd(env._h, p(rgbd), None, None, size, size, 6, 1, s), "bb_render_rgbd")

    for _ in range(3):
        run_depth()
        run_rgbd()
    torch.cuda.synchronize()
    td, tr = [], []
    for _ in range(repeats):
        td.append(timed(run_depth))
        tr.append(timed(run_rgbd))
    far = float((rgbd[:, :, 3] >= 1).float().mean())
    env.close()
    out = {"terrain": terrain, "envs": n, "size": size, "repeats": repeats, "state_steps": steps,
           "depth": spread(td), "rgbd": spread(tr), "share_of_pixels_at_depth_1": far}
    out["ratio_rgbd_over_depth"] = out["rgbd"]["median_ms"] / out["depth"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = [measure(t, a.envs, a.size, a.repeats, a.steps, a.seed) for t in ("flat", "perlin")]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}, indent=1) + "\n")


if __name__ == "__main__":
    main()
