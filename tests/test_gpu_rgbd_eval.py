"""GPU: the device-side evaluator and the evaluation command line on an RGB-D env
(camera.disable_rgb: false) with frozen 4-channel encoders -- the twins of tests/test_gpu_eval.py's
depth tests, with its constructions (Twin, _env's streams, the saturating policy) and its bit-for-bit
comparison.  Before bb_rgbd_encoder the DeviceEvaluator refused such an env outright."""
import json
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rgbd_encoder_ref as G  # noqa: E402
import test_gpu_eval as E  # noqa: E402

DEV = E.DEV


def _policy(seed=0, scale=150.0):
    """test_gpu_eval._policy for RGB-D frames: the action head scaled up so that the robot falls."""
    from ballbot_rl.policies.mlp_policy import ActorCriticPolicy, obs_spaces

    torch.manual_seed(seed)
    pol = ActorCriticPolicy(obs_spaces(cameras=True, channels=4), 3, frozen_encoder=G.random_frozen_encoder(seed + 1))
    with torch.no_grad():
        pol.action_net.weight.mul_(scale)
    return pol.to(DEV).eval()


def _env(n, terrain="flat", max_ep_steps=None, seed=5):
    from ballbot_gym.envs import BallbotVecEnv

    kw = {"n_terrains": None} if terrain == "perlin" else {}
    return BallbotVecEnv(n, device=DEV, seed=seed, terrain_config={"type": terrain, "config": {}},
                         max_ep_steps=max_ep_steps, disable_cameras=False,
                         env_config={"camera": {"disable_rgb": False}},
                         stream_seeds=[seed + 100 + i for i in range(n)], **kw)


class RgbdTwin(E.Twin):
    """The stepwise twin reading each camera's four planes: the same kernels, called eagerly, no cache."""

    def features(self):
        from ballbot_rl.encoders.models import fused_encoder_forward

        env = self.env
        ext = self.policy.features_extractor.extractors
        return torch.cat([env.obs[:, 0:12], env.rel_ts.reshape(-1, 1),
                          fused_encoder_forward(ext["rgbd_0"], env.rgbd[:, 0]),
                          fused_encoder_forward(ext["rgbd_1"], env.rgbd[:, 1]), env.obs[:, 12:15]], dim=1).contiguous()


CASES = {"flat13": (8, 10, "flat", 13), "perlin60": (8, 10, "perlin", 60)}
_twins = {}


def _twin(name):
    if name not in _twins:
        n, ne, terrain, mes = CASES[name]
        pol = _policy(seed=len(name))
        env = _env(n, terrain, mes)
        assert env.cam_channels == 4
        tw = RgbdTwin(pol, env)
        rows = tw.evaluate(ne)
        print(f"twin {name}: {len(rows)} episodes in {tw.steps} steps, {tw.partial_mask_steps} steps with a partial mask")
        _twins[name] = (pol, tw, rows)
    return _twins[name]


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_the_stepwise_twin_on_rgbd(name):
    from ballbot_rl.evaluation import DeviceEvaluator, evaluate_policy

    n, ne, terrain, mes = CASES[name]
    pol, tw, rows = _twin(name)
    assert float(tw.first_feats[:, 13:53].abs().max()) > 0
    env = _env(n, terrain, mes)
    r = evaluate_policy(pol, env, n_eval_episodes=ne, fused=True, poll=1)
    assert E._rows(r) == rows and len(rows) == ne
    assert r["mean_reward"] == float(np.mean([x[0] for x in rows]))
    E._assert_same_env(env, tw.env)  # poll = 1 stops where the eager loop stops
    assert torch.equal(env.rgbd, tw.env.rgbd)
    env.close()
    env = _env(n, terrain, mes)
    ev = DeviceEvaluator(pol, env)
    r7 = ev.evaluate(ne, poll=7)
    assert E._rows(r7) == rows and tw.steps <= ev.steps < tw.steps + 7 and ev.steps % 7 == 0
    env.close()


def test_channel_mismatch_is_refused_in_both_directions():
    from ballbot_rl.evaluation import DeviceEvaluator

    depth_env = E._env(2, True)
    with pytest.raises(ValueError, match="RGB-D"):
        DeviceEvaluator(_policy(1), depth_env)
    depth_env.close()
    rgbd_env = _env(2)
    with pytest.raises(ValueError, match="RGB-D"):
        DeviceEvaluator(E._policy(True, seed=1), rgbd_env)
    rgbd_env.close()


def test_cli_on_a_synthetic_rgbd_checkpoint(tmp_path):
    from safetensors.torch import save_file

    from ballbot_rl.evaluation import save_sb3_policy_pth

    pol = _policy(seed=9)
    save_sb3_policy_pth(pol, tmp_path / "policy.pth")
    zpath = tmp_path / "ppo_agent_4096_steps.zip"
    with zipfile.ZipFile(zpath, "w") as z:
        z.writestr("data", json.dumps({"num_timesteps": 4096, "n_envs": 3, "seed": 1, "terrain_type": "flat"}))
        z.write(tmp_path / "policy.pth", "policy.pth")
        z.writestr("_stable_baselines3_version", "2.6.0")
    spath = tmp_path / "final_model.safetensors"
    save_file({k: v.contiguous() for k, v in pol.state_dict().items()}, str(spath))
    cfg = tmp_path / "config.yaml"
    cfg.write_text("num_envs: 3\nseed: 4\ncamera:\n  height: 64\n  width: 64\n  frame_rate: 90\n  disable_rgb: false\n"
                   "evaluation:\n  n_episodes: 4\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(E.ROOT / "openballbot-rl_amd"),
                                                       os.environ.get("PYTHONPATH", "")]))
    results = []
    for model in (zpath, spath):
        p = subprocess.run([sys.executable, "-m", "ballbot_rl.evaluation", "--model", str(model), "--config", str(cfg)],
                           capture_output=True, text=True, env=env, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        assert r["fused"] and len(r["episode_rewards"]) == 4 and r["episode_envs"] and r["n_envs"] == 3
        results.append(r)
    assert results[0]["episode_rewards"] == results[1]["episode_rewards"]
