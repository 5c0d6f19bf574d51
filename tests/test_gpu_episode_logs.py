"""The reference's per-episode logs from the batched env: the recorder
kernel bb_reward_terms, bb_rollout's buf_terminal_obs / buf_flags, the files of
BallbotVecEnv.flush_logs() and BBotSimulation, and the trainer's hook.

What is held to what:
- the two terms are the step kernels' own floats: fl32(fl32(t1 + t2) + survival_bonus) ==
  reward bit for bit (no bonus on a failure step), on every row of a window with failure
  rows, time-limit rows and an unfinished tail, at the project's ragged env counts;
- independently, term_1 against torch eager float32 ops on the terminal observation (bit
  equal: every op is one correctly rounded IEEE operation and the kernel does not contract),
  term_2 within relative 1e-6 of coef * |a|^2 in float64 (about 8 float32 ulp: a square root
  that is 1 ulp off, squared and scaled);
- one K = 7 launch against seven K = 1 launches: bit-identical histories and bookkeeping;
- bb_rollout with the two optional buffers attached against the same launch without them
  (every other output bit-identical), on a flat bank (rollout_kernel and its finish launch)
  and on a perlin bank (the relief pair with the policy in it);
- the files against the device history and against the envs' own terrain draw sequences.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TARGET = [0.6, 0.8]  # not an axis: both products of term_1 are live
REWARD = {"type": "directional", "config": {"target_direction": TARGET}}


def _env(n, terrain="flat", log=None, **kw):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device=DEV, seed=11, precision="fp64", reward_config=REWARD,
                         terrain_config={"type": terrain, "config": {}}, log_options=log, **kw)


def _tilt(env, idx):
    """Tilt the base of envs `idx` by 30 degrees: their next step ends in failure (tilt > 20)."""
    q, v, w, s = env.get_state()
    t = np.radians(30.0)
    q[idx, 3:7] = [np.cos(t / 2), *(np.sin(t / 2) * np.array([0.6, 0.8, 0.0]))]
    env.set_state(q, v, w, s)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_identity(env, terms, reward, flags):
    """reward == fl32(fl32(t1 + t2) + bonus), without the bonus where the failure bit is set."""
    bonus = torch.tensor(env._params.survival_bonus, dtype=torch.float32, device=DEV)
    s = terms[..., 0] + terms[..., 1]
    want = torch.where((flags & 2) != 0, s, s + bonus)
    assert torch.equal(_bits(want), _bits(reward)), (want - reward).abs().max()


@pytest.mark.parametrize("n", [1, 3, 17, 65])
def test_terms_are_the_steps_own_floats(n, tmp_path):
    K = 7
    log = {"reward_terms": True, "dir": str(tmp_path / "a")}
    a = _env(n, log=log, max_ep_steps=3)
    b = _env(n, log={**log, "dir": str(tmp_path / "b")}, max_ep_steps=3)
    tilted = [0] if n == 1 else [0, n - 1]
    for e in (a, b):
        _tilt(e, tilted)
    acts = torch.rand(K, n, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) * 2 - 1
    out = a.step_multi(acts)
    rew, fl, tobs = [], [], []
    for k in range(K):
        _, r, _, _, info = b.step(acts[k])
        rew.append(r.clone()); fl.append(info["done_flags"].clone()); tobs.append(info["terminal_observation"].clone())
    rew, fl, tobs = torch.stack(rew), torch.stack(fl), torch.stack(tobs)
    # the K = 7 launch and the seven K = 1 launches: the same steps, histories and bookkeeping
    assert torch.equal(_bits(out["reward"]), _bits(rew)) and torch.equal(out["done"], fl)
    assert torch.equal(_bits(out["terminal_obs"]), _bits(tobs))
    ha, last_a, eps_a = a.log_state()
    hb, last_b, eps_b = b.log_state()
    assert ha.shape == (K, n, 2) and hb.shape == (K, n, 2)
    assert torch.equal(_bits(ha), _bits(hb))
    np.testing.assert_array_equal(last_a, last_b)
    np.testing.assert_array_equal(eps_a, eps_b)
    # the window holds failure rows, time-limit rows and an unfinished tail
    term, fail = (fl & 1) != 0, (fl & 2) != 0
    assert bool(fail.any()) and bool((term & ~fail).any())
    assert bool(fail[0, tilted].all())
    rest = [e for e in range(n) if e not in tilted]  # terminal at rows 2 and 5, row 6 an unfinished tail
    assert bool(term[[2, 5]][:, rest].all()) and not bool(term[K - 1, rest].any())
    fl_h = fl.cpu().numpy()
    for e in range(n):
        rows = np.nonzero(fl_h[:, e] & 1)[0]
        assert len(rows) >= 2 and eps_a[e] == len(rows) and last_a[e] == rows[-1] + 1
    _check_identity(a, ha, rew, fl)
    # independent: torch eager float32 ops (one rounding each) on the terminal observation
    p = a._params
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)  # noqa: E731
    t1 = (tobs[..., 12] * f32(p.target_dir[0]) + tobs[..., 13] * f32(p.target_dir[1])) * f32(p.reward_scale)
    assert torch.equal(_bits(t1), _bits(ha[..., 0]))
    act = tobs[..., 0:3].double()
    t2 = float(p.action_reg_coef) * (act * act).sum(-1)
    assert bool(((ha[..., 1].double() - t2).abs() <= 1e-6 * t2.abs()).all())
    assert bool((ha[..., 1] != 0).any()) and bool((ha[..., 0] != 0).any())
    a.close(); b.close()


def _ppo(env, T, seed=4):
    from ballbot_rl.training.logger import CSVLogger
    from ballbot_rl.training.ppo import BatchedPPO, fused_mlp_slots

    m = BatchedPPO(env, n_steps=T, batch_size=256, n_epochs=1, seed=seed, logger=CSVLogger(None, stdout=False))
    with torch.no_grad():  # a non-trivial policy
        for p in m.policy.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    slots = fused_mlp_slots(m, update=False)
    assert slots
    return m, slots


@pytest.mark.parametrize("terrain", ["flat", "perlin"])
@pytest.mark.parametrize("n", [3, 65])
def test_rollout_keeps_terminal_obs_and_flags(n, terrain, tmp_path):
    """flat: rollout_kernel and its finish launch; perlin: the relief pair with the policy in it."""
    T = 4
    kw = {"max_ep_steps": 3}
    if terrain == "perlin":
        kw.update(n_terrains=4, shared_stream=True)  # a small bank: the 4 first draws of one generator
    a = _env(n, terrain, log={"reward_terms": True, "dir": str(tmp_path)}, **kw)
    b = _env(n, terrain, **kw)
    assert a.relief == (terrain == "perlin")
    res = []
    for env in (a, b):
        _tilt(env, [0])
        m, slots = _ppo(env, T)
        m._last_obs = env.obs
        m._last_starts.fill_(1)
        ep_r, ep_l = m._collect_rollout_kernel(slots)
        torch.cuda.synchronize()
        res.append((m, ep_r, ep_l))
    (ma, ep_r, ep_l), (mb, ep_r_b, ep_l_b) = res
    assert getattr(mb, "_log_tobs", None) is None  # the twin ran with the two fields NULL
    flags, tobs, buf = ma._log_flags, ma._log_tobs, ma.buf
    done = (flags & 1) != 0
    assert torch.equal(done, ep_l != 0)
    # the tilted env fails at once (then runs to its time limit at row 3); the others end at row 2
    assert bool(done[2, 1:].all()) and bool(done[0, 0]) and bool((flags[0, 0] & 2) != 0) and bool(done[3, 0])
    hist, last, eps = a.log_state()
    assert hist.shape == (T, n, 2)
    _check_identity(a, hist, buf.rewards, flags)
    nxt = torch.cat([buf.obs[1:], a.obs[None]])  # the observation the next step (or the caller) saw
    keep = ~done
    assert torch.equal(_bits(tobs[keep]), _bits(nxt[keep]))
    assert bool((nxt[done] == 0).all())  # ... the reset observation where the episode ended
    assert torch.equal(_bits(tobs[done][:, 0:3]), _bits(buf.actions.clamp(-1.0, 1.0)[done]))
    fl_h = flags.cpu().numpy()
    for e in range(n):
        rows = np.nonzero(fl_h[:, e] & 1)[0]
        assert eps[e] == len(rows) and last[e] == rows[-1] + 1
    # with the two fields NULL every other output of the launch is the same, bit for bit
    bb = mb.buf
    for x, y in ((buf.obs, bb.obs), (buf.actions, bb.actions), (buf.values, bb.values),
                 (buf.log_probs, bb.log_probs), (buf.rewards, bb.rewards), (a.obs, b.obs)):
        assert torch.equal(_bits(x), _bits(y))
    assert torch.equal(buf.starts, bb.starts) and torch.equal(ep_l, ep_l_b)
    assert torch.equal(ep_r.view(torch.int64), ep_r_b.view(torch.int64))
    assert torch.equal(ma._last_starts, mb._last_starts) and torch.equal(ma._ep_ret, mb._ep_ret)
    for x, y in zip(a.get_state(), b.get_state()):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a.env_terrain(), b.env_terrain()):
        np.testing.assert_array_equal(x, y)
    assert a.stats() == b.stats()
    a.close(); b.close()


def _mtimes(root):
    return {os.path.join(d, f): os.stat(os.path.join(d, f)).st_mtime_ns for d, _, fs in os.walk(root) for f in fs}


def test_files_after_flush(tmp_path):
    from ballbot_gym.envs.config import stream_draws

    n, first = 5, 300
    env = _env(n, "perlin", log={"reward_terms": True, "terrain_seeds": True, "dir": str(tmp_path)}, max_ep_steps=8,
               n_terrains=6, first_env=first)
    gen = torch.Generator(device=DEV).manual_seed(1)
    for _ in range(5):  # 40 steps: five episodes of 8 steps per env
        env.step_multi((torch.rand(8, n, 3, device=DEV, generator=gen) * 2 - 1) * 0.3)
    assert list(tmp_path.iterdir()) == []  # files are current after flush_logs(), not after every step
    env.flush_logs()
    hist, last, eps = env.log_state()
    assert hist.shape == (40, n, 2) and last.tolist() == [40] * n and eps.tolist() == [5] * n
    assert sorted(p.name for p in tmp_path.iterdir()) == [f"env_{first + e:05d}" for e in range(n)]
    hist_h = hist.cpu().numpy()
    _, draws = env.env_terrain()
    _, last_seed = env.terrain_rng()
    for e in range(n):
        d = tmp_path / f"env_{first + e:05d}"
        for c, name in enumerate(("term_1.npy", "term_2.npy")):
            t = np.load(d / name)
            assert t.dtype == np.float32 and t.shape == (40,)
            assert t.tobytes() == np.ascontiguousarray(hist_h[:40, e, c]).tobytes()
        want = stream_draws(env.terrain_plan.stream_seeds[e], 6)
        assert (d / "terrain_seed_history").read_text() == "".join(f"{int(s)}\n" for s in want[:5])
        assert draws[e] == 6 and last_seed[e] == want[5]  # the device drew what the file says, and one more
    before = _mtimes(tmp_path)
    env.flush_logs()  # no new episode: nothing is rewritten
    env.step_multi(torch.zeros(3, n, 3, device=DEV))
    env.flush_logs()  # new steps but no new episode
    assert _mtimes(tmp_path) == before
    env.step_multi(torch.zeros(5, n, 3, device=DEV))
    env.close()  # close() flushes: the sixth episode
    for e in range(n):
        d = tmp_path / f"env_{first + e:05d}"
        assert np.load(d / "term_1.npy").shape == (48,)
        assert len((d / "terrain_seed_history").read_text().split()) == 6


def test_only_the_listed_envs_log(tmp_path):
    env = _env(17, log={"reward_terms": True, "envs": [2, 16], "dir": str(tmp_path)}, max_ep_steps=3)
    env.step_multi(torch.zeros(4, 17, 3, device=DEV))
    env.flush_logs()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["env_00002", "env_00016"]
    hist = env.log_state()[0].cpu().numpy()
    assert np.load(tmp_path / "env_00016" / "term_2.npy").tobytes() == np.ascontiguousarray(hist[:3, 16, 1]).tobytes()
    assert not (tmp_path / "env_00002" / "terrain_seed_history").exists()  # flat, and the switch is off
    env.close()


def test_single_env_logs(tmp_path):
    import string

    from ballbot_gym.envs.ballbot_env import BBotSimulation
    from ballbot_gym.envs.config import np_random
    from test_episode_logs_host import _decode_png

    sim = BBotSimulation(log_options={"cams": True, "reward_terms": True, "dir": str(tmp_path)},
                         disable_cameras=False, max_ep_steps=13, terrain_type="perlin", reward_config=REWARD)
    sim.reset(seed=3)
    g = np_random(3)
    g.integers(0, 10000)
    name = "log_" + "".join(g.permutation(list(string.ascii_letters + string.digits))[:12])
    assert sim.log_dir == str(tmp_path / name) and os.path.isdir(sim.log_dir)
    d = tmp_path / name
    seeds, rewards = [], []
    for ep in range(2):
        if ep:
            sim.reset()
        seeds.append(sim.last_r_seed)
        frames = []
        for t in range(1, 14):
            obs, r, term, trunc, info = sim.step(np.array([0.3, -0.2, 0.1], np.float32))
            rewards.append(np.float32(r))
            assert term == (t == 13) and not info["failure"]
            if t in (6, 12):
                assert float(obs["relative_image_timestamp"][0]) == 0.0
                frames.append((obs["rgbd_0"].copy(), obs["rgbd_1"].copy()))
        depth = d / f"rgbd_log_episode_{ep}" / "depth"
        assert sorted(p.name for p in depth.iterdir()) == ["depth_a_0.png", "depth_a_1.png", "depth_b_0.png",
                                                           "depth_b_1.png"]
        assert (d / f"rgbd_log_episode_{ep}" / "rgb").is_dir()
        for i, (f0, f1) in enumerate(frames):
            assert np.array_equal(_decode_png(depth / f"depth_a_{i}.png"), (f0[0] * 255).astype("uint8"))
            assert np.array_equal(_decode_png(depth / f"depth_b_{i}.png"), (f1[0] * 255).astype("uint8"))
        t1, t2 = np.load(d / "term_1.npy"), np.load(d / "term_2.npy")
        assert t1.dtype == np.float32 and t1.shape == t2.shape == (13 * (ep + 1),)  # never cleared: the quirk
        want = (t1 + t2) + np.float32(0.02)
        assert want.astype(np.float32).tobytes() == np.asarray(rewards, np.float32).tobytes()
        assert (d / "terrain_seed_history").read_text() == "".join(f"{s}\n" for s in seeds)
    sim.close()


def test_single_env_without_switches_creates_no_directory(tmp_path):
    from ballbot_gym.envs.ballbot_env import BBotSimulation

    sim = BBotSimulation(log_options={"cams": False, "reward_terms": False, "dir": str(tmp_path)},
                         disable_cameras=True, max_ep_steps=2, terrain_type="flat")
    sim.reset(seed=1)
    for _ in range(2):
        _, _, term, _, _ = sim.step(np.zeros(3, np.float32))
    assert term and sim.log_dir is None and list(tmp_path.iterdir()) == []
    sim.close()


def _train(tmp_path, log):
    from ballbot_rl.training.logger import CSVLogger
    from ballbot_rl.training.ppo import BatchedPPO

    env = _env(17, log=log, max_ep_steps=3)
    m = BatchedPPO(env, n_steps=4, batch_size=34, n_epochs=1, seed=9, logger=CSVLogger(None, stdout=False))
    m.warm_up()
    m.learn(total_timesteps=2 * 17 * 4)
    torch.cuda.synchronize()
    return env, m


@pytest.mark.parametrize("fused", ["1", "0"])
def test_trainer_records_and_flushes(fused, tmp_path, monkeypatch):
    """fused 1: the rollout is one bb_rollout launch with buf_terminal_obs / buf_flags attached;
    0: the per-step rollout captured as one HIP graph, the recorder's launches inside it."""
    monkeypatch.setenv("BB_FUSED_ROLLOUT", fused)
    env, m = _train(tmp_path, {"reward_terms": True, "dir": str(tmp_path)})
    ref_env, ref = _train(tmp_path, None)
    assert (m._rgraph is None) == (fused == "1")
    hist, last, eps = env.log_state()
    assert hist.shape == (8, 17, 2)  # two rollouts of four steps: nothing from warm_up()
    assert last.tolist() == [6] * 17 and eps.tolist() == [2] * 17
    hist_h = hist.cpu().numpy()
    for e in range(17):  # learn() flushed: the files exist and hold the history up to step 6
        t1 = np.load(tmp_path / f"env_{e:05d}" / "term_1.npy")
        assert t1.tobytes() == np.ascontiguousarray(hist_h[:6, e, 0]).tobytes()
    # (no env fails within three steps on flat ground: without the rollout's flag buffer, no failure bits)
    flags = m._log_flags if fused == "1" else torch.zeros(4, 17, dtype=torch.uint8, device=DEV)
    _check_identity(env, hist[4:], m.buf.rewards, flags)
    for name in ("obs", "actions", "values", "log_probs", "rewards", "advantages", "returns"):
        assert torch.equal(_bits(getattr(m.buf, name)), _bits(getattr(ref.buf, name))), name
    assert torch.equal(m.buf.starts, ref.buf.starts)
    assert torch.equal(_bits(m.optimizer.flat), _bits(ref.optimizer.flat))
    assert not hasattr(ref_env, "_log_hist") and getattr(ref, "_log_tobs", None) is None
    env.close(); ref_env.close()


def test_log_options_that_are_refused(tmp_path):
    import ctypes as C

    from ballbot_gym import _native as N
    from ballbot_gym.envs import BallbotVecEnv

    with pytest.raises(ValueError, match="single-env feature"):
        _env(3, log={"cams": True, "dir": str(tmp_path)})
    dist = {"type": "distance", "config": {"goal_position": [1.0, 0.0]}}
    with pytest.raises(ValueError, match="directional reward"):
        BallbotVecEnv(3, device=DEV, reward_config=dist, reward_compat="fused",
                      log_options={"reward_terms": True, "dir": str(tmp_path)})
    # env_config's logging section overrides log_options (as the reference's constructor does)
    env = _env(3, log={"reward_terms": True, "dir": str(tmp_path)}, env_config={"logging": {"reward_terms": False}})
    assert env.log_dir is None and not env._log_on
    env.close()
    assert list(tmp_path.iterdir()) == []  # no switch on, no directory
    # the kernel itself refuses a handle whose reward is not the directional one
    env = BallbotVecEnv(3, device=DEV, reward_config=dist, reward_compat="fused")
    t = torch.zeros(64, device=DEV)
    book = torch.zeros(8, dtype=torch.int64, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert N.lib().bb_reward_terms(env._h, p(t), p(env.done), 1, p(t), 1, p(book), None) < 0
    assert "not BB_REWARD_DIRECTIONAL" in N.last_error()
    env.close()
