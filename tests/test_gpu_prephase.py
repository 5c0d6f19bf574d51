"""The forward's twin forms and once-per-launch model terms (csrc/bb_physics.h, bb_step.h) on the GPU.

The product library against the build of the same source with the four items compiled out
(-DBB_NO_TWIN_KIN -DBB_NO_TWIN_POS -DBB_NO_TWIN_BIAS -DBB_NO_MODEL_ONCE, _native.SERIAL_LIB_PATH: the serial
pre-phase every lane computed before), on flat terrain in fp64 and fp32: one bb_step, then one 20-step
bb_step_multi launch, at 1, 3, 17 and 65 envs (a lone team, partial waves, more than one workgroup).  Final
state, warm start and step counters, the five output arrays of both calls and every counter of bb_get_stats
(solver_iters among them) must be equal bit for bit.  A partial wave has exited teams beside live ones: the
new team_sync after the twin position update is passed by the live teams alone, and the run ending with equal
bits at 1 and 3 envs is the check of that.

Among the envs (where the count leaves room): one four steps from its episode's step limit (auto-reset inside
the window), one whose base lies on the ground (the fast path hands it over: parked by the multi-step
launch, its start state restored, and finished by the full step), and one started from a NaN qpos
(MuJoCo's divergence reset at the step's start).

fp64 against the oracle, at the tolerances of tests/test_gpu_parity.py (qpos 1e-9, qvel 1e-6 max(1, |qvel|)):
the single step on every env but the NaN one, and the 20-step window on the envs that neither reset nor hand
over (the oracle steps an episode, not a vectorised env with auto-reset).  The hand-over env topples, so its
episode ends and it auto-resets: its terminal observation (1e-6, as there) stands in for its state.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ENV_COUNTS = (1, 3, 17, 65)
K = 20
MAX_EP_STEPS = 400
Q_TOL, V_TOL, OBS_TOL = 1e-9, 1e-6, 1e-6


def _states(O, n):
    """(qpos, qvel, warm, steps, kind) for n envs; kind: 0 regular, 1 auto-reset in the window, 2 hand-over,
    3 NaN qpos."""
    rng = np.random.default_rng(11)
    hf, cfg = O.flat_hfield(), O.default_cfg()
    q, v, w = O.reset_state(0.01)
    sc = np.zeros(1, np.int32)
    for _ in range(60):  # settled but moving
        O.env_step(cfg, q, v, w, sc, rng.uniform(-1, 1, 3).astype(np.float32), hf)
    qs, ws = np.tile(q, (n, 1)), np.tile(w, (n, 1))
    vs = np.tile(v, (n, 1)) + rng.normal(0, 0.05, (n, 15))
    steps = np.full(n, int(sc[0]), np.int32)
    kind = np.zeros(n, np.int32)
    special = {3: {1: 3, 2: 2}, 17: {5: 1, 9: 2, 13: 3}, 65: {5: 1, 9: 2, 13: 3, 40: 1, 50: 2, 64: 3}}.get(n, {})
    for e, kd in special.items():
        kind[e] = kd
        if kd == 1:
            steps[e] = MAX_EP_STEPS - 4
        elif kd == 2:  # the base rolled onto the ground, the ball beside it (tests/test_gpu_parity.py)
            t = np.radians(75.0 + e % 7)  # the tower's lowest point 0.03 below the ground
            qs[e, 3:7] = [np.cos(t / 2), np.sin(t / 2), 0, 0]
            qs[e, 2] = 0.06
            qs[e, 10:13] = [0.7, -0.4, 0.5]
            qs[e, 13:17] = [1, 0, 0, 0]
            ws[e] = 0
        else:
            qs[e, 4] = np.nan
    return qs, vs, ws, steps, kind


def _run(lib, n, precision, st, acts1, actsK, monkeypatch):
    from ballbot_gym import _native as N
    from ballbot_gym.envs import BallbotVecEnv

    monkeypatch.setattr(N, "_lib", lib)
    monkeypatch.setenv("BB_ROUTE", "1")  # fast kernel, then the full kernel over its hand-overs
    env = BallbotVecEnv(n, device="cuda:0", precision=precision, seed=3, max_ep_steps=MAX_EP_STEPS,
                        terrain_config={"type": "flat", "config": {}})
    qs, vs, ws, steps, _ = st
    out = {}
    env.set_state(qs, vs, ws, steps)
    obs, rew, _, _, info = env.step(acts1)
    out["step"] = [x.clone().cpu().numpy() for x in (obs, rew, info["done_flags"], info["terminal_observation"],
                                                    info["pos2d"])]
    out["step_state"] = env.get_state()
    out["step_stats"] = env.stats()
    env.set_state(qs, vs, ws, steps)
    o = env.step_multi(actsK)
    out["multi"] = [o[k].clone().cpu().numpy() for k in ("obs", "reward", "done", "terminal_obs", "pos2d")]
    out["multi_state"] = env.get_state()
    out["multi_stats"] = env.stats()
    env.close()
    return out


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bad = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
    assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at {tuple(bad[0][:-1])}"


@pytest.fixture(scope="module")
def libs():
    from ballbot_gym import _native as N

    assert N.SERIAL_LIB_PATH.exists(), f"{N.SERIAL_LIB_PATH} not built (__graft_entry__.build())"
    return N._load(N.LIB_PATH), N._load(N.SERIAL_LIB_PATH)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_product_equals_serial_build(libs, oracle, n, precision, monkeypatch):
    O = oracle
    st = _states(O, n)
    kind = st[4]
    rng = np.random.default_rng(100 + n)
    a1 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    aK = rng.uniform(-1, 1, (K, n, 3)).astype(np.float32)
    acts1, actsK = torch.tensor(a1, device="cuda:0"), torch.tensor(aK, device="cuda:0")
    got, ref = (_run(lib, n, precision, st, acts1, actsK, monkeypatch) for lib in libs)
    names = ("obs", "reward", "done", "terminal_obs", "pos2d")
    for call in ("step", "multi"):
        for name, x, y in zip(names, got[call], ref[call]):
            _same_bits(x, y, f"{call} {name}")
        for name, x, y in zip(("qpos", "qvel", "warm", "steps"), got[call + "_state"], ref[call + "_state"]):
            _same_bits(x, y, f"{call} {name}")
        assert got[call + "_stats"] == ref[call + "_stats"], (call, got[call + "_stats"], ref[call + "_stats"])
    # the directed envs did what they are there for
    done1, doneK = got["step"][2], got["multi"][2]
    stats = got["multi_stats"]
    for e in np.nonzero(kind == 1)[0]:
        assert doneK[3, e] & 1 and not doneK[2, e] & 1, f"env {e}: no episode end at its step limit"
        assert got["multi_state"][3][e] == K - 4, f"env {e}: step counter after the auto-reset"
    for e in np.nonzero(kind == 3)[0]:
        assert done1[e] & 4 and doneK[0, e] & 4, f"env {e}: no divergence reset from the NaN qpos"
        assert np.isfinite(got["multi_state"][0][e]).all() and np.isfinite(got["multi_state"][1][e]).all()
    if (kind == 2).any():
        assert stats["slow_path"] > got["step_stats"]["slow_path"] > 0, "no hand-over to the full step"
    else:
        assert stats["slow_path"] == 0
    assert stats["resets"] >= int((kind == 1).sum())
    if precision != "fp64":
        for call in ("step", "multi"):
            for x in got[call + "_state"][:3]:
                assert np.isfinite(x).all()
        return
    # fp64 against the oracle
    hf, cfg = O.flat_hfield(), O.default_cfg(max_ep_steps=MAX_EP_STEPS)
    worst = dict(q1=0.0, v1=0.0, qK=0.0, vK=0.0, obs_handover=0.0)
    q1, v1 = got["step_state"][0], got["step_state"][1]
    qK, vK = got["multi_state"][0], got["multi_state"][1]
    for e in range(n):
        if kind[e] == 3:
            continue
        qe, ve, we, se = st[0][e].copy(), st[1][e].copy(), st[2][e].copy(), np.array([st[3][e]], np.int32)
        o, _, fl, _, _ = O.env_step(cfg, qe, ve, we, se, a1[e], hf)
        if kind[e] == 2:
            # toppled: the episode ends and the env auto-resets, so the state is gone; the terminal
            # observation is the full step's, from the restored start state (multi: parked, then finished)
            assert fl & 1 and done1[e] & 1
            qe, ve, we, se = st[0][e].copy(), st[1][e].copy(), st[2][e].copy(), np.array([st[3][e]], np.int32)
            oK, _, _, _, _ = O.env_step(cfg, qe, ve, we, se, aK[0, e], hf)
            eo = max(np.abs(got["step"][3][e] - o).max(), np.abs(got["multi"][3][0, e] - oK).max())
            worst["obs_handover"] = max(worst["obs_handover"], float(eo))
            continue
        eq, ev = np.abs(q1[e] - qe).max(), np.abs(v1[e] - ve).max() / max(1.0, np.abs(ve).max())
        worst["q1"], worst["v1"] = max(worst["q1"], eq), max(worst["v1"], ev)
        if kind[e] != 0:
            continue
        qe, ve, we, se = st[0][e].copy(), st[1][e].copy(), st[2][e].copy(), np.array([st[3][e]], np.int32)
        for k in range(K):
            _, _, fl, _, _ = O.env_step(cfg, qe, ve, we, se, aK[k, e], hf)
            assert not fl & 1, f"env {e}: the oracle's episode ended inside the window"
        eq, ev = np.abs(qK[e] - qe).max(), np.abs(vK[e] - ve).max() / max(1.0, np.abs(ve).max())
        worst["qK"], worst["vK"] = max(worst["qK"], eq), max(worst["vK"], ev)
    print(f"\n{n} envs against the oracle: one step qpos {worst['q1']:.2e} qvel {worst['v1']:.2e}; "
          f"{K} steps qpos {worst['qK']:.2e} qvel {worst['vK']:.2e}; hand-over terminal obs {worst['obs_handover']:.2e}")
    assert worst["q1"] < Q_TOL and worst["qK"] < Q_TOL, worst
    assert worst["v1"] < V_TOL and worst["vK"] < V_TOL, worst
    assert worst["obs_handover"] < OBS_TOL, worst
