"""The forward's batched LDS reads outside the Newton loop (csrc/bb_physics.h: kPreBatchRk / kPreBatchDense;
bb_step.h: rk_sums_batch, bb_team16.h: mass_dense_team<true>) on the GPU.

The product library against the build of the same source with every pre-phase form compiled out
(_native.SERIAL_FLAGS, -DBB_NO_PRE_BATCH among them: _native.SERIAL_LIB_PATH), bit for bit, in fp64 and fp32 at
1, 3, 17 and 65 envs (a lone team, partial waves, more than one workgroup): one bb_step, then one 20-step
bb_step_multi launch; final state, warm start, step counters, the five output arrays of both calls and every counter
of bb_get_stats.

  flat    tests/test_gpu_prephase.py's states: settled and moving, with an env that auto-resets inside the window,
          one that hands over to the full step and one started from a NaN qpos; fp64 also against the oracle at that
          file's bounds (one step and twenty steps: qpos 1e-9, qvel 1e-6 max(1, |qvel|))
  perlin  a bank with one generator per env; the settled robot set on its env's terrain with the ball pressed in by
          0.2 mm to 30 mm, which puts the ball-terrain contact count on both sides of 13 (the contacts whose
          Jacobians ground_setup stores in the mass blocks that mass_dense_team has just read), and envs whose base
          lies on the terrain (hand-overs)

  forms   65 flat envs, fp64: 20 bb_step calls, one bb_step_multi launch and the rollout kernel agree bit for bit
          (tests/test_gpu_solve_overhead.py's comparison on its states)
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_prephase as PP  # noqa: E402
import test_gpu_solve_overhead as OV  # noqa: E402
from test_gpu_solve_overhead import overhead_states  # noqa: E402,F401  (fixture)

ENV_COUNTS = PP.ENV_COUNTS
K = PP.K
BALL_R = 0.09  # m (csrc/bb_model.h)
PRESS = (-0.0002, -0.001, -0.002, -0.004, -0.008, -0.015, -0.03)  # m, the ball's centre below where it touches a vertex
NAMES = ("obs", "reward", "done", "terminal_obs", "pos2d")


@pytest.fixture(scope="module")
def libs():
    from ballbot_gym import _native as N

    assert N.SERIAL_LIB_PATH.exists(), f"{N.SERIAL_LIB_PATH} not built (__graft_entry__.build())"
    return N._load(N.LIB_PATH), N._load(N.SERIAL_LIB_PATH)


def _assert_same(got, ref):
    for call in ("step", "multi"):
        for name, x, y in zip(NAMES, got[call], ref[call]):
            PP._same_bits(x, y, f"{call} {name}")
        for name, x, y in zip(("qpos", "qvel", "warm", "steps"), got[call + "_state"], ref[call + "_state"]):
            PP._same_bits(x, y, f"{call} {name}")
        assert got[call + "_stats"] == ref[call + "_stats"], (call, got[call + "_stats"], ref[call + "_stats"])


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_flat_product_equals_serial_build(libs, oracle, n, precision, monkeypatch):
    O = oracle
    st = PP._states(O, n)
    kind = st[4]
    rng = np.random.default_rng(300 + n)
    a1 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    aK = rng.uniform(-1, 1, (K, n, 3)).astype(np.float32)
    acts1, actsK = torch.tensor(a1, device="cuda:0"), torch.tensor(aK, device="cuda:0")
    got, ref = (PP._run(lib, n, precision, st, acts1, actsK, monkeypatch) for lib in libs)
    _assert_same(got, ref)
    done1, doneK = got["step"][2], got["multi"][2]
    for e in np.nonzero(kind == 1)[0]:
        assert doneK[3, e] & 1 and not doneK[2, e] & 1, f"env {e}: no episode end at its step limit"
    for e in np.nonzero(kind == 3)[0]:
        assert done1[e] & 4 and doneK[0, e] & 4, f"env {e}: no divergence reset from the NaN qpos"
    if precision != "fp64":
        return
    # fp64 against the oracle: the regular envs, one step and the 20-step window
    hf, cfg = O.flat_hfield(), O.default_cfg(max_ep_steps=PP.MAX_EP_STEPS)
    worst = dict(q1=0.0, v1=0.0, qK=0.0, vK=0.0)
    for e in np.nonzero(kind == 0)[0]:
        for key, acts, state in (("1", a1[None], got["step_state"]), ("K", aK, got["multi_state"])):
            qe, ve, we, se = st[0][e].copy(), st[1][e].copy(), st[2][e].copy(), np.array([st[3][e]], np.int32)
            for a in acts:
                _, _, fl, _, _ = O.env_step(cfg, qe, ve, we, se, a[e], hf)
                assert not fl & 1, f"env {e}: the oracle's episode ended inside the window"
            eq = float(np.abs(state[0][e] - qe).max())
            ev = float(np.abs(state[1][e] - ve).max() / max(1.0, np.abs(ve).max()))
            worst["q" + key], worst["v" + key] = max(worst["q" + key], eq), max(worst["v" + key], ev)
    print(f"\n{n} envs against the oracle: one step qpos {worst['q1']:.2e} qvel {worst['v1']:.2e}; "
          f"{K} steps qpos {worst['qK']:.2e} qvel {worst['vK']:.2e}")
    assert worst["q1"] < PP.Q_TOL and worst["qK"] < PP.Q_TOL, worst
    assert worst["v1"] < PP.V_TOL and worst["vK"] < PP.V_TOL, worst


def _on_terrain(env, O, n):
    """(qpos, qvel, warm, steps, handover) for n envs of a perlin env: the settled robot moved about its env's
    terrain and set where the ball touches the highest vertex under it, then pressed in by PRESS[e % 7] (the base
    moves with the ball); every sixth env (from env 2 on) lies on the terrain
    with its base, the ball beside it."""
    rng = np.random.default_rng(23)
    hf0, cfg = O.flat_hfield(), O.default_cfg()
    q, v, w = O.reset_state(0.01)
    sc = np.zeros(1, np.int32)
    for _ in range(60):  # settled but moving (flat; the offset to the terrain is added below)
        O.env_step(cfg, q, v, w, sc, rng.uniform(-1, 1, 3).astype(np.float32), hf0)
    size_z = float(env.terrain_plan.size_z)
    slots, _ = env.env_terrain()
    qs, ws = np.tile(q, (n, 1)), np.tile(w, (n, 1))
    vs = np.tile(v, (n, 1)) + rng.normal(0, 0.05, (n, 15))
    handover = np.zeros(n, bool)
    gy, gx = np.meshgrid(np.arange(-4, 5), np.arange(-4, 5), indexing="ij")
    for e in range(n):
        hf = env.hfield(int(slots[e])).reshape(293, 293)
        x, y = rng.uniform(-3, 3, 2)
        qs[e, [0, 10]] += x
        qs[e, [1, 11]] += y
        # the height at which the ball (radius BALL_R) touches the highest of the vertices under it
        r, c = int(round((qs[e, 11] + 5) / 10 * 292)), int(round((qs[e, 10] + 5) / 10 * 292))
        d2 = (((r + gy) / 292 * 10 - 5 - qs[e, 11]) ** 2 + ((c + gx) / 292 * 10 - 5 - qs[e, 10]) ** 2)
        h = hf[r - 4:r + 5, c - 4:c + 5].astype(np.float64) * size_z
        rest = float(np.max(np.where(d2 < BALL_R ** 2, h + np.sqrt(np.maximum(BALL_R ** 2 - d2, 0.0)), -np.inf)))
        if e % 6 == 2:
            handover[e] = True
            t = np.radians(75.0 + e % 7)
            qs[e, 3:7] = [np.cos(t / 2), np.sin(t / 2), 0, 0]
            qs[e, 2] = rest - BALL_R + 0.06
            qs[e, 10:13] = [qs[e, 0] + 0.7, qs[e, 1] - 0.4, rest + 0.8]
            qs[e, 13:17] = [1, 0, 0, 0]
            ws[e] = 0
        else:
            dz = rest + PRESS[e % len(PRESS)] - BALL_R  # from where the settled state rests on the flat ground
            qs[e, 2] += dz
            qs[e, 12] += dz
    return qs, vs, ws, np.zeros(n, np.int32), handover


def _run_perlin(lib, O, n, precision, st, acts1, actsK, monkeypatch):
    from ballbot_gym import _native as N
    from ballbot_gym.envs import BallbotVecEnv

    monkeypatch.setattr(N, "_lib", lib)
    monkeypatch.setenv("BB_ROUTE", "1")  # multi_step_kernel, hand-overs finished by the full step
    env = BallbotVecEnv(n, device="cuda:0", precision=precision, seed=3, max_ep_steps=PP.MAX_EP_STEPS,
                        terrain_config={"type": "perlin", "config": {}}, n_terrains=None,
                        stream_seeds=[50 + i for i in range(n)])
    if st is None:
        st = _on_terrain(env, O, n)
    qs, vs, ws, steps, _ = st
    out = {"st": st}
    env.set_state(qs, vs, ws, steps)
    out["ncon"] = env.forward(np.zeros(3))[1].copy()
    env.set_state(qs, vs, ws, steps)
    obs, rew, _, _, info = env.step(acts1)
    out["step"] = [x.clone().cpu().numpy() for x in (obs, rew, info["done_flags"], info["terminal_observation"],
                                                    info["pos2d"])]
    out["step_state"] = env.get_state()
    out["step_stats"] = env.stats()
    env.set_state(qs, vs, ws, steps)
    o = env.step_multi(actsK)
    out["multi"] = [o[k].clone().cpu().numpy() for k in NAMES]
    out["multi_state"] = env.get_state()
    out["multi_stats"] = env.stats()
    env.close()
    return out


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_perlin_product_equals_serial_build(libs, oracle, n, precision, monkeypatch):
    rng = np.random.default_rng(500 + n)
    a1 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    aK = rng.uniform(-1, 1, (K, n, 3)).astype(np.float32)
    acts1, actsK = torch.tensor(a1, device="cuda:0"), torch.tensor(aK, device="cuda:0")
    got = _run_perlin(libs[0], oracle, n, precision, None, acts1, actsK, monkeypatch)
    ref = _run_perlin(libs[1], oracle, n, precision, got["st"], acts1, actsK, monkeypatch)
    assert np.array_equal(got["ncon"], ref["ncon"])
    _assert_same(got, ref)
    ng, nb, handover = got["ncon"][:, 0], got["ncon"][:, 1], got["st"][4]
    print(f"\n{n} perlin envs {precision}: ball-terrain contacts {sorted(ng.tolist())}, base-tree contacts on "
          f"{int((nb > 0).sum())} envs, slow_path {got['multi_stats']['slow_path']}")
    if n >= 17:  # the directed envs did what they are there for
        fast = nb == 0  # the fast kernel's envs
        assert ((ng[fast] >= 1) & (ng[fast] <= 13)).any() and (ng[fast] >= 14).any(), sorted(ng[fast].tolist())
        assert (nb[handover] > 0).any(), nb[handover]
        assert got["multi_stats"]["slow_path"] > got["step_stats"]["slow_path"] > 0, "no hand-over to the full step"


def test_launch_forms_bit_equal(overhead_states, monkeypatch):  # noqa: F811
    """65 flat envs x 20 steps from tests/test_gpu_solve_overhead.py's states: the rollout kernel (not a FUSE kernel:
    the serial text), 20 bb_step calls and one bb_step_multi launch (both with the batched forms)."""
    OV.test_launch_forms_bit_equal(overhead_states, monkeypatch)
