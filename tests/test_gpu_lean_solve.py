"""The lean forms of the FUSE kernels' factorisation and sweeps (csrc/bb_team16.h: kLeanMax, kLeanFloor, kLeanDiag,
kLeanLtr in chol_rows and chol_solve_rows) on the GPU.

The product library against the build of the same source with the set compiled out (_native.SERIAL_FLAGS:
-DBB_NO_LEAN_SOLVE among them), bit for bit, in fp64 and fp32: one bb_step, then one 20-step bb_step_multi launch;
final state, warm start, step counters, the five output arrays of both calls and every counter of bb_get_stats.

  flat     tests/test_gpu_prephase.py's states at 1, 3, 17 and 65 envs (a lone team, partial waves, more than one
           workgroup): settled and moving, with an env that auto-resets inside the window, one that hands over to
           the full step and one started from a NaN qpos (the factorisation and the sweeps on NaN operands); fp64
           also against the oracle, one step, at that file's bounds (qpos 1e-9, qvel 1e-6 max(1, |qvel|))
  perlin   tests/test_gpu_pre_batch.py's bank with one generator per env at the same env counts
  regimes  the states with 0, 1, 13 and 14 ball-terrain contacts of the pool tests/test_gpu_solve_regimes.py builds,
           on its flat and hills terrains; fp64 one step also against the pool's oracle results
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_pre_batch as PB  # noqa: E402
import test_gpu_prephase as PP  # noqa: E402
import test_gpu_solve_regimes as SR  # noqa: E402

ENV_COUNTS = (1, 3, 17, 65)
K = 20
NG_WANTED = (0, 1, 13, 14)
PER_NG = 3  # states per terrain and contact count


@pytest.fixture(scope="module")
def libs():
    from ballbot_gym import _native as N

    assert N.SERIAL_LIB_PATH.exists(), f"{N.SERIAL_LIB_PATH} not built (__graft_entry__.build())"
    assert "-DBB_NO_LEAN_SOLVE" in N.SERIAL_FLAGS
    return N._load(N.LIB_PATH), N._load(N.SERIAL_LIB_PATH)


def _actions(seed, n):
    rng = np.random.default_rng(seed)
    a1 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    aK = rng.uniform(-1, 1, (K, n, 3)).astype(np.float32)
    return a1, aK, torch.tensor(a1, device="cuda:0"), torch.tensor(aK, device="cuda:0")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_flat_product_equals_serial_build(libs, oracle, n, precision, monkeypatch):
    O = oracle
    st = PP._states(O, n)
    kind = st[4]
    a1, _, acts1, actsK = _actions(1500 + n, n)
    got, ref = (PP._run(lib, n, precision, st, acts1, actsK, monkeypatch) for lib in libs)
    PB._assert_same(got, ref)
    done1, doneK = got["step"][2], got["multi"][2]
    for e in np.nonzero(kind == 1)[0]:
        assert doneK[3, e] & 1 and not doneK[2, e] & 1, f"env {e}: no episode end at its step limit"
    for e in np.nonzero(kind == 3)[0]:
        assert done1[e] & 4 and doneK[0, e] & 4, f"env {e}: no divergence reset from the NaN qpos"
    if (kind == 2).any():
        assert got["multi_stats"]["slow_path"] > 0, "no hand-over to the full step"
    if precision != "fp64":
        return
    hf, cfg = O.flat_hfield(), O.default_cfg(max_ep_steps=PP.MAX_EP_STEPS)
    worst_q = worst_v = 0.0
    for e in np.nonzero(kind == 0)[0]:
        qe, ve, we, se = st[0][e].copy(), st[1][e].copy(), st[2][e].copy(), np.array([st[3][e]], np.int32)
        O.env_step(cfg, qe, ve, we, se, a1[e], hf)
        worst_q = max(worst_q, float(np.abs(got["step_state"][0][e] - qe).max()))
        worst_v = max(worst_v, float(np.abs(got["step_state"][1][e] - ve).max() / max(1.0, np.abs(ve).max())))
    print(f"\n{n} envs, one step against the oracle: qpos {worst_q:.2e} qvel {worst_v:.2e}")
    assert worst_q < PP.Q_TOL and worst_v < PP.V_TOL, (worst_q, worst_v)


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_perlin_product_equals_serial_build(libs, oracle, n, precision, monkeypatch):
    _, _, acts1, actsK = _actions(1700 + n, n)
    got = PB._run_perlin(libs[0], oracle, n, precision, None, acts1, actsK, monkeypatch)
    ref = PB._run_perlin(libs[1], oracle, n, precision, got["st"], acts1, actsK, monkeypatch)
    assert np.array_equal(got["ncon"], ref["ncon"])
    PB._assert_same(got, ref)
    ng, nb = got["ncon"][:, 0], got["ncon"][:, 1]
    print(f"\n{n} perlin envs {precision}: ball-terrain contacts {sorted(ng.tolist())}, base-tree contacts on "
          f"{int((nb > 0).sum())} envs, slow_path {got['multi_stats']['slow_path']}")
    if n >= 17:
        fast = nb == 0
        assert ((ng[fast] >= 1) & (ng[fast] <= 13)).any() and (ng[fast] >= 14).any(), sorted(ng[fast].tolist())
        assert got["multi_stats"]["slow_path"] > 0, "no hand-over to the full step"


@pytest.fixture(scope="module")
def regime_pick(oracle):
    """{terrain: records} with NG_WANTED ball-terrain contacts, PER_NG of each where the pool has them."""
    states, _, _ = SR.build(oracle)
    pick = {}
    for terrain in SR.TERRAINS:
        recs = []
        for ng in NG_WANTED:
            have = [r for r in states[terrain] if r["ng"] == ng]
            assert have, f"the pool has no {terrain} state with {ng} ball-terrain contacts"
            recs += have[:PER_NG]
        pick[terrain] = recs
    return pick


def _run_regime(lib, terrain, recs, precision, acts1, actsK, monkeypatch):
    from ballbot_gym import _native as N
    from ballbot_gym.envs import BallbotVecEnv

    monkeypatch.setattr(N, "_lib", lib)
    monkeypatch.setenv("BB_ROUTE", "1")
    n = len(recs)
    env = BallbotVecEnv(n, device="cuda:0", precision=precision, seed=3, auto_reset=False,
                        terrain_config=SR._terrain_cfg(terrain))  # as the pool's own GPU step (SR._step_on_gpu)
    qs, vs, ws = SR._stack(recs, "q"), SR._stack(recs, "v"), SR._stack(recs, "w")
    steps = np.zeros(n, np.int32)
    out = {}
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
    out["multi"] = [o[k].clone().cpu().numpy() for k in PB.NAMES]
    out["multi_state"] = env.get_state()
    out["multi_stats"] = env.stats()
    env.close()
    return out


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("terrain", SR.TERRAINS)
def test_regime_states_product_equals_serial_build(libs, regime_pick, terrain, precision, monkeypatch):
    recs = regime_pick[terrain]
    n = len(recs)
    rng = np.random.default_rng(1900)
    a1 = SR._stack(recs, "a").astype(np.float32)  # the pool's own action: its oracle step is the reference below
    aK = rng.uniform(-1, 1, (K, n, 3)).astype(np.float32)
    acts1, actsK = torch.tensor(a1, device="cuda:0"), torch.tensor(aK, device="cuda:0")
    got, ref = (_run_regime(lib, terrain, recs, precision, acts1, actsK, monkeypatch) for lib in libs)
    assert np.array_equal(got["ncon"], ref["ncon"])
    PB._assert_same(got, ref)
    ng = got["ncon"][:, 0]
    print(f"\n{terrain} {precision}: ball-terrain contacts {ng.tolist()}")
    if precision != "fp64":
        return
    assert set(ng.tolist()) >= set(NG_WANTED), ng.tolist()  # the kernel counts what the oracle counted
    assert got["step_stats"]["slow_path"] == 0, "an env left the fast kernel"
    eq = np.abs(got["step_state"][0] - SR._stack(recs, "q1")).max()
    ev = np.abs(got["step_state"][1] - SR._stack(recs, "v1")).max()
    print(f"{terrain}: one step against the oracle: qpos {eq:.2e} qvel {ev:.2e}")
    assert eq < PP.Q_TOL and ev < PP.V_TOL, (eq, ev)
