"""The fast kernels' solve with jar and M a carried across the Newton iterations (bb_team16.h:solve16), at 1 to 8
envs.

States (flat ground, built on the CPU with the oracle, as tests/test_host_solve_carry.py scans them): one per
ball-terrain contact count 0, 1, 6, 13, 14 and 30 -- none, one, a typical count, the last count at which every
contact is some lane's first (the carried one; their Jacobians are the stored ones, GC_LDS = 13), the first with a
contact of a second round beside them (rebuilt from a at every use), and a lane's third contact -- the one with the
most Newton iterations of each count, plus the two longest solves of the scan; at least 2 of them take 10 iterations
or more.

  ng boundaries   one fast-kernel step and one full-kernel forward against the oracle, with the tolerances and the
                  allowance (no outlier) of tests/test_gpu_solve_regimes.py for the same quantities
  mixed wave      ng = (0, 6, 13, 14) in one wave of 4, and 1, 3 and 5 envs: bit-equal to every env stepped alone
  forms agree     bb_step_multi with K = 3 against three bb_step calls: states and all five outputs bit-equal

On an MI355X the 8 states (ng 0, 1, 6, 13, 14, 30, 35, 28; 13, 9, 12, 13, 10, 11, 15, 14 iterations) step within
qpos 2.6e-13, qvel 1.9e-10, warm start 1.4e-9 of the oracle; the full kernel's forward within 9.9e-10.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_solve_regimes as R  # noqa: E402

NG_WANTED = (0, 1, 6, 13, 14, 30)
LONG_ITERS, MIN_LONG = 10, 2


@pytest.fixture(scope="module")
def carry_states(oracle):
    """Up to 8 state records (test_gpu_solve_regimes._evaluate), NG_WANTED's first, in that order."""
    O = oracle
    hf, cfg = O.flat_hfield(), O.default_cfg()
    rng = np.random.default_rng(0)
    q, v, w = O.reset_state(0.01)
    sc = np.zeros(1, np.int32)
    for _ in range(60):
        O.env_step(cfg, q, v, w, sc, rng.uniform(-1, 1, 3).astype(np.float32), hf)
    best, others = {}, []
    depths = np.concatenate([np.arange(0.012, 0.002, -0.00005), np.arange(0.002, -0.024, -0.00025)])
    for dz in depths:
        x, y = rng.uniform(-3, 3, 2)
        cand = (R._placed(q, hf, x, y, dz), v + rng.normal(0, 0.05, 15), np.zeros(15),
                rng.uniform(-1, 1, 3).astype(np.float32))
        fo = O.forward(cand[0], cand[1], R._ctrl(cand[3]), cand[2], hf)
        if fo.nbody:
            continue
        if fo.nground in NG_WANTED and fo.niter > best.get(fo.nground, (-1, None))[0]:
            best[fo.nground] = (fo.niter, cand)
        others.append((fo.niter, len(others), cand))
    assert set(best) == set(NG_WANTED), sorted(best)
    chosen = [best[ng][1] for ng in NG_WANTED]
    for _, _, cand in sorted(others, key=lambda t: (-t[0], t[1])):
        if len(chosen) == 8:
            break
        if not any(cand is c for c in chosen):
            chosen.append(cand)
    recs = R._evaluate(O, "flat", chosen)
    assert len(recs) == len(chosen) and [r["ng"] for r in recs[:6]] == list(NG_WANTED)
    assert all(r["ambig"] <= R.AMBIG_TOL for r in recs), [r["ambig"] for r in recs]
    assert sum(r["niter"] >= LONG_ITERS for r in recs) >= MIN_LONG, [r["niter"] for r in recs]
    return recs


@pytest.mark.gpu
def test_ng_boundaries_fast_step(carry_states, monkeypatch):
    recs = carry_states
    g = R._step_on_gpu("flat", recs, "fp64", monkeypatch)
    eq = np.abs(g["q1"] - R._stack(recs, "q1")).max(axis=1)
    ev = np.abs(g["v1"] - R._stack(recs, "v1")).max(axis=1)
    eo = np.abs(g["obs"] - R._stack(recs, "obs")).max(axis=1)
    er = np.abs(g["r"] - R._stack(recs, "r"))
    ew = R._relerr(g["w1"], R._stack(recs, "w1"))
    print(f"ng {[r['ng'] for r in recs]} niter {[r['niter'] for r in recs]}: worst qpos {eq.max():.2e} "
          f"qvel {ev.max():.2e} obs {eo.max():.2e} reward {er.max():.2e} warm {ew.max():.2e}")
    bad = np.nonzero((eq > R.Q_TOL) | (ev > R.V_TOL) | (eo > R.OBS_TOL) | (er > R.R_TOL) | (ew > R.QACC_TOL))[0]
    assert len(bad) == 0, [(int(i), recs[i]["ng"], eq[i], ev[i], eo[i], er[i], ew[i]) for i in bad]
    assert np.array_equal(g["flags"] & 7, R._stack(recs, "flags") & 7)
    assert np.array_equal((g["flags"] & 8) != 0, R._stack(recs, "over") != 0)


@pytest.mark.gpu
def test_ng_boundaries_full_forward(carry_states):
    from ballbot_gym.envs import BallbotVecEnv

    recs = carry_states
    env = BallbotVecEnv(len(recs), device="cuda:0", precision="fp64", auto_reset=False,
                        terrain_config=R._terrain_cfg("flat"))
    env.set_state(R._stack(recs, "q"), R._stack(recs, "v"), R._stack(recs, "w"))
    qacc, ncon = env.forward(np.array([R._ctrl(r["a"]) for r in recs]))
    env.close()
    assert np.array_equal(ncon[:, 0], R._stack(recs, "ng")) and not ncon[:, 1].any()
    err = R._relerr(qacc, R._stack(recs, "qacc"))
    print(f"full kernel's forward, qacc: worst {err.max():.2e}")
    assert (err <= R.QACC_TOL).all(), [(r["ng"], e) for r, e in zip(recs, err)]


@pytest.mark.gpu
def test_mixed_wave_equals_envs_alone(carry_states, monkeypatch):
    recs = carry_states
    by_ng = {r["ng"]: r for r in recs[:6]}
    alone = {id(r): R._step_on_gpu("flat", [r], "fp64", monkeypatch) for r in recs[:6]}
    groups = [[by_ng[0], by_ng[6], by_ng[13], by_ng[14]], [by_ng[13]], [by_ng[14], by_ng[0], by_ng[30]],
              [by_ng[6], by_ng[30], by_ng[1], by_ng[13], by_ng[14]]]
    for grp in groups:
        g = R._step_on_gpu("flat", grp, "fp64", monkeypatch)
        for i, r in enumerate(grp):
            for k in ("q1", "v1", "w1", "obs", "r", "flags"):
                assert np.array_equal(g[k][i], alone[id(r)][k][0]), (len(grp), i, r["ng"], k)


@pytest.mark.gpu
def test_step_multi_equals_three_steps(carry_states, monkeypatch):
    from ballbot_gym.envs import BallbotVecEnv

    recs = carry_states
    n = len(recs)
    monkeypatch.setenv("BB_ROUTE", "1")
    envs = [BallbotVecEnv(n, device="cuda:0", precision="fp64", seed=3, terrain_config=R._terrain_cfg("flat"))
            for _ in range(2)]
    for e in envs:
        e.set_state(R._stack(recs, "q"), R._stack(recs, "v"), R._stack(recs, "w"), np.zeros(n, np.int32))
    g = torch.Generator(device="cuda:0").manual_seed(2)
    actions = torch.rand(3, n, 3, generator=g, device="cuda:0") * 2 - 1
    ref = {k: [] for k in ("obs", "reward", "done", "terminal_obs", "pos2d")}
    for t in range(3):
        obs, rew, _, _, info = envs[0].step(actions[t])
        for k, x in zip(ref, (obs, rew, info["done_flags"], info["terminal_observation"], info["pos2d"])):
            ref[k].append(x.clone())
    got = envs[1].step_multi(actions.contiguous())
    for k in ref:
        assert torch.equal(torch.stack(ref[k]), got[k]), k
    for x, y in zip(envs[0].get_state(), envs[1].get_state()):
        np.testing.assert_array_equal(x, y)
    for e in envs:
        e.close()
