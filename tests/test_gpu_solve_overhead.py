"""The fast kernels' Newton iteration after exec-mask branches round one-instruction bodies were cut (bb_team16.h:
the transpose of L stored to selected addresses, with a spare slot for what is not below the diagonal, and the
gradient's wheel terms as selected operands), on the shapes at which a change to that loop can go wrong.

States: tests/test_gpu_solve_regimes.py's flat-ground candidates (same seed), evaluated with the oracle alone; 65 of
them, chosen so that every cell below is populated, the rest in the builder's order.

  niter 0 | 1 | >= 12       solves that end before the first factorisation, after one, and long ones
  ng 0 | 1 | 13 | 14 | > 13 no ball-terrain contact (no ball block: the team sums are skipped), one, the last count
                            at which every Jacobian is the stored one, the first with a rebuilt one, and a lane
                            with two contacts (c = tl and tl + 16; ng >= 14 puts contact 16 on lane 0)
  early stop                the oracle's default forward ends more than 1e-8 (relative) from its own (100
                            iterations, 1e-12) forward: it left on MuJoCo's improvement test away from the
                            minimiser, the stop that IMPR_GRAD guards in the kernels (bb_physics.h).  The oracle
                            cannot say that the kernel's guard fired; it says that the state is one where it can.

  step vs oracle    one fast-kernel step of the first 1, 3, 17 and all 65 states (idle teams in the last wave,
                    ragged waves): qpos 1e-9, qvel 1e-6, warm start 1e-7 relative, no outlier, the oracle's flags
  fp32              the same 65 states: finite, the oracle's done flags (the fp32 solve's diagonal-Newton
                    fallback runs on roundoff-indefinite Hessians, conditioned ~1e10 in fp32)
  forms agree       bb_step x 20, bb_step_multi (20 steps) and the rollout kernel on 65 flat envs from these
                    states: observations, rewards, flags and final states bit for bit
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_solve_regimes as R  # noqa: E402

N_STATES = 65
ENV_COUNTS = (1, 3, 17, 65)
EARLY_STOP = 1e-8
CELLS = {"niter >= 12": 4, "niter 0": 2, "niter 1": 2, "ng 0": 2, "ng 1": 2, "ng 13": 2, "ng 14": 2, "ng > 13": 4,
         "early stop": 1}
T_FORMS = 20


def _cells(r):
    c = []
    if r["niter"] == 0:
        c.append("niter 0")
    if r["niter"] == 1:
        c.append("niter 1")
    if r["niter"] >= 12:
        c.append("niter >= 12")
    if r["ng"] in (0, 1, 13, 14):
        c.append(f"ng {r['ng']}")
    if r["ng"] > 13:
        c.append("ng > 13")
    if r["early"] > EARLY_STOP:
        c.append("early stop")
    return c


@pytest.fixture(scope="module")
def overhead_states(oracle):
    """65 read-only state records (test_gpu_solve_regimes._evaluate plus "early" and "ocells"): first one state
    per cell, in CELLS' order, then the cells' other states up to twice their minimum, then the rest."""
    O = oracle
    hf = R._hfield(O, "flat")
    recs = [r for r in R._evaluate(O, "flat", R._candidates(O, "flat", seed=100)) if r["ambig"] <= R.AMBIG_TOL]
    try:
        O.set_solver(100, 1e-12)
        tight = [np.array(O.forward(r["q"], r["v"], R._ctrl(r["a"]), r["w"], hf).qacc) for r in recs]
    finally:
        O.set_solver(100, 1e-8)
    for r, t in zip(recs, tight):
        r["early"] = float(R._relerr(t, r["qacc"]))
        r["ocells"] = _cells(r)
    order = []

    def take(i):
        if i not in order and len(order) < N_STATES:
            order.append(i)

    for rounds in (1, 2):
        for cell, need in CELLS.items():
            have = [i for i, r in enumerate(recs) if cell in r["ocells"]]
            for i in have[:need * rounds if rounds == 2 else 1]:
                take(i)
    for i in range(len(recs)):
        take(i)
    out = [recs[i] for i in order]
    for r in out:
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def test_census(overhead_states):
    """CPU, from the oracle alone: 65 states, every cell populated, and each env count's prefix holds what it is
    there for (1: a long solve; 3: also a solve without iteration and one that ends after one)."""
    recs = overhead_states
    assert len(recs) == N_STATES
    counts = {c: sum(c in r["ocells"] for r in recs) for c in CELLS}
    print(f"\ncensus {counts}; first three: {[(r['ng'], r['niter']) for r in recs[:3]]}")
    short = {c: (n, CELLS[c]) for c, n in counts.items() if n < CELLS[c]}
    assert not short, f"cells short of their minimum (have, need): {short}"
    assert [r["ocells"][0] for r in recs[:3]] == ["niter >= 12", "niter 0", "niter 1"]


def test_index_and_select_helpers_on_host():
    """CPU: tests/hostcheck/overhead_check.cpp, the transpose's slots against the packed triangle of the
    predicated stores on random rows, and the selected zero against the skipped subtraction, bit for bit."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    src, exe = root / "tests" / "hostcheck" / "overhead_check.cpp", root / "tests" / "_build" / "overhead_check"
    csrc = root / "openballbot-rl_amd" / "csrc"
    exe.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", f"-I{csrc}", "-o", str(exe), str(src)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _against_oracle(recs, g):
    eq = np.abs(g["q1"] - R._stack(recs, "q1")).max(axis=1)
    ev = np.abs(g["v1"] - R._stack(recs, "v1")).max(axis=1)
    ew = R._relerr(g["w1"], R._stack(recs, "w1"))
    print(f"{len(recs)} envs: worst qpos {eq.max():.2e} qvel {ev.max():.2e} warm {ew.max():.2e}")
    bad = np.nonzero((eq > R.Q_TOL) | (ev > R.V_TOL) | (ew > R.QACC_TOL))[0]
    assert len(bad) == 0, [(int(i), eq[i], ev[i], ew[i], recs[i]["ocells"]) for i in bad]
    assert np.array_equal(g["flags"] & 7, R._stack(recs, "flags") & 7)
    assert np.array_equal((g["flags"] & 8) != 0, R._stack(recs, "over") != 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_fast_step_vs_oracle(overhead_states, n, monkeypatch):
    recs = overhead_states[:n]
    _against_oracle(recs, R._step_on_gpu("flat", recs, "fp64", monkeypatch))


@pytest.mark.gpu
def test_fast_step_fp32_finite(overhead_states, monkeypatch):
    recs = overhead_states
    g = R._step_on_gpu("flat", recs, "fp32", monkeypatch)
    for k in ("q1", "v1", "w1", "obs", "r"):
        assert np.isfinite(g[k]).all(), k
    assert np.array_equal(g["flags"] & 3, R._stack(recs, "flags") & 3)
    assert np.array_equal((g["flags"] & 8) != 0, R._stack(recs, "over") != 0)


@pytest.mark.gpu
def test_launch_forms_bit_equal(overhead_states, monkeypatch):
    """The rollout kernel's 20 steps from the directed states, its own clipped actions replayed through bb_step
    and through one bb_step_multi launch on twin envs.  A first bb_step with zero actions on all three gives the
    rollout its observations (set_state does not form them); the states are then one step on."""
    from ballbot_gym.envs import BallbotVecEnv
    from ballbot_rl.training.logger import CSVLogger
    from ballbot_rl.training.ppo import BatchedPPO, fused_mlp_slots

    recs, n, T = overhead_states, N_STATES, T_FORMS
    monkeypatch.setenv("BB_ROUTE", "1")
    envs = [BallbotVecEnv(n, device="cuda:0", precision="fp64", seed=3, terrain_config=R._terrain_cfg("flat"))
            for _ in range(3)]
    zero = torch.zeros(n, 3, device="cuda:0")
    for e in envs:
        e.set_state(R._stack(recs, "q"), R._stack(recs, "v"), R._stack(recs, "w"), np.zeros(n, np.int32))
        e.step(zero)
    a, b, c = envs
    assert torch.equal(a.obs, b.obs) and torch.equal(a.obs, c.obs)
    m = BatchedPPO(a, n_steps=T, batch_size=n * T, n_epochs=1, seed=4, logger=CSVLogger(None, stdout=False))
    with torch.no_grad():
        for p in m.policy.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    slots = fused_mlp_slots(m, update=False)
    assert slots
    m._last_obs = a.obs
    m._last_starts.fill_(1)
    m._collect_rollout_kernel(slots)
    torch.cuda.synchronize()
    actions = m.buf.actions[:T].clamp(-1.0, 1.0).contiguous()
    obs = b.obs.clone()
    step_obs, step_rew, step_done = [], [], []
    for t in range(T):
        assert torch.equal(m.buf.obs[t], obs), t
        o, r, _, _, info = b.step(actions[t])
        assert torch.equal(m.buf.rewards[t], r), t
        step_obs.append(o.clone()), step_rew.append(r.clone()), step_done.append(info["done_flags"].clone())
        obs = o.clone()
    assert torch.equal(a.obs, obs)
    got = c.step_multi(actions)
    assert torch.equal(got["obs"], torch.stack(step_obs))
    assert torch.equal(got["reward"], torch.stack(step_rew))
    assert torch.equal(got["done"], torch.stack(step_done))
    sb = b.get_state()
    for other in (a, c):
        for x, y in zip(sb, other.get_state()):
            np.testing.assert_array_equal(x, y)
    for e in envs:
        e.close()
