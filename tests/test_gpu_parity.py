"""GPU parity: the HIP step (through the C-ABI) vs the fp64 CPU oracle.

Teacher-forced: every env starts each step from the oracle's state, so the
comparison measures one mj_step + glue, not chaotic drift.

fp64 kernel (the default): qpos 1e-9, qvel 1e-6, obs 1e-6, reward 1e-7 and the warm start
the step leaves (the last RK stage's solved qacc: the fast kernels' solve before h scales it)
1e-7 relative to max(1, max|warm|), the forward tests' bound, for every
env-step but at most ONE per test, and every env-step within qvel 2e-5.  The oracle
restates MuJoCo's solver (PrimalSearch line search, improvement-or-gradient stop at 1e-8);
the kernel keeps its own line search.  Where the two searches end an iteration at
different points, the improvement test can stop one Newton iteration apart:
tools/solver_parity.py (host build of the kernel templates) finds that in 1 of 81,920
teacher-forced env-steps, at qvel 1.0e-5 / qpos 5e-9 (profiles/r05_solver_parity.json).
Each test prints its worst errors and outlier count (DESIGN §4 keeps the measured ones).

fp32 kernel: qpos 1e-5, qvel 1e-3, obs 1e-4, reward 1e-6 for
at least 99.9% of env-steps; the rest must stay below qvel 1e-2; the warm start finite.  Residual
fp32 outliers are states where a wheel contact's drive-direction row (R scaled
by (0.001/1.0)^2, ballbot.xml:90-92) makes the Newton Hessian ~1e10
ill-conditioned for float arithmetic; DESIGN.md §fp32 documents them.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = {"fp32": dict(q=1e-5, v=1e-3, obs=1e-4, r=1e-6, frac=0.999, vmax=1e-2),
       "fp64": dict(q=1e-9, v=1e-6, obs=1e-6, r=1e-7, max_bad=1, vmax=2e-5)}
WARM_TOL = 1e-7  # fp64: the forward tests' qacc bound, relative to max(1, max|warm|)


@pytest.fixture(scope="module")
def flat_traj(oracle):
    import traj

    return traj.record(n_envs=64, n_steps=120, hfield=oracle.flat_hfield(), seed=3)


@pytest.fixture(scope="module")
def hills_traj(oracle):
    import traj
    from ballbot_gym.terrain import generate_hills_terrain

    hf = generate_hills_terrain(293, seed=7).astype(np.float32)
    return hf, traj.record(n_envs=32, n_steps=80, hfield=hf, seed=5)


def _make_env(n, precision, terrain=None):
    from ballbot_gym.envs import BallbotVecEnv

    env = BallbotVecEnv(n, device="cuda:0", precision=precision, auto_reset=False,
                        terrain_config=terrain or {"type": "flat", "config": {}})
    return env


def _teacher_forced(env, rec, tol):
    """Step every env from the oracle's pre-step state; compare post-step state/outputs."""
    bad = 0
    total = 0
    worst = dict(q=0.0, v=0.0, obs=0.0, r=0.0, w=0.0)
    fp64 = "max_bad" in tol
    for t in range(rec["qpos"].shape[0]):
        env.set_state(rec["qpos"][t], rec["qvel"][t], rec["warm"][t], rec["steps"][t])
        a = torch.tensor(rec["action"][t], dtype=torch.float32, device=env.device)
        obs, rew, term, trunc, info = env.step(a)
        q, v, w, s = env.get_state()
        eq = np.abs(q - rec["qpos1"][t]).max(axis=1)
        ev = np.abs(v - rec["qvel1"][t]).max(axis=1)
        eo = np.abs(obs.cpu().numpy() - rec["obs"][t]).max(axis=1)
        er = np.abs(rew.cpu().numpy() - rec["reward"][t])
        ok = state_ok = (eq <= tol["q"]) & (ev <= tol["v"]) & (eo <= tol["obs"]) & (er <= tol["r"])
        # the warm start is the last RK stage's solved qacc: the solve itself, not yet multiplied by h
        assert np.isfinite(w).all(), f"step {t}: warm start not finite"
        ew = np.abs(w - rec["warm1"][t]).max(axis=1) / np.maximum(1.0, np.abs(rec["warm1"][t]).max(axis=1))
        if fp64:
            ok = state_ok & (ew <= WARM_TOL)
        bad += int((~ok).sum())
        total += len(ok)
        for k, arr in (("q", eq), ("v", ev), ("obs", eo), ("r", er), ("w", ew)):
            worst[k] = max(worst[k], float(arr.max()))
        assert ev.max() <= tol["vmax"], f"step {t}: qvel error {ev.max():.3e} beyond outlier bound"
        gflags = info["done_flags"].cpu().numpy() & 3
        mism = np.nonzero((gflags != (rec["flags"][t] & 3)) & state_ok)[0]
        assert len(mism) == 0, f"step {t}: termination flags differ for envs {mism}"
    print(f"\nteacher-forced: {total} env-steps, {bad} outside tolerance, worst {worst}")
    if "max_bad" in tol:
        assert bad <= tol["max_bad"], f"{bad} of {total} env-steps outside tolerance ({worst})"
    else:
        frac = 1.0 - bad / total
        assert frac >= tol["frac"], f"only {frac:.4%} of env-steps within tolerance ({worst})"
    return worst


def test_native_library_loads():
    from ballbot_gym import _native

    L = _native.lib()
    assert L.bb_abi_version() == _native.ABI_VERSION


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_forward_parity(oracle, flat_traj, precision):
    rec = flat_traj
    env = _make_env(rec["qpos"].shape[1], precision)
    hf = oracle.flat_hfield()
    rng = np.random.default_rng(0)
    for t in (0, 30, 60, 100):
        ctrl = rng.uniform(-10, 10, (env.num_envs, 3))
        env.set_state(rec["qpos"][t], rec["qvel"][t], rec["warm"][t])
        qacc, ncon = env.forward(ctrl)
        for e in range(env.num_envs):
            fo = oracle.forward(rec["qpos"][t][e], rec["qvel"][t][e], ctrl[e], rec["warm"][t][e], hf)
            ref = np.array(fo.qacc)
            assert ncon[e, 0] == fo.nground and ncon[e, 1] == fo.nbody
            err = np.abs(qacc[e] - ref).max() / max(1.0, np.abs(ref).max())
            assert err < (2e-4 if precision == "fp32" else 1e-7), (t, e, err)
    env.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_step_parity_flat(flat_traj, precision):
    env = _make_env(flat_traj["qpos"].shape[1], precision)
    _teacher_forced(env, flat_traj, TOL[precision])
    env.close()


@pytest.mark.parametrize("precision", ["fp32", "fp64"])
def test_step_parity_hills(hills_traj, precision):
    hf, rec = hills_traj
    env = _make_env(rec["qpos"].shape[1], precision, terrain={"type": "hills", "config": {"seed": 7}})
    _teacher_forced(env, rec, TOL[precision])
    env.close()


def _body_contact_states(oracle, n, seed):
    """States where base-tree geoms touch the terrain or the ball: rolled and
    lowered bases (tower/stick/wheel vs hfield), displaced balls (ball vs
    tower/sticks), random velocities."""
    rng = np.random.default_rng(seed)
    qs, vs = [], []
    for i in range(n):
        q, v, _ = oracle.reset_state(0.01)
        ang = rng.uniform(30, 100)
        ax = rng.normal(size=3)
        ax[2] = 0
        ax /= np.linalg.norm(ax)
        t = np.radians(ang)
        q[3:7] = [np.cos(t / 2), *(np.sin(t / 2) * ax)]
        q[2] = rng.uniform(0.06, 0.16)
        if i % 3 == 0:
            q[10:13] = q[0:3] + rng.normal(0, 0.12, 3)  # ball near the base geoms
        else:
            q[10:13] = [rng.uniform(-1, 1), rng.uniform(-1, 1), 0.5]
        q[13:17] = [1, 0, 0, 0]
        q[7:10] = rng.uniform(-3, 3, 3)
        v[:] = rng.normal(0, 0.3, 15)
        qs.append(q)
        vs.append(v)
    return np.array(qs), np.array(vs)


@pytest.mark.parametrize("precision", ["fp64"])
@pytest.mark.parametrize("terrain", ["flat", "hills"])
def test_forward_parity_base_tree_contacts(oracle, precision, terrain):
    """Dynamic pairs hfield x {tower, sticks, wheels} and ball x {tower, sticks}:
    the HIP forward (qacc, contact counts) vs the oracle."""
    from ballbot_gym.terrain import generate_hills_terrain

    n = 64
    if terrain == "flat":
        hf = oracle.flat_hfield()
        tcfg = {"type": "flat", "config": {}}
    else:
        hf = generate_hills_terrain(293, seed=7).astype(np.float32)
        tcfg = {"type": "hills", "config": {"seed": 7}}
    env = _make_env(n, precision, tcfg)
    qs, vs = _body_contact_states(oracle, n, seed=11)
    rng = np.random.default_rng(1)
    ctrl = rng.uniform(-10, 10, (n, 3))
    env.set_state(qs, vs, np.zeros((n, 15)))
    qacc, ncon = env.forward(ctrl)
    touched = 0
    for e in range(n):
        fo = oracle.forward(qs[e], vs[e], ctrl[e], np.zeros(15), hf)
        assert (ncon[e, 0], ncon[e, 1]) == (fo.nground, fo.nbody), e
        touched += fo.nbody > 0
        ref = np.array(fo.qacc)
        err = np.abs(qacc[e] - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 1e-7, (e, err, fo.nbody)
    assert touched >= n // 4
    env.close()


def _toppled_states(oracle, n, terrain, rng):
    """Robots lying on the terrain ("flat" or "hills"), the ball beside them in the air."""
    qs, vs = [], []
    for i in range(n):
        q, v, _ = oracle.reset_state(0.01)
        t, yaw = np.radians(rng.uniform(80, 100)), rng.uniform(0, 2 * np.pi)
        ax = np.array([np.cos(yaw), np.sin(yaw), 0.0])
        q[3:7] = [np.cos(t / 2), *(np.sin(t / 2) * ax)]
        q[0:2] = rng.uniform(-0.5, 0.5, 2)
        q[2] = rng.uniform(0.09, 0.12) + (0.0 if terrain == "flat" else 0.02)
        q[10:13] = [q[0] + 0.6 * np.cos(yaw), q[1] + 0.6 * np.sin(yaw), 0.5]
        q[13:17] = [1, 0, 0, 0]
        v[:] = rng.normal(0, 0.1, 15)
        qs.append(q)
        vs.append(v)
    return np.array(qs), np.array(vs)


@pytest.mark.parametrize("terrain", ["flat", "hills"])
def test_forward_parity_contacts_past_lds(oracle, terrain):
    """Toppled robots lying on the terrain: more base-tree contacts than the
    team's 32 LDS slots (the rest spill to the env's HBM block), and towers
    across more prisms than MuJoCo's mjMAXCONPAIR (that pair keeps its first
    50 in prism order).  Contact counts, overflow-free qacc vs the oracle."""
    from ballbot_gym.terrain import generate_hills_terrain

    n = 32
    if terrain == "flat":
        hf = oracle.flat_hfield()
        tcfg = {"type": "flat", "config": {}}
    else:
        hf = generate_hills_terrain(293, seed=7).astype(np.float32)
        tcfg = {"type": "hills", "config": {"seed": 7}}
    rng = np.random.default_rng(21)
    qs, vs = _toppled_states(oracle, n, terrain, rng)
    env = _make_env(n, "fp64", tcfg)
    ctrl = rng.uniform(-10, 10, (n, 3))
    env.set_state(qs, vs, np.zeros((n, 15)))
    qacc, ncon = env.forward(ctrl)
    past = 0
    for e in range(n):
        fo = oracle.forward(qs[e], vs[e], ctrl[e], np.zeros(15), hf)
        assert (ncon[e, 0], ncon[e, 1]) == (fo.nground, fo.nbody), e
        past += fo.nbody > 32
        ref = np.array(fo.qacc)
        err = np.abs(qacc[e] - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 1e-7, (e, err, fo.nbody)
    assert past >= n // 8, past
    env.close()


@pytest.mark.parametrize("terrain", ["flat", "hills"])
def test_ball_hfield_contact_cap(oracle, terrain):
    """The ball pressed into the terrain (its centre within ~3 cm of the surface)
    intersects more prisms than MuJoCo keeps for one geom pair (mjMAXCONPAIR = 50,
    bb_team16.h collide_team MAXG, oracle/bb_oracle.c BBO_MAXGROUND): both keep the
    first 50 in prism order.  Contact counts and qacc of the forward, then one
    teacher-forced step (state, obs, reward) vs the oracle, and the step's
    overflow counter."""
    from ballbot_gym.terrain import generate_hills_terrain

    n = 48
    if terrain == "flat":
        hf, tcfg, top = oracle.flat_hfield(), {"type": "flat", "config": {}}, 0.0
    else:
        hf = generate_hills_terrain(293, seed=7).astype(np.float32)
        tcfg = {"type": "hills", "config": {"seed": 7}}
    rng = np.random.default_rng(8)
    qs, vs = [], []
    H = hf.reshape(293, 293)
    for i in range(n):
        q, v, _ = oracle.reset_state(0.01)
        x, y = rng.uniform(-0.3, 0.3, 2)
        if terrain != "flat":  # the terrain's height under the ball centre (nearest vertex)
            r, c = int(round((y + 5) / 10 * 292)), int(round((x + 5) / 10 * 292))
            top = float(H[r, c]) * 2.0
        q[10:13] = [x, y, top + 0.14 + rng.uniform(-0.03, 0.08)]  # ball body: geom centre 0.14 below
        q[0:3] = [x, y, top + 1.0]  # the base well above (no base-tree contact)
        v[:] = rng.normal(0, 0.05, 15)
        qs.append(q)
        vs.append(v)
    qs, vs = np.array(qs), np.array(vs)
    env = _make_env(n, "fp64", tcfg)
    ctrl = rng.uniform(-10, 10, (n, 3))
    env.set_state(qs, vs, np.zeros((n, 15)))
    qacc, ncon = env.forward(ctrl)
    capped = 0
    for e in range(n):
        fo = oracle.forward(qs[e], vs[e], ctrl[e], np.zeros(15), hf)
        assert (ncon[e, 0], ncon[e, 1]) == (fo.nground, fo.nbody), e
        capped += fo.ground_overflow != 0
        ref = np.array(fo.qacc)
        err = np.abs(qacc[e] - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 1e-7, (e, err, fo.nground)
    assert capped >= n // 4 and (ncon[:, 0] == 50).sum() == capped, (capped, np.bincount(ncon[:, 0]))
    acts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    s0 = env.stats()
    env.set_state(qs, vs, np.zeros((n, 15)))
    obs, rew, _, _, info = env.step(torch.tensor(acts, device="cuda:0"))
    q1, v1, _, _ = env.get_state()
    assert env.stats()["overflow"] - s0["overflow"] >= capped
    cfg = oracle.default_cfg()
    for e in range(n):
        qe, ve, we, se = qs[e].copy(), vs[e].copy(), np.zeros(15), np.zeros(1, np.int32)
        o, r, f, _, _ = oracle.env_step(cfg, qe, ve, we, se, acts[e], hf)
        assert np.abs(q1[e] - qe).max() < 1e-9, e
        assert np.abs(v1[e] - ve).max() < 1e-6 * max(1.0, np.abs(ve).max()), e
        assert np.abs(obs.cpu().numpy()[e] - o).max() < 1e-6 and abs(float(rew[e]) - r) < 1e-7, e
    env.close()


@pytest.mark.parametrize("terrain", ["flat", "hills"])
def test_step_routes_agree(oracle, terrain, monkeypatch):
    """The two step routes (predict + concurrent full kernel, BB_ROUTE=0; serial
    fast-then-full, BB_ROUTE=1; the default picks serial on flat banks) and the
    full kernel's envs per wave (BB_EPW_FULL) only move work between kernels:
    the same states and outputs over several steps from base-tree-contact states.  An env
    the predictor sends to the full kernel without a base-tree contact runs the full
    kernel's instantiation of the same physics, so agreement is to rounding, not bitwise.
    128 envs = 32 workgroups, so the list launches' XCD-aware permutation over the
    active workgroups is exercised."""
    from ballbot_gym.terrain import generate_hills_terrain  # noqa: F401  (hills bank via the env config)

    n = 128
    tcfg = {"type": "flat", "config": {}} if terrain == "flat" else {"type": "hills", "config": {"seed": 7}}
    qs, vs = _body_contact_states(oracle, n, seed=13)
    acts = torch.tensor(np.random.default_rng(3).uniform(-1, 1, (5, n, 3)), dtype=torch.float32, device="cuda:0")
    res = []
    for route, epf in (("0", "4"), ("1", "4"), ("0", "1")):
        monkeypatch.setenv("BB_ROUTE", route)
        monkeypatch.setenv("BB_EPW_FULL", epf)
        env = _make_env(n, "fp64", tcfg)
        env.set_state(qs, vs, np.zeros((n, 15)), np.zeros(n, np.int32))
        outs = []
        for k in range(5):
            obs, rew, term, trunc, info = env.step(acts[k])
            outs += [obs.clone(), rew.clone(), info["done_flags"].clone()]
        q, v, w, st = env.get_state()
        res.append((outs, q, v, w, env.stats()["slow_path"]))
        env.close()
    for outs, q, v, w, slow in res:
        assert slow > 0  # some env-steps took the full kernel on every route
        assert np.allclose(q, res[0][1], rtol=0, atol=1e-11)
        assert np.allclose(v, res[0][2], rtol=1e-9, atol=1e-9)
        for i, (a, b) in enumerate(zip(outs, res[0][0])):
            if i % 3 == 2:
                assert torch.equal(a, b)  # done flags
            else:
                assert torch.allclose(a, b, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("terrain", ["flat", "hills"])
def test_step_parity_base_tree_contacts(oracle, terrain):
    """env.step from states with base-tree contacts: they are routed to the full
    kernel (stats.slow_path counts full-kernel env-steps), results vs the oracle."""
    from ballbot_gym.terrain import generate_hills_terrain

    n = 64
    if terrain == "flat":
        hf = oracle.flat_hfield()
        tcfg = {"type": "flat", "config": {}}
    else:
        hf = generate_hills_terrain(293, seed=7).astype(np.float32)
        tcfg = {"type": "hills", "config": {"seed": 7}}
    env = _make_env(n, "fp64", tcfg)
    qs, vs = _body_contact_states(oracle, n, seed=12)
    rng = np.random.default_rng(2)
    acts = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    env.set_state(qs, vs, np.zeros((n, 15)), np.zeros(n, np.int32))
    s0 = env.stats()["slow_path"]
    obs, rew, term, trunc, info = env.step(torch.tensor(acts, device=env.device))
    assert env.stats()["slow_path"] - s0 >= n // 4
    q, v, w, st = env.get_state()
    cfg = oracle.default_cfg()
    for e in range(n):
        qe, ve, we, se = qs[e].copy(), vs[e].copy(), np.zeros(15), np.zeros(1, np.int32)
        o, r, fl, _, _ = oracle.env_step(cfg, qe, ve, we, se, acts[e], hf)
        assert np.abs(q[e] - qe).max() < 1e-9, e
        assert np.abs(v[e] - ve).max() < 1e-6 * max(1.0, np.abs(ve).max()), e
        assert np.abs(obs.cpu().numpy()[e] - o).max() < 1e-6, e
    env.close()


@pytest.mark.parametrize("cameras", [False, True])
def test_step_as_hip_graph(cameras):
    """One rollout step (route + fast/full step kernels on two streams + depth cameras)
    captured as a single HIP graph and replayed == eager stepping, bit for bit."""
    from ballbot_gym.envs import BallbotVecEnv

    n = 512
    envs = [BallbotVecEnv(n, device="cuda:0", seed=4, disable_cameras=not cameras,
                          terrain_config={"type": "perlin", "config": {}}, n_terrains=8) for _ in range(2)]
    g = torch.Generator(device="cuda:0").manual_seed(0)
    acts = torch.rand(20, n, 3, generator=g, device="cuda:0") * 2 - 1
    static_a = torch.zeros(n, 3, device="cuda:0")
    e_eager, e_graph = envs
    graph = e_graph.capture_step(static_a)
    for t in range(20):
        e_eager.step(acts[t])
        static_a.copy_(acts[t])
        graph.replay()
    torch.cuda.synchronize()
    qa, va, wa, sa = e_eager.get_state()
    qb, vb, wb, sb = e_graph.get_state()
    assert np.array_equal(qa, qb) and np.array_equal(va, vb) and np.array_equal(sa, sb)
    assert torch.equal(e_eager.obs, e_graph.obs) and torch.equal(e_eager.reward, e_graph.reward)
    if cameras:
        assert torch.equal(e_eager.depth, e_graph.depth)
    for e in envs:
        e.close()


def test_c_abi_range_errors_on_gpu():
    """Out-of-range ids and sizes come back as errors with messages, the handle stays usable."""
    import ctypes as C

    from ballbot_gym import _native as N
    from ballbot_gym.envs import BallbotVecEnv

    env = BallbotVecEnv(64, device="cuda:0", n_terrains=2, terrain_config={"type": "hills", "config": {}},
                        shared_stream=True)
    L, h = N.lib(), env._h
    hf = np.zeros(293 * 293, np.float32)
    fp = hf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.bb_set_hfield(h, 5, fp, C.c_float(2.0)) < 0 and "out of range" in N.last_error()
    assert L.bb_set_hfield(h, 0, fp, C.c_float(0.0)) < 0 and "size_z" in N.last_error()
    assert L.bb_get_hfield(h, -1, fp) < 0 and "out of range" in N.last_error()
    seeds = np.array([1, 2, 3], np.int32)
    pc = N.PerlinCfg(25.0, 4, 0.2, 2.0, 1.0)
    assert L.bb_generate_perlin(h, 0, 3, seeds.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(pc),
                                C.c_float(2.0)) < 0
    assert "out of range" in N.last_error()
    d = torch.zeros(64, 2, 8, 8, device="cuda:0")
    assert L.bb_render_depth(h, C.c_void_p(d.data_ptr()), None, 0, 8, 6, 1, None) < 0
    assert "image size" in N.last_error()
    assert L.bb_render_depth(h, C.c_void_p(d.data_ptr()), None, 8, 8, 0, 1, None) < 0
    assert "frame interval" in N.last_error()
    assert L.bb_time_kernel(h, -1) < 0
    env.step(torch.zeros(64, 3, device="cuda:0"))  # still fine
    assert env.stats()["diverged"] == 0
    env.close()


def test_full_size_step_properties():
    """BASELINE configs[1] size (4096 envs), 150 steps of random actions: properties that
    hold for every env-step whatever the trajectory (size-independent checks):
    - the reward is the reference's float32 chain of the returned obs and action
      (DirectionalReward + action penalty + survival bonus, ballbot_env.py:929-937, 1019);
    - failure <=> tilt(obs orientation) > 20 deg (:982-1017), done => reset obs;
    - obs echoes the action, clips hold (|vel|, |angular_vel| <= 2, |motor| <= 2);
    - free-joint quaternions stay unit, nothing diverges."""
    from ballbot_gym.envs import BallbotVecEnv
    from scipy.spatial.transform import Rotation as Rot

    n = 4096
    env = BallbotVecEnv(n, device="cuda:0", seed=11)
    g = torch.Generator(device="cuda:0").manual_seed(5)
    f32 = np.float32
    for t in range(150):
        a = (torch.rand(n, 3, generator=g, device="cuda:0") * 2.4 - 1.2)
        obs, rew, term, trunc, info = env.step(a)
        a_h = a.cpu().numpy()
        o = info["terminal_observation"].cpu().numpy()
        r = rew.cpu().numpy()
        fl = info["done_flags"].cpu().numpy()
        assert np.array_equal(o[:, 0:3], a_h)
        assert np.abs(o[:, 3:9]).max() <= 2 and np.abs(o[:, 12:15]).max() <= 2
        failed = (fl & 2) != 0
        vel = o[:, 12:15]
        base = (vel[:, 0] * f32(0.0) + vel[:, 1] * f32(1.0)) * f32(0.01)
        nrm = np.sqrt((a_h * a_h).sum(1, dtype=f32), dtype=f32)
        exp = base + f32(-0.0001) * (nrm * nrm)
        exp = np.where(failed, exp, exp + f32(0.02)).astype(f32)
        assert np.allclose(r, exp, rtol=0, atol=2e-8), np.abs(r - exp).max()
        tilt = np.degrees(np.arccos(np.clip(Rot.from_rotvec(o[:, 9:12].astype(np.float64)).as_matrix()[:, 2, 2],
                                            -1, 1)))
        edge = np.abs(tilt - 20.0) < 1e-4
        assert np.array_equal(failed[~edge], tilt[~edge] > 20.0)
        done = (fl & 1) != 0
        assert np.all(obs.cpu().numpy()[done] == 0)  # auto-reset observation
    q, v, _, _ = env.get_state()
    assert np.allclose(np.linalg.norm(q[:, 3:7], axis=1), 1, atol=1e-9)
    assert np.allclose(np.linalg.norm(q[:, 13:17], axis=1), 1, atol=1e-9)
    assert env.stats()["diverged"] == 0
    env.close()
