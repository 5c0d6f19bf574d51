"""GPU: bb_pid_rollout (pid_rollout_kernel, csrc/bb_kernels.hip), BatchedPID.rollout and
balance(fused=True): K steps of the PID balance loop in one launch against the per-step loop.

Twin envs built alike: twin A runs K x (pid.act, env.step) eagerly and keeps everything, twin B makes
rollout() calls.  "Equal" is bit for bit (_bits / array_equal): every trace, the controller's state,
env.obs / done / reward / terminal_obs / pos2d, get_state(), env_terrain() and stats().  Both twins
are on the serial route (flat banks take it by default; the relief cases set BB_ROUTE=1), where the
multi-step forms compute the per-step loop's bits; the default route on a relief bank is only run for
completion.  Conditions such as "both kinds of ending occurred" are asserted on twin A, never on the
code under test.

Endings inside a launch: episodes are 12 steps long, too short for the toppling setpoint (pitch 0.5 rad
on the even envs) to bring a robot from upright past the tilt limit, so _tip() also starts every fourth
env 30 degrees over (failure at step 0) and every fourth 17 degrees over and turning (failure some steps
later; on the MI355X half of the failure endings fall after step 0).  balance() resets the env itself,
so its cases tip two envs with set_state from inside a wrapped env.reset().  Measured there: the 25
tests take 5 s; the perlin twin takes 2842 full steps and 70 resets in 256 steps of 64 envs."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_pid_host import GAINS  # noqa: E402
from test_pid_rollout_host import check_pid_rollout_argument_errors  # noqa: E402

DEV = "cuda:0"
GUARD = 64  # sentinel rows behind every written buffer
SENTINEL, SENTINEL_U8 = -7.25, 0xA5
TRACES = ("actions", "angle_deg", "obs", "reward", "done", "terminal_obs", "pos2d")
K, EP = 37, 12  # 37 steps with 12-step episodes: every env auto-resets three times inside the launch
DONE_BITS = 1 | 2 | 4 | 8  # BB_DONE_*


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(x, y, what):
    assert x.shape == y.shape and x.dtype == y.dtype, what
    bad = (_bits(x) != _bits(y)).nonzero()
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first {bad[:4].tolist()}"


def _env(n, precision="fp64", terrain="flat", **kw):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device=DEV, seed=3, precision=precision, terrain_config={"type": terrain, "config": {}},
                         **kw)


def _twins(n, count=2, **kw):
    from ballbot_gym.controllers import BatchedPID

    envs = [_env(n, **kw) for _ in range(count)]
    return [(e, BatchedPID(e, *GAINS)) for e in envs]


def _setpoints(n, k=None, seed=11):
    """(pitch, roll) f32[n] (or [k, n]): make_rotvec_case's scale U(+-0.05 rad); the even envs get the
    toppling pitch 0.5 rad."""
    rng = np.random.default_rng(seed + n)
    sp = rng.uniform(-0.05, 0.05, ((k or 1), n, 2)).astype(np.float32)
    sp[:, 0::2, 0] = 0.5
    sp = sp if k else sp[0]
    return torch.tensor(sp[..., 0], device=DEV), torch.tensor(sp[..., 1], device=DEV)


def _tip(env):
    """Every fourth env 30 degrees over (its next step ends in failure), every fourth (offset 2) 17
    degrees over and turning on at 3 rad/s about the same axis (it fails some steps later)."""
    n = env.num_envs
    q, v, w, s = env.get_state()
    axis = np.array([0.6, 0.8, 0.0])
    for idx, deg, spin in ((np.arange(0, n, 4), 30.0, 0.0), (np.arange(2, n, 4), 17.0, 3.0)):
        t = np.radians(deg)
        q[idx, 3:7] = [np.cos(t / 2), *(np.sin(t / 2) * axis)]
        v[idx, 3:6] = spin * axis
    env.set_state(q, v, w, s)


def _eager(env, pid, k, sp_p, sp_r):
    """k x (pid.act, env.step) -> the traces [k, ...]; sp_*: float, f32[n] or a schedule f32[k, n]."""
    rows = {name: [] for name in TRACES}
    for t in range(k):
        p, r = (v[t] if isinstance(v, torch.Tensor) and v.dim() == 2 else v for v in (sp_p, sp_r))
        a, deg = pid.act(env.obs, setpoint_r=r, setpoint_p=p)
        rows["actions"].append(a.clone()); rows["angle_deg"].append(deg.clone())
        obs, rew, _, _, info = env.step(a)
        rows["obs"].append(obs.clone()); rows["reward"].append(rew.clone()); rows["done"].append(info["done_flags"].clone())
        rows["terminal_obs"].append(info["terminal_observation"].clone()); rows["pos2d"].append(info["pos2d"].clone())
    return {name: torch.stack(v) for name, v in rows.items()}


def _same_end(a, pa, b, pb):
    """Everything the two forms leave behind."""
    for name in ("obs", "done", "reward", "terminal_obs", "pos2d"):
        _same(getattr(a, name), getattr(b, name), f"env.{name}")
    _same(pa.state, pb.state, "controller state")
    _same(pa.setpoint, pb.setpoint, "controller setpoints")
    for x, y, name in zip(a.get_state(), b.get_state(), ("qpos", "qvel", "warm", "steps")):
        assert np.array_equal(x, y), name
    for x, y in zip(a.env_terrain(), b.env_terrain()):
        assert np.array_equal(x, y)
    assert a.stats() == b.stats(), (a.stats(), b.stats())


def _guard_env(env, pid):
    """Move the buffers the launch writes (the env's outputs, the controller's state) into storage with
    GUARD sentinel rows behind row n -> the guarded tensors."""
    n, held = env.num_envs, []
    for obj, name in [(env, x) for x in ("obs", "reward", "done", "terminal_obs", "pos2d")] + [(pid, "state")]:
        old = getattr(obj, name)
        sent = SENTINEL_U8 if old.dtype == torch.uint8 else SENTINEL
        big = torch.full((n + GUARD,) + tuple(old.shape[1:]), sent, dtype=old.dtype, device=DEV)
        big[:n] = old
        setattr(obj, name, big[:n])
        held.append((big, n, sent))
    return held


def _guarded_traces(k, n, names=TRACES):
    from ballbot_gym.controllers import BatchedPID

    out, held = {}, []
    for name in names:
        _, tail, dtype = BatchedPID.TRACES[name]
        sent = SENTINEL_U8 if dtype == torch.uint8 else SENTINEL
        big = torch.full((k * n + GUARD,) + tail, sent, dtype=dtype, device=DEV)
        out[name] = big[:k * n].view((k, n) + tail)
        held.append((big, k * n, sent))
    return out, held


def _guards_intact(held):
    for big, rows, sent in held:
        assert bool((big[rows:] == sent).all()), "a sentinel row was written"


def _both_endings(done):
    term, fail = (done & 1) != 0, (done & 2) != 0
    assert bool(fail.any()) and bool((term & ~fail).any()), "twin A must show failures and step-limit endings"
    return int(fail.sum()), int((term & ~fail).sum())


# ------------------------------------------------------------------ flat
def _flat_case(n, precision, monkeypatch):
    # four envs per workgroup whatever n (read by bb_create; the default is one up to 1024 envs), so that
    # n = 1, 3, 4, 5, 63, 64, 65, 257 are team, workgroup and wave edges
    monkeypatch.setenv("BB_EPW", "4")
    (a, pa), (b, pb) = _twins(n, precision=precision, max_ep_steps=EP)
    assert a.launch_config()["envs_per_wave"] == 4 and b.launch_config()["envs_per_wave"] == 4
    try:
        sp_p, sp_r = _setpoints(n)
        for env in (a, b):
            env.reset()
            _tip(env)
        ref = _eager(a, pa, K, sp_p, sp_r)
        nf, nl = _both_endings(ref["done"])
        late = int(((ref["done"][1:] & 2) != 0).sum())
        assert a.stats()["resets"] >= 3 * n  # every env auto-reset three times (and its controller row cleared)
        held = _guard_env(b, pb)
        out, held_t = _guarded_traces(K, n)
        got = pb.rollout(K, setpoint_r=sp_r, setpoint_p=sp_p, trace=TRACES, out=out)
        assert got is out
        torch.cuda.synchronize()
        _guards_intact(held + held_t)
        for name in TRACES:
            _same(ref[name], got[name], f"trace {name}")
        _same_end(a, pa, b, pb)
        print(f"n={n} {precision}: {nf} failure endings ({late} after step 0), {nl} step-limit endings, "
              f"stats {a.stats()}")
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 257])
def test_flat_fp64_rollout_equals_the_per_step_loop(n, monkeypatch):
    _flat_case(n, "fp64", monkeypatch)


def test_flat_fp32_rollout_equals_the_per_step_loop(monkeypatch):
    _flat_case(65, "fp32", monkeypatch)


@pytest.mark.parametrize("chunks", [(1,) * K, (7,) * 5 + (2,), (K,), (10, -5, 22)])
def test_chunking_and_mixing_with_eager_steps(chunks):
    """The same 37 steps as rollouts of 1, of 7 (and a rest of 2) and of 37, and as 10 fused steps, 5
    eager steps (negative entry) and 22 fused steps."""
    n = 21
    (a, pa), (b, pb) = _twins(n, max_ep_steps=EP)
    try:
        sp_p, sp_r = _setpoints(n)
        for env in (a, b):
            env.reset()
            _tip(env)
        ref = _eager(a, pa, K, sp_p, sp_r)
        _both_endings(ref["done"])
        parts, out = [], None
        for c in chunks:
            if c < 0:
                parts.append(_eager(b, pb, -c, sp_p, sp_r))
                continue
            out = pb.rollout(c, setpoint_r=sp_r, setpoint_p=sp_p, trace=TRACES, out=out)
            parts.append({name: t.clone() for name, t in out.items()})
        assert sum(abs(c) for c in chunks) == K
        for name in TRACES:
            _same(ref[name], torch.cat([p[name] for p in parts]), f"trace {name}")
        _same_end(a, pa, b, pb)
    finally:
        a.close(); b.close()


def test_setpoint_schedule_and_null_setpoints():
    """f32[K, N] setpoints against the eager loop fed row t at step t; a float with a schedule; NULL
    setpoint pointers (the C call) against zeros."""
    N = _native()
    n = 21
    (a, pa), (b, pb) = _twins(n, max_ep_steps=EP)
    try:
        sp_p, sp_r = _setpoints(n, k=K)
        assert sp_p.shape == (K, n) and bool((sp_p[1] != sp_p[0]).any())
        for env in (a, b):
            env.reset()
        ref = _eager(a, pa, K, sp_p, sp_r)
        got = pb.rollout(K, setpoint_r=sp_r, setpoint_p=sp_p, trace=TRACES)
        for name in TRACES:
            _same(ref[name], got[name], f"trace {name}")
        _same_end(a, pa, b, pb)
        ref = _eager(a, pa, 9, sp_p[:9], 0.01)  # a schedule for one angle, a float for the other
        got = pb.rollout(9, setpoint_r=0.01, setpoint_p=sp_p[:9], trace=TRACES)
        for name in TRACES:
            _same(ref[name], got[name], f"trace {name}")
        _same_end(a, pa, b, pb)
        with pytest.raises(ValueError):
            pb.rollout(9, setpoint_p=sp_p[:8])
        with pytest.raises(ValueError):
            pb.rollout(0)
        # NULL setpoints: the raw call on twin B against eager zero setpoints on twin A
        ref = _eager(a, pa, 6, 0.0, 0.0)
        acts = torch.empty(6, n, 3, device=DEV)
        args = N.PIDRolloutArgs()
        args.cfg = N.PIDCfg(pb.dt, *GAINS, 10.0, N.PID_ROTVEC, N.PID_MOTOR)
        args.n_steps = 6
        args.state, args.obs, args.done = pb.state.data_ptr(), b.obs.data_ptr(), b.done.data_ptr()
        args.reward, args.terminal_obs, args.pos2d = b.reward.data_ptr(), b.terminal_obs.data_ptr(), b.pos2d.data_ptr()
        args.buf_actions = acts.data_ptr()
        b.run_pid_rollout(args)
        pb.setpoint.zero_()  # the raw call does not touch the controller's setpoint buffer
        _same(ref["actions"], acts, "actions with NULL setpoints")
        _same_end(a, pa, b, pb)
    finally:
        a.close(); b.close()


def test_optional_outputs_off_equal_on():
    """All traces off against all on, and the env's optional reward / terminal_obs / pos2d pointers NULL
    against given: the same final buffers and state."""
    N = _native()
    n = 21
    (a, pa), (b, pb), (c, pc) = _twins(n, count=3, max_ep_steps=EP)
    try:
        sp_p, sp_r = _setpoints(n)
        for env in (a, b, c):
            env.reset()
            _tip(env)
        assert pa.rollout(K, setpoint_r=sp_r, setpoint_p=sp_p) == {}
        pb.rollout(K, setpoint_r=sp_r, setpoint_p=sp_p, trace=TRACES)
        _same_end(a, pa, b, pb)
        assert a.stats()["resets"] >= 3 * n
        # reward / terminal_obs / pos2d NULL: obs, done, the controller and the handle's state as before
        pc._set_setpoints(sp_r, sp_p)
        args = N.PIDRolloutArgs()
        args.cfg = N.PIDCfg(pc.dt, *GAINS, 10.0, N.PID_ROTVEC, N.PID_MOTOR)
        args.n_steps = K
        args.setpoint = pc.setpoint.data_ptr()
        args.state, args.obs, args.done = pc.state.data_ptr(), c.obs.data_ptr(), c.done.data_ptr()
        before = [t.clone() for t in (c.reward, c.terminal_obs, c.pos2d)]
        c.run_pid_rollout(args)
        for x, y in zip(before, (c.reward, c.terminal_obs, c.pos2d)):
            _same(x, y, "an output whose pointer was NULL")
        for name in ("obs", "done"):
            _same(getattr(a, name), getattr(c, name), f"env.{name}")
        _same(pa.state, pc.state, "controller state")
        for x, y in zip(a.get_state(), c.get_state()):
            assert np.array_equal(x, y)
        assert a.stats() == c.stats()
    finally:
        a.close(); b.close(); c.close()


# ------------------------------------------------------------------ relief banks: hand-overs
def _perlin_twins(n, monkeypatch, route, park, count=2):
    from ballbot_gym.controllers import BatchedPID

    if route is None:
        monkeypatch.delenv("BB_ROUTE", raising=False)
    else:
        monkeypatch.setenv("BB_ROUTE", route)  # read by bb_create
    monkeypatch.setenv("BB_MULTI_PARK", park)
    envs = [_env(n, terrain="perlin", n_terrains=None, stream_seeds=[50 + i for i in range(n)], max_ep_steps=200)
            for _ in range(count)]
    return [(e, BatchedPID(e, *GAINS)) for e in envs]


@pytest.mark.parametrize("park", ["1", "0"])
def test_perlin_hand_overs_parked_and_inline(park, monkeypatch):
    """Perlin with per-env generators, 64 envs x 256 steps, both twins on the serial route: the fast
    path hands steps over (base-tree contacts), parked for the finish launch (BB_MULTI_PARK=1) or
    taken inline (0).  In chunks of 96, 96 and 64 steps, so that parked launches follow each other."""
    n, steps = 64, 256
    (a, pa), (b, pb) = _perlin_twins(n, monkeypatch, "1", park)
    try:
        sp_p, sp_r = _setpoints(n)
        for env in (a, b):
            env.reset()
        ref = _eager(a, pa, steps, sp_p, sp_r)
        st = a.stats()
        print(f"perlin twin A: {st}")
        assert st["slow_path"] > 0 and st["resets"] > 0  # checked on the per-step twin
        parts = []
        for c in (96, 96, 64):
            out = pb.rollout(c, setpoint_r=sp_r, setpoint_p=sp_p, trace=TRACES)
            parts.append(out)
        for name in TRACES:
            _same(ref[name], torch.cat([p[name] for p in parts]), f"trace {name}")
        _same_end(a, pa, b, pb)
        b.check()
    finally:
        a.close(); b.close()


def test_perlin_default_route_completes(monkeypatch):
    """A default-route perlin handle (route 0 per step): the rollout runs its serial forms, completes with a
    clean check(), and its done trace holds BB_DONE_* bits only.  No equality claim: the two routes
    agree per step only to rounding."""
    n = 64
    (b, pb), = _perlin_twins(n, monkeypatch, None, "1", count=1)
    try:
        sp_p, sp_r = _setpoints(n)
        b.reset()
        out = pb.rollout(256, setpoint_r=sp_r, setpoint_p=sp_p, trace=("done", "reward", "obs"))
        b.check()
        done = out["done"]
        assert not bool((done & ~DONE_BITS).any())
        assert bool(((done & 2) != 0).le((done & 1) != 0).all())  # a failure is a termination
        assert bool(torch.isfinite(out["reward"]).all()) and bool(torch.isfinite(out["obs"]).all())
        assert b.stats()["resets"] == int(((done & 1) != 0).sum())
        obs, _, _, _, _ = b.step(pb.act(b.obs)[0])  # the per-step loop goes on from there
        assert bool(torch.isfinite(obs).all())
    finally:
        b.close()


# ------------------------------------------------------------------ the summary
def _tipping_reset(env, idx):
    """env.reset() that then tips envs idx 30 degrees over with set_state (their first step fails)."""
    plain = env.reset

    def reset(mask=None):
        out = plain(mask)
        q, v, w, s = env.get_state()
        t = np.radians(30.0)
        q[idx, 3:7] = [np.cos(t / 2), *(np.sin(t / 2) * np.array([0.6, 0.8, 0.0]))]
        env.set_state(q, v, w, s)
        return out

    env.reset = reset


@pytest.mark.parametrize("chunk", [300, 64, 1])
def test_fused_balance_equals_balance(chunk):
    from ballbot_gym.controllers import balance

    n, steps = 8, 300
    (a, pa), (b, pb) = _twins(n, max_ep_steps=120)
    try:
        for env in (a, b):
            _tipping_reset(env, [2, 5])
        sp_p = torch.tensor(np.radians([0, 1, 0, -1, 0.5, 0, 0, 2]).astype(np.float32), device=DEV)
        want = balance(a, pa, steps, setpoint_p=sp_p, setpoint_r=0.01)
        got = balance(b, pb, steps, setpoint_p=sp_p, setpoint_r=0.01, fused=True, chunk=chunk)
        # twin A: failures, episodes shorter than the run and positions frozen at their end all occur
        assert want["failed"].tolist() == [e in (2, 5) for e in range(n)]
        assert (want["steps"] < steps).all() and want["steps"][2] == 1 and (want["steps"][[0, 1, 3]] == 120).all()
        assert not np.array_equal(want["pos2d"], a.pos2d.cpu().numpy())
        assert set(got) == set(want)
        for key in want:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
            assert got[key].tobytes() == want[key].tobytes(), (key, got[key], want[key])
        assert (want["G_tau"] != 0).all()
        _same_end(a, pa, b, pb)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------ graph, logs, errors, CLI
def test_graph_replays_equal_eager_rollouts():
    """One captured rollout(8) replayed three times against three eager rollout(8) calls on a twin."""
    n = 21
    (a, pa), (b, pb) = _twins(n, max_ep_steps=EP)
    try:
        for env in (a, b):
            env.reset()
            _tip(env)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up: the setpoints are filled here, so the capture holds the launch alone
            pb.rollout(8, setpoint_r=-0.02, setpoint_p=0.01)
        torch.cuda.current_stream().wait_stream(side)
        pa.rollout(8, setpoint_r=-0.02, setpoint_p=0.01)
        b.note_graph_capture()
        graph = torch.cuda.CUDAGraph()
        state0 = pb.state.clone()
        with torch.cuda.graph(graph):
            out = pb.rollout(8, setpoint_r=-0.02, setpoint_p=0.01, trace=("actions", "done"))
        _same(state0, pb.state, "a capture runs nothing")
        for _ in range(3):
            graph.replay()
            ref = pa.rollout(8, setpoint_r=-0.02, setpoint_p=0.01, trace=("actions", "done"))
            for name in ref:
                _same(ref[name], out[name], f"trace {name}")
            _same_end(a, pa, b, pb)
        assert a.stats()["resets"] >= 2 * n
    finally:
        a.close(); b.close()


def test_episode_logs_equal_the_per_step_loops(tmp_path):
    """An env that logs its reward terms: the files of flush_logs() after fused and after eager steps, byte
    for byte; without the terminal_obs and done traces the rollout is refused."""
    from ballbot_gym.controllers import BatchedPID

    n = 5
    reward = {"type": "directional", "config": {"target_direction": [0.6, 0.8]}}
    envs = [_env(n, max_ep_steps=EP, reward_config=reward,
                 log_options={"reward_terms": True, "dir": str(tmp_path / d)}) for d in ("a", "b")]
    (a, pa), (b, pb) = [(e, BatchedPID(e, *GAINS)) for e in envs]
    try:
        sp_p, sp_r = _setpoints(n)
        for env in (a, b):
            env.reset()
            _tip(env)
        with pytest.raises(RuntimeError, match="buf_terminal_obs and buf_flags"):
            pb.rollout(K, setpoint_r=sp_r, setpoint_p=sp_p, trace=("actions",))
        _eager(a, pa, K, sp_p, sp_r)
        pb.rollout(20, setpoint_r=sp_r, setpoint_p=sp_p, trace=("terminal_obs", "done"))
        pb.rollout(K - 20, setpoint_r=sp_r, setpoint_p=sp_p, trace=("terminal_obs", "done"))
        _same_end(a, pa, b, pb)
        a.flush_logs(); b.flush_logs()
        fa = sorted(p.relative_to(tmp_path / "a") for p in (tmp_path / "a").rglob("*") if p.is_file())
        fb = sorted(p.relative_to(tmp_path / "b") for p in (tmp_path / "b").rglob("*") if p.is_file())
        assert fa == fb and len(fa) >= n
        for rel in fa:
            assert (tmp_path / "a" / rel).read_bytes() == (tmp_path / "b" / rel).read_bytes(), rel
    finally:
        a.close(); b.close()


def _native():
    from ballbot_gym import _native as N

    return N


def test_argument_errors_and_refusals():
    """The CPU file's table on the GPU machine, the BB_REWARD_NONE handle, pitch/roll space, the env-side
    refusals, and a refused call leaves every buffer alone."""
    from ballbot_gym import ComponentRegistry
    from ballbot_gym.controllers import BatchedPID
    from ballbot_gym.rewards import BaseReward

    N = _native()
    check_pid_rollout_argument_errors(N)

    class Upright(BaseReward):
        def __call__(self, state):
            return -float(np.linalg.norm(state["orientation"]))

    if "upright_pid_rollout_test" not in ComponentRegistry.list_rewards():
        ComponentRegistry.register_reward("upright_pid_rollout_test", Upright)
    env = _env(3, reward_config={"type": "upright_pid_rollout_test", "config": {}})
    try:
        pid = BatchedPID(env, *GAINS)
        env.reset()
        with pytest.raises(RuntimeError, match="built-in reward"):
            pid.rollout(4)
        args = N.PIDRolloutArgs()
        args.cfg = N.PIDCfg(pid.dt, *GAINS, 10.0, N.PID_ROTVEC, N.PID_MOTOR)
        args.n_steps = 4
        args.state, args.obs, args.done = pid.state.data_ptr(), env.obs.data_ptr(), env.done.data_ptr()
        before = (pid.state.clone(), env.obs.clone(), env.done.clone())
        assert N.lib().bb_pid_rollout(env._h, C.byref(args), 1, None) < 0
        assert "BB_REWARD_NONE" in N.last_error()
        torch.cuda.synchronize()
        for x, y in zip(before, (pid.state, env.obs, env.done)):
            _same(x, y, "a refused call wrote")
    finally:
        env.close()
    env = _env(3)
    try:
        with pytest.raises(ValueError, match="motor"):
            BatchedPID(env, *GAINS, space="pitch_roll").rollout(4)
        with pytest.raises(ValueError, match="unknown trace"):
            BatchedPID(env, *GAINS).rollout(4, trace=("wheels",))
    finally:
        env.close()


def test_install_check_fused_prints_what_the_unfused_run_prints(capsys):
    from ballbot_gym.controllers import main

    assert main(["--num-envs", "4", "--steps", "300"]) == 0
    plain = capsys.readouterr().out
    assert main(["--num-envs", "4", "--steps", "300", "--fused"]) == 0
    fused = capsys.readouterr().out
    assert plain.count("successfuly balanced robot for 299 steps") == 4 and plain.count("G_tau==") == 4
    assert fused == plain
    with pytest.raises(SystemExit):
        main(["--steps", "10", "--fused", "--video", "x.png"])
