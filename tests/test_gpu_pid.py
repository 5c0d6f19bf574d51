"""GPU: the batched PID balance controller (csrc/bb_pid.hip, bb_pid_act) and ballbot_gym.controllers.

What is held to what (the tolerance is test_pid_host.py's, derived there: B(m) = sqrt(2) (k_p + k_i dt T
+ 2 k_d / dt) m spacing(float32(max |angle|)); state rows: integral T dt m ulp, prev_err m ulp;
angle_deg rtol 1e-6 against the float64 acos of the same float R22):
- the kernel against tests/pid_batch_ref.py (float64 angles, m = 1) and against the CPU torch path
  (float32 atan2, m = 2) at wave and block edges, through observation rows (obs + 9, stride 15) and
  through matrices, in both output spaces, with the optional pointers NULL and given, and with
  sentinel rows behind every buffer it writes;
- the reference's golden trajectory (m = 2), and 64 envs x 1 call against 64 one-env calls;
- the clamp with k_p = 1e4 and a NaN row that stays in its row;
- the argument errors and n == 0;
- a captured act() replayed three times against three eager calls, bit for bit;
- the closed loop on 17 flat envs (zero setpoints and sixteen headings on the 1 degree circle,
  which the fp64 CPU oracle holds for 1500 steps with at most 1.50 degrees of tilt), the binding to
  an auto-reset env's done flags, evaluate_policy, balance and the install check's main().
"""
import ctypes as C
import functools
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import pid_batch_ref as PR  # noqa: E402
from pid_ref import rotvec_to_R  # noqa: E402
from test_pid_host import (DT, GAINS, check_against_reference, check_pid_argument_errors, make_rotvec_case,  # noqa: E402
                           reference_run)

DEV = "cuda:0"
GOLD = Path(__file__).resolve().parent / "golden"
GUARD = 64  # sentinel rows behind every written buffer
SENTINEL = -7.25
T = 6


def _N():
    from ballbot_gym import _native

    return _native


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _pid_act(cfg, orient, offset, stride, sp, reset, mask, state, n, out, angle):
    N = _N()
    ptr = C.c_void_p(orient.data_ptr() + 4 * offset)
    N.check(N.lib().bb_pid_act(C.byref(cfg), ptr, stride, _p(sp), _p(reset), mask, _p(state), n, _p(out), _p(angle),
                               None), "bb_pid_act")


def _cfg(kind=0, space=0, gains=GAINS, dt=DT, limit=10.0):
    return _N().PIDCfg(dt, *gains, limit, kind, space)


def _guarded(n, w):
    return torch.full((n + GUARD, w), SENTINEL, dtype=torch.float32, device=DEV)


def _run_kernel(n, kind, space, orient, offset, stride, sp, reset, with_angle=True):
    """T steps of bb_pid_act over device orientations orient[t] -> (out, angle_deg, state) as numpy [T, ...];
    every written buffer has GUARD sentinel rows behind row n, checked after every call."""
    w = 2 if space == 1 else 3
    state = _guarded(n, 4)
    state[:n] = 0
    outs, degs, states = [], [], []
    for t in range(T):
        out, deg = _guarded(n, w), _guarded(n, 1)
        _pid_act(_cfg(kind, space), orient[t], offset, stride, None if sp is None else sp[t],
                 None if reset is None else reset[t], 0xFF, state, n, out, deg if with_angle else None)
        for buf in (out, state) + ((deg,) if with_angle else ()):
            assert (buf[n:] == SENTINEL).all(), "a sentinel row was written"
        outs.append(out[:n].cpu().numpy()); degs.append(deg[:n, 0].cpu().numpy()); states.append(state[:n].cpu().numpy())
    return np.array(outs), (np.array(degs) if with_angle else None), np.array(states)


@functools.lru_cache(maxsize=None)
def _case(n):
    """The case of n rows, its matrices, pid_batch_ref's run and the CPU torch path's run (made once)."""
    from ballbot_gym.controllers import BatchedPID

    obs, sp, reset = make_rotvec_case(n)
    R = np.stack([[rotvec_to_R(rv) for rv in obs[t, :, 9:12]] for t in range(T)]).astype(np.float32)
    ref = reference_run(obs, sp, reset)
    cpu = {}
    for space, name in ((0, "motor"), (1, "pitch_roll")):
        ctl = BatchedPID(n, *GAINS, dt=DT, space=name)
        rows = []
        for t in range(T):
            a, _ = ctl.act(torch.tensor(obs[t]), setpoint_r=torch.tensor(sp[t, :, 1]), setpoint_p=torch.tensor(sp[t, :, 0]),
                           reset=torch.tensor(reset[t]))
            rows.append((a.numpy().copy(), ctl.state.numpy().copy()))
        cpu[space] = rows
    return obs, sp, reset, R, ref, cpu


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_kernel_against_both_references(n):
    obs, sp, reset, R, ref, cpu = _case(n)
    obs_d, sp_d, reset_d = (torch.tensor(a, device=DEV) for a in (obs, sp, reset))
    R_d = torch.tensor(R.reshape(T, n, 9), device=DEV)
    ulp = ref[5]
    for space in (0, 1):
        runs = {"obs": _run_kernel(n, 0, space, obs_d, 9, 15, sp_d, reset_d),
                "mat": _run_kernel(n, 1, space, R_d, 0, 9, sp_d, reset_d)}
        for name, (out, deg, state) in runs.items():
            check_against_reference(out, deg, state, ref, space, m=1)  # pid_batch_ref, float64 angles
            for t in range(T):  # the CPU torch path, float32 atan2
                a_cpu, s_cpu = cpu[space][t]
                assert (np.abs(out[t] - a_cpu) <= 2 * ref[4][t]).all(), (name, space, t)
                assert (np.abs(state[t][:, :2] - s_cpu[:, :2]) <= (t + 1) * DT * 2 * ulp).all(), (name, space, t)
                assert (np.abs(state[t][:, 2:] - s_cpu[:, 2:]) <= 2 * ulp).all(), (name, space, t)
        assert (runs["obs"][1][:, 0] == 0).all()  # the all-zero rotation vector: no tilt, e = the setpoint
        assert runs["obs"][2][:, 0, 2:].tobytes() == sp[:, 0].tobytes()
    # the optional pointers NULL against given (zero setpoints, no reset flag set): the same actions
    zeros_sp = torch.zeros(T, n, 2, device=DEV)
    zeros_rs = torch.zeros(T, n, dtype=torch.uint8, device=DEV)
    given = _run_kernel(n, 0, 0, obs_d, 9, 15, zeros_sp, zeros_rs)
    null = _run_kernel(n, 0, 0, obs_d, 9, 15, None, None, with_angle=False)
    assert given[0].tobytes() == null[0].tobytes() and given[2].tobytes() == null[2].tobytes()
    check_against_reference(null[0], None, null[2], reference_run(obs, None, None), 0, m=1)


def test_golden_trajectory_and_fresh_first_steps():
    g = np.load(GOLD / "pid.npz")
    gains, dt = tuple(float(x) for x in g["gains"]), float(g["dt"])
    R = torch.tensor(g["R"].reshape(64, 9), device=DEV)
    cfg = _cfg(1, 0, gains, dt)
    # one env x 64 sequential calls
    state = torch.zeros(1, 4, device=DEV)
    out, deg = torch.zeros(64, 3, device=DEV), torch.zeros(64, device=DEV)
    for t in range(64):
        _pid_act(cfg, R[t:t + 1], 0, 9, None, None, 0, state, 1, out[t:t + 1], deg[t:t + 1])
    pitch, roll, deg_ref = PR.angles(g["R"][:, 2])
    B = PR.bound(2, *gains, dt, 64, max(np.abs(pitch).max(), np.abs(roll).max()))
    err = np.abs(out.cpu().numpy() - g["ctrl"]).max()
    print(f"golden on the GPU: max error {err:.3e}, B(2) = {B:.3e}")
    assert err <= B
    np.testing.assert_allclose(deg.cpu().numpy(), deg_ref, rtol=1e-6)
    np.testing.assert_allclose(deg.cpu().numpy(), g["angle"], rtol=1e-6)
    # 64 envs x 1 call == 64 fresh first steps
    state64 = torch.zeros(64, 4, device=DEV)
    out64, deg64 = torch.zeros(64, 3, device=DEV), torch.zeros(64, device=DEV)
    _pid_act(cfg, R, 0, 9, None, None, 0, state64, 64, out64, deg64)
    one_state, one_out, one_deg = torch.zeros(64, 4, device=DEV), torch.zeros(64, 3, device=DEV), torch.zeros(64, device=DEV)
    for e in range(64):
        _pid_act(cfg, R[e:e + 1], 0, 9, None, None, 0, one_state[e:e + 1], 1, one_out[e:e + 1], one_deg[e:e + 1])
    for a, b in ((out64, one_out), (deg64, one_deg), (state64, one_state)):
        assert torch.equal(_bits(a), _bits(b))


def test_clamp_with_a_large_gain():
    """k_p = 1e4: every command is exactly +-limit, with the sign of the reference's unclamped command.
    The rows are those whose three unclamped reference commands all exceed 100 in magnitude."""
    rng = np.random.default_rng(21)
    rv = rng.normal(0, 0.25, (600, 3)).astype(np.float32)
    gains = (1e4, 15.0, 2.0)
    row3 = PR.third_rows(rv)
    _, u, _ = PR.BatchRef(len(rv), DT, *gains).act(row3)
    mix = np.stack([u[:, 1].astype(np.float64) * c + u[:, 0].astype(np.float64) * s for c, s in zip(PR.MIX_C, PR.MIX_S)], 1)
    keep = (np.abs(mix) > 100).all(1)
    assert keep.sum() >= 300
    rv, mix = rv[keep], mix[keep]
    n = len(rv)
    for limit in (10.0, 2.5):
        state, out = torch.zeros(n, 4, device=DEV), torch.zeros(n, 3, device=DEV)
        _pid_act(_cfg(0, 0, gains, limit=limit), torch.tensor(rv, device=DEV), 0, 3, None, None, 0, state, n, out, None)
        assert np.array_equal(out.cpu().numpy(), np.where(mix > 0, limit, -limit).astype(np.float32))


def test_a_nan_row_stays_in_its_row():
    n, bad = 130, 64
    obs, sp, _ = make_rotvec_case(n)
    clean = torch.tensor(obs[0], device=DEV)
    dirty = clean.clone()
    dirty[bad, 9:12] = float("nan")
    res = []
    for o in (clean, dirty):
        state, out, deg = torch.zeros(n, 4, device=DEV), torch.zeros(n, 3, device=DEV), torch.zeros(n, device=DEV)
        _pid_act(_cfg(), o, 9, 15, torch.tensor(sp[0], device=DEV), None, 0, state, n, out, deg)
        res.append((state, out, deg))
    others = torch.arange(n, device=DEV) != bad
    for a, b in zip(*res):
        assert torch.equal(_bits(a[others]), _bits(b[others]))
        assert torch.isnan(b[bad]).all()


def test_argument_errors_and_zero_rows():
    N = _N()
    check_pid_argument_errors(N)
    state, out, obs = _guarded(0, 4), _guarded(0, 3), torch.zeros(4, 15, device=DEV)
    assert N.lib().bb_pid_act(C.byref(_cfg()), _p(obs), 15, None, None, 0, _p(state), 0, _p(out), None, None) == 0
    torch.cuda.synchronize()
    assert (state == SENTINEL).all() and (out == SENTINEL).all()


def test_graph_replays_equal_eager_calls():
    """One captured act(): three replays against three eager calls of a twin controller, state included."""
    from ballbot_gym.controllers import BatchedPID

    n = 200
    obs_seq = torch.tensor(make_rotvec_case(n)[0][:4], device=DEV)
    captured, eager = (BatchedPID(n, *GAINS, dt=DT, device=DEV) for _ in range(2))
    obs = obs_seq[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up: the setpoints are filled here, so the capture holds one kernel
        captured.act(obs, setpoint_r=-0.02, setpoint_p=0.01)
    torch.cuda.current_stream().wait_stream(side)
    captured.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.act(obs, setpoint_r=-0.02, setpoint_p=0.01)
    assert not captured.state.any()  # a capture runs nothing
    for t in range(1, 4):
        obs.copy_(obs_seq[t])
        graph.replay()
        a, d = eager.act(obs_seq[t], setpoint_r=-0.02, setpoint_p=0.01)
        assert a.abs().max() > 0
        for x, y in ((captured.actions, a), (captured.angle_deg, d), (captured.state, eager.state)):
            assert torch.equal(_bits(x), _bits(y)), t


def _flat_env(n, **kw):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device=DEV, precision="fp64", terrain_config={"type": "flat", "config": {}}, **kw)


def test_closed_loop_holds_the_one_degree_circle():
    """17 flat envs, gains 20/15/2, 1500 steps: env 0 with zero setpoints, envs 1-16 on the sixteen
    headings (cos, sin)(2 pi k / 16) of the 1 degree circle (pitch, roll).  No done flag ever; the tilt
    stays under test_oracle.py's 5 degrees (oracle: 1.50); env 0 stays within 0.1 m (oracle 0.021 m),
    every other env travels more than 0.1 m (oracle minimum 0.217 m)."""
    from ballbot_gym.controllers import BatchedPID

    env = _flat_env(17)
    try:
        pid = BatchedPID(env, 20, 15, 2)
        k = np.arange(16)
        sp = np.zeros((17, 2), np.float32)
        sp[1:, 0], sp[1:, 1] = np.radians(np.cos(2 * np.pi * k / 16)), np.radians(np.sin(2 * np.pi * k / 16))
        sp_p, sp_r = torch.tensor(sp[:, 0], device=DEV), torch.tensor(sp[:, 1], device=DEV)
        obs, _ = env.reset()
        flags = torch.zeros(17, dtype=torch.uint8, device=DEV)
        worst = torch.zeros(17, device=DEV)
        start = None
        for t in range(1500):
            a, deg = pid.act(obs, setpoint_r=sp_r, setpoint_p=sp_p)
            worst = torch.maximum(worst, deg)
            obs, _, done = env.step_flags(a)
            flags |= done
            if start is None:  # one step from the reset position (the base moves well under a millimetre in it)
                start = env.pos2d.clone()
        dist = (env.pos2d - start).norm(dim=1).cpu().numpy()
        print(f"closed loop: worst tilt {worst.max().item():.3f} deg, env 0 moved {dist[0]:.4f} m, "
              f"headings {dist[1:].min():.3f} to {dist[1:].max():.3f} m")
        assert not flags.any()
        assert worst.max().item() < 5.0
        assert dist[0] < 0.1
        assert (dist[1:] > 0.1).all()
    finally:
        env.close()


def test_auto_reset_clears_the_controller_rows():
    """8 envs, max_ep_steps 40, setpoint (1 degree, 0), 100 steps; env 3 is tipped over at step 10 and
    fails alone.  A CPU controller given the same observations and the done flags of the step before
    as its reset mask follows every row within the state tolerance (m = 2, T = steps since the row's
    reset); the step after a termination the row is a fresh controller's: integral == fl32(prev_err dt)."""
    from ballbot_gym.controllers import BatchedPID

    n, sp_p = 8, float(np.radians(1.0))
    env = _flat_env(n, max_ep_steps=40)
    try:
        pid = BatchedPID(env, *GAINS)
        cpu = BatchedPID(n, *GAINS, dt=env.opt_timestep)
        obs, _ = env.reset()
        ended = torch.zeros(n, dtype=torch.bool)
        age = np.zeros(n, np.int64)
        amax, resets = 0.0, 0
        for t in range(100):
            a, _ = pid.act(obs, setpoint_p=sp_p)
            cpu.act(obs.cpu(), setpoint_p=sp_p, reset=ended)
            age = np.where(ended.numpy(), 1, age + 1)
            pitch, roll, _ = PR.angles(PR.third_rows(obs[:, 9:12].cpu().numpy()))
            amax = max(amax, float(np.abs(pitch).max()), float(np.abs(roll).max()))
            ulp = float(np.spacing(np.float32(amax)))
            g, c = pid.state.cpu().numpy(), cpu.state.numpy()
            assert (np.abs(g[:, :2] - c[:, :2]) <= age[:, None] * DT * 2 * ulp).all(), t
            assert (np.abs(g[:, 2:] - c[:, 2:]) <= 2 * ulp).all(), t
            for e in range(n):  # a fresh row's integral is its first error times dt; a continuing row's is not
                first = np.array_equal(g[e, :2], (g[e, 2:] * np.float32(DT)).astype(np.float32))
                assert first == bool(age[e] == 1), (t, e, g[e])
            resets += int(ended.sum())
            if t == 10:
                q, v, w, s = env.get_state()
                q[3, 3:7] = [np.cos(np.radians(15.0)), *(np.sin(np.radians(15.0)) * np.array([0.6, 0.8, 0.0]))]
                env.set_state(q, v, w, s)
            obs, _, term, _, info = env.step(a)
            ended = term.cpu()
            if t == 10:
                assert ended.tolist() == [e == 3 for e in range(n)] and bool(info["failure"][3])
        assert env.opt_timestep == DT
        assert resets == 1 + 2 * (n - 1) + 2  # env 3 alone at step 10, then every env after each 40 steps of its own
    finally:
        env.close()


def test_evaluate_policy_balance_and_install_check(capsys):
    from ballbot_gym.controllers import BatchedPID, balance, main
    from ballbot_rl.evaluation.evaluate import evaluate_policy

    env = _flat_env(4, max_ep_steps=200)
    try:
        pid = BatchedPID(env, *GAINS)
        pid.reset()
        res = evaluate_policy(pid, env, n_eval_episodes=4)
        assert res["episode_lengths"] == [200] * 4
        assert len(res["episode_rewards"]) == 4 and np.isfinite(res["episode_rewards"]).all()
        out = balance(env, pid, 200)
        assert set(out) == {"steps", "failed", "max_angle_deg", "G_tau", "pos2d"}
        assert out["steps"].tolist() == [200] * 4 and not out["failed"].any()
        assert out["max_angle_deg"].shape == (4,) and (out["max_angle_deg"] < 5).all()
        assert np.isfinite(out["G_tau"]).all() and out["pos2d"].shape == (4, 2)
    finally:
        env.close()
    assert main(["--num-envs", "4", "--steps", "300"]) == 0
    printed = capsys.readouterr().out
    assert printed.count("successfuly balanced robot for 299 steps") == 4 and printed.count("G_tau==") == 4
    assert "failed!" not in printed
