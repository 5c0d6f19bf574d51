"""The shipped library's constraint solve at 1, 3 and 5 envs (a lone team, a ragged wave, a second
wave holding one team) from three states whose Newton trip counts differ, so that teams of one
wave leave the Newton loop at different iterations while the others go on through the row-wide
DPP instructions (bb_team16.h: the fused broadcast-FMAs of the factorisation, the forward sweep
and the wheel blocks need every lane of a live row active):

  fall    the robot on its ball in free fall: no ball-terrain contact (solve16's gsum false)
  rest    the robot settled on flat ground
  slip    the base tilted 0.3 rad about the ball's centre, the wheels spinning against a ball at rest

bb_forward and one bb_step against the fp64 oracle at tests/test_gpu_parity.py's bounds: qacc 1e-7
relative, qpos 1e-9, qvel 1e-6 (fp64); fp32 is held to finite outputs and the oracle's done flags.
The first test, on the CPU, holds the host build of the same solver templates to the same bounds
from the same states: the states themselves are not among the rare ones where the oracle's and
the kernel's line searches stop a Newton iteration apart (tests/test_gpu_parity.py's docstring).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

Q_TOL, V_TOL, QACC_TOL = 1e-9, 1e-6, 1e-7
ENVS = [1, 3, 5]
ACTION = np.array([0.4, -0.7, 0.2], np.float32)


def _quat_mul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def build_states(O):
    """(name, qpos, qvel, warm) of the three states, read-only (tests/test_gpu_solve_regimes.py starts from them too)."""
    hf, cfg = O.flat_hfield(), O.default_cfg()
    q0, v0, w0 = O.reset_state(0.01)
    fall_q = q0.copy()
    fall_q[2] += 0.3
    fall_q[12] += 0.3
    q, v, w = q0.copy(), v0.copy(), w0.copy()
    sc = np.zeros(1, np.int32)
    for _ in range(400):  # drop 4 cm and settle
        O.env_step(cfg, q, v, w, sc, np.zeros(3, np.float32), hf)
    rest = (q.copy(), v.copy(), w.copy())
    # the base turned 0.3 rad about the world x axis through the ball's centre (the wheels stay on
    # the ball), and wheel speeds the resting ball does not match: the wheel contacts slide
    sq = q.copy()
    th = 0.3
    R = np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])
    sq[0:3] = sq[10:13] + R @ (sq[0:3] - sq[10:13])
    sq[3:7] = _quat_mul(np.array([np.cos(th / 2), np.sin(th / 2), 0, 0]), sq[3:7])
    sv = np.zeros(15)
    sv[6:9] = [8.0, -6.0, 5.0]
    out = [("fall", fall_q, np.zeros(15), np.zeros(15)), ("rest",) + rest, ("slip", sq, sv, np.zeros(15))]
    for _, a, b, c in out:
        for x in (a, b, c):
            x.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def states(oracle):
    """The three states; computed once, never modified."""
    return build_states(oracle)


@pytest.fixture(scope="module")
def expected(oracle, states):
    """The oracle's forward (qacc, contact counts, iterations) and one env step from each state."""
    O = oracle
    hf, cfg = O.flat_hfield(), O.default_cfg()
    ctrl = ACTION.astype(np.float64) * 10.0
    out = {}
    for name, q, v, w in states:
        fo = O.forward(q, v, ctrl, w, hf)
        qe, ve, we, se = q.copy(), v.copy(), w.copy(), np.zeros(1, np.int32)
        obs, rew, flags, _, _ = O.env_step(cfg, qe, ve, we, se, ACTION, hf)
        out[name] = dict(qacc=np.array(fo.qacc), nground=fo.nground, nbody=fo.nbody, niter=fo.niter, q1=qe, v1=ve,
                         obs=obs, flags=flags & 3)
    return ctrl, out


def test_states_hold_the_bounds_on_the_host(states, expected):
    """CPU: the three states do what their names say, and the host build of the kernel's solver
    templates steps each of them within the bounds."""
    import hostcheck_lib as H

    _, exp = expected
    assert exp["fall"]["nground"] == 0 and exp["rest"]["nground"] > 0 and exp["slip"]["nground"] > 0
    assert all(e["nbody"] == 0 for e in exp.values())  # the fast kernel's envs
    assert len({e["niter"] for e in exp.values()}) > 1, "the states should differ in Newton iterations"
    hf, cfg = np.zeros(293 * 293, np.float32), H.default_cfg()
    for name, q, v, w in states:
        qe, ve, we, se = q.copy(), v.copy(), w.copy(), np.zeros(1, np.int32)
        H.env_step(cfg, qe, ve, we, se, ACTION, hf)
        eq, ev = np.abs(qe - exp[name]["q1"]).max(), np.abs(ve - exp[name]["v1"]).max()
        print(f"{name}: host vs oracle qpos {eq:.2e} qvel {ev:.2e}, oracle iterations {exp[name]['niter']}")
        assert eq <= Q_TOL and ev <= V_TOL, name


def _env(n, precision):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device="cuda:0", precision=precision, auto_reset=False,
                         terrain_config={"type": "flat", "config": {}})


def _tiled(states, n):
    pick = [states[e % 3] for e in range(n)]
    return [s[0] for s in pick], *(np.array([s[k] for s in pick]) for k in (1, 2, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("n", ENVS)
def test_forward_fused_solve(states, expected, n):
    ctrl, exp = expected
    names, qs, vs, ws = _tiled(states, n)
    env = _env(n, "fp64")
    env.set_state(qs, vs, ws)
    qacc, ncon = env.forward(ctrl)
    env.close()
    for e, name in enumerate(names):
        ref = exp[name]["qacc"]
        assert (ncon[e, 0], ncon[e, 1]) == (exp[name]["nground"], 0), (e, name)
        err = np.abs(qacc[e] - ref).max() / max(1.0, np.abs(ref).max())
        print(f"n={n} env {e} {name}: qacc error {err:.2e}")
        assert err < QACC_TOL, (e, name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENVS)
def test_step_fused_solve(states, expected, n, precision):
    _, exp = expected
    names, qs, vs, ws = _tiled(states, n)
    env = _env(n, precision)
    env.set_state(qs, vs, ws, np.zeros(n, np.int32))
    acts = torch.tensor(np.tile(ACTION, (n, 1)), device="cuda:0")
    obs, rew, term, trunc, info = env.step(acts)
    q1, v1, w1, _ = env.get_state()
    flags = info["done_flags"].cpu().numpy()
    stats = env.stats()
    env.close()
    assert np.isfinite(q1).all() and np.isfinite(v1).all() and np.isfinite(w1).all()
    assert torch.isfinite(obs).all() and torch.isfinite(rew).all()
    assert stats["diverged"] == 0 and stats["overflow"] == 0
    for e, name in enumerate(names):
        assert flags[e] & 3 == exp[name]["flags"], (e, name)
        if precision == "fp64":
            eq, ev = np.abs(q1[e] - exp[name]["q1"]).max(), np.abs(v1[e] - exp[name]["v1"]).max()
            print(f"n={n} env {e} {name}: qpos error {eq:.2e} qvel error {ev:.2e}")
            assert eq <= Q_TOL and ev <= V_TOL, (e, name, eq, ev)
