"""The fast kernels' solve after the wheel Jacobian's LDS reads were batched (bb_solve.h: wheel_dot3 / wheel_jar3 in
the line-search setup and the first iteration's contact pass, bb_team16.h: the Hessian row's wheel reads issued
together): the same arithmetic in another order of issue, on the states where the wheel lanes' part of the Newton
iteration decides the result.

Directed states, flat ground, built with the oracle alone from a seed (nothing read from a file); the first five are
the directed ones, in this order, the other sixty are copies of the five (moved about the plane, under random
actions; the long one as below), so that 65 envs fill sixteen waves and leave a lone team:

  long       the settled robot turning at 3 rad/s over a ball that turns at 15 rad/s about the vertical (the ball
             slides on the ground and under the wheels): a solve of 12 or more Newton iterations, every one
             through the batched line-search setup (its copies: other turning rates, kept where the solve is long)
  free fall  the reset state, 1 cm above the ground: ng = 0, the wheel contacts are all there is, so the wheel
             lanes are the whole contact pass
  clip       the settled robot with its wheels at +-20 rad/s, where the observation clips the motor speeds (2 x the
             10 rad/s command scale): all three wheel contacts slide (the cone's middle zone)
  tilt       the base turned about the ball's centre until it leans 19.5 degrees, half a degree inside the 20 degree
             limit, at rest: the step does not terminate
  rest       upright at rest, from its own warm start

  step vs oracle    one fast-kernel step of the first 1, 3, 17 and all 65 states: qpos 1e-9, qvel 1e-6, warm start 1e-7
                    relative (tests/test_gpu_solve_regimes.py's bounds), no outlier, the oracle's flags
  fp32              the same 65 states stay finite, the oracle's done flags
  forms agree       bb_step x 20, bb_step_multi (20 steps) and the rollout kernel on the 65 envs, bit for bit
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_solve_overhead as OV  # noqa: E402
import test_gpu_solve_regimes as R  # noqa: E402

N_STATES = OV.N_STATES
ENV_COUNTS = (1, 3, 17, 65)
KINDS = ("long", "free fall", "clip", "tilt", "rest")
LONG_ITERS = 12
LONG_YAW = (3.0, 15.0)  # rad/s of the base and of the ball about the vertical through the ball's centre
CLIP_SPEED = 20.0  # rad/s: the observation's motor-speed clip
TILT_DEG = 19.5


def _tilted(q, deg):
    """q with the base turned deg degrees about the world x axis through the ball's centre (the wheels stay on
    the ball)."""
    from test_gpu_solve_fused import _quat_mul

    th = np.deg2rad(deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])
    q = q.copy()
    q[0:3] = q[10:13] + Rx @ (q[0:3] - q[10:13])
    q[3:7] = _quat_mul(np.array([np.cos(th / 2), np.sin(th / 2), 0, 0]), q[3:7])
    return q


def _tilt_deg(q):
    """The angle between the base's z axis and the vertical, in degrees (what the env's tilt limit is applied to)."""
    return float(np.degrees(np.arccos(np.clip(1 - 2 * (q[4] ** 2 + q[5] ** 2) / np.dot(q[3:7], q[3:7]), -1, 1))))


def _directed(O):
    """{kind: (qpos, qvel, warm, action)}"""
    from test_gpu_solve_fused import build_states

    base = {name: (q, v, w) for name, q, v, w in build_states(O)}
    rq, rv, rw = base["rest"]
    zero = np.zeros(3, np.float32)
    spin = np.zeros(15)
    spin[6:9] = [CLIP_SPEED, -CLIP_SPEED, CLIP_SPEED]
    q0, v0, w0 = O.reset_state(0.01)
    return {"long": (rq.copy(), R._yaw(rq, *LONG_YAW), rw.copy(), zero),
            "free fall": (q0, v0, w0, zero),
            "clip": (rq.copy(), spin, rw.copy(), zero),
            # the settled robot already leans a few degrees, about the same axis
            "tilt": (_tilted(rq, TILT_DEG - _tilt_deg(rq)), np.zeros(15), rw.copy(), zero),
            "rest": (rq.copy(), rv.copy(), rw.copy(), zero)}


@pytest.fixture(scope="module")
def overhead_states(oracle):
    """65 read-only state records (test_gpu_solve_regimes._evaluate plus "kind" and "ocells"), under the name
    that test_gpu_solve_overhead's launch-form test takes its states by."""
    O = oracle
    rng = np.random.default_rng(11)
    d = _directed(O)
    recs = []
    for i in range(N_STATES):
        kind = KINDS[i % len(KINDS)]
        for attempt in range(40):
            q, v, w, a = d[kind]
            if i >= len(KINDS) and kind == "long":  # other turning rates in the same place, until the solve is long
                v = R._yaw(q, rng.uniform(0, 3), rng.uniform(5, 30))
                a = (rng.uniform(-1, 1, 3) * 0.01).astype(np.float32)
            elif i >= len(KINDS):  # the same state elsewhere on the plane, under another action
                x, y = rng.uniform(-2, 2, 2)
                q = q.copy()
                q[[0, 10]] += x
                q[[1, 11]] += y
                # (clip: a small one, a full torque can lift a wheel's contact out of the cone's middle zone)
                a = (rng.uniform(-1, 1, 3) * (0.01 if kind == "clip" else 1.0)).astype(np.float32)
            # kept: the fast kernel's (no base-tree contact), and the oracle's own stop is not ambiguous
            rec = [r for r in R._evaluate(O, "flat", [(q, v, w, a)])
                   if r["ambig"] <= R.AMBIG_TOL and (kind != "long" or r["niter"] >= LONG_ITERS)]
            if rec:
                break
            assert i >= len(KINDS), f"the directed state '{kind}' is not what it is for"
        assert rec, f"no usable variant of '{kind}' in 40 draws"
        rec[0]["kind"] = kind
        recs += rec
    for r in recs:
        k = r["kind"]
        r["ocells"] = [k]
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return recs


def test_states_are_what_they_are_for(overhead_states):
    """CPU, from the oracle alone."""
    recs = overhead_states
    assert [r["kind"] for r in recs[:5]] == list(KINDS)
    by = {k: [r for r in recs if r["kind"] == k] for k in KINDS}
    print("\n" + "; ".join(f"{k}: ng {sorted({r['ng'] for r in v})} niter {sorted({r['niter'] for r in v})}"
                           for k, v in by.items()))
    assert len(recs) == N_STATES and all(r["ambig"] <= R.AMBIG_TOL for r in recs)
    assert all(r["niter"] >= LONG_ITERS for r in by["long"]), [r["niter"] for r in by["long"]]
    assert all(r["ng"] == 0 and len(r["zw"]) == 3 and r["niter"] >= 1 for r in by["free fall"])
    assert all(r["zw"] == [1, 1, 1] for r in by["clip"]), [r["zw"] for r in by["clip"]]
    tilts = [_tilt_deg(r["q"]) for r in by["tilt"]]
    assert all(19.0 < t < 20.0 for t in tilts), tilts
    assert all(not (int(r["flags"]) & 3) for r in by["tilt"]), "the tilt state terminates"
    assert all(len(r["zw"]) == 3 and r["ng"] >= 1 for r in by["rest"])


def test_batched_rows_on_host():
    """CPU: tests/hostcheck/lds_batch_check.cpp, wheel_dot3 / wheel_jar3 against three wheel_dot calls on random J
    and x, every wheel, floats and doubles, bit for bit."""
    import subprocess
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    src, exe = root / "tests" / "hostcheck" / "lds_batch_check.cpp", root / "tests" / "_build" / "lds_batch_check"
    csrc = root / "openballbot-rl_amd" / "csrc"
    exe.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", f"-I{csrc}", "-o", str(exe), str(src)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_fast_step_vs_oracle(overhead_states, n, monkeypatch):
    recs = overhead_states[:n]
    OV._against_oracle(recs, R._step_on_gpu("flat", recs, "fp64", monkeypatch))


@pytest.mark.gpu
def test_fast_step_fp32_finite(overhead_states, monkeypatch):
    OV.test_fast_step_fp32_finite(overhead_states, monkeypatch)


@pytest.mark.gpu
def test_launch_forms_bit_equal(overhead_states, monkeypatch):
    """65 flat envs x 20 steps from the directed states: the rollout kernel, 20 bb_step calls and one
    bb_step_multi launch (test_gpu_solve_overhead's comparison, on these states)."""
    OV.test_launch_forms_bit_equal(overhead_states, monkeypatch)
