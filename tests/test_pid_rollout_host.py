"""bb_pid_rollout without a GPU: its argument errors, the PIDRolloutArgs mirror against the header,
balance()'s accumulation step (csrc/bb_pid.h: pid_summary_step, through
tests/hostcheck/pid_rollout_check.cpp) against a numpy restatement of balance()'s own lines, bit for
bit, and the Python-side refusals of BatchedPID.rollout and balance(fused=True)."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
SRC = ROOT / "tests" / "hostcheck" / "pid_rollout_check.cpp"
EXE = ROOT / "tests" / "_build" / "pid_rollout_check"
GAINS = (20.0, 15.0, 2.0)
DT = 0.002
SUMMARY = ("weights", "alive", "steps", "failed", "max_angle", "g_tau", "sum_pos2d")


@pytest.fixture(scope="module")
def native():
    from ballbot_gym import _native

    _native.build()  # no-op when up to date
    return _native


# ------------------------------------------------------------------ the C-ABI
def _args(native, **over):
    """Valid arguments (16 stands for any non-NULL pointer; nothing is dereferenced before the checks)."""
    a = native.PIDRolloutArgs()
    a.cfg = native.PIDCfg(DT, *GAINS, 10.0, native.PID_ROTVEC, native.PID_MOTOR)
    a.n_steps = 4
    a.state, a.obs, a.done = 16, 16, 16
    for k, v in over.items():
        if k in ("dt", "limit", "orient_kind", "space"):
            setattr(a.cfg, k, v)
        else:
            setattr(a, k, v)
    return a


PID_ROLLOUT_ARGUMENT_ERRORS = (
    # (handle, argument overrides or None for NULL args) -> message
    (None, {}, "bb_pid_rollout: NULL handle"),
    (16, None, "bb_pid_rollout: NULL args"),
    (16, {"n_steps": 0}, "bb_pid_rollout: n_steps must be >= 1 (got 0)"),
    (16, {"n_steps": -3}, "bb_pid_rollout: n_steps must be >= 1 (got -3)"),
    (16, {"dt": 0.0}, "bb_pid_rollout: dt must be > 0"),
    (16, {"dt": -0.002}, "bb_pid_rollout: dt must be > 0"),
    (16, {"limit": 0.0}, "bb_pid_rollout: limit must be > 0"),
    (16, {"orient_kind": 1}, "bb_pid_rollout: orient_kind must be BB_PID_ROTVEC"),
    (16, {"space": 1}, "bb_pid_rollout: space must be BB_PID_MOTOR"),
    (16, {"setpoint": 16, "setpoint_seq": 16}, "bb_pid_rollout: setpoint and setpoint_seq are both set"),
    (16, {"weights": 16}, "bb_pid_rollout: the summary is partly set (1 of 7"),
    (16, {k: 16 for k in SUMMARY if k != "g_tau"}, "bb_pid_rollout: the summary is partly set (6 of 7"),
    (16, {"state": None}, "bb_pid_rollout: state/obs/done must be non-NULL"),
    (16, {"obs": None}, "bb_pid_rollout: state/obs/done must be non-NULL"),
    (16, {"done": None}, "bb_pid_rollout: state/obs/done must be non-NULL"),
)


def check_pid_rollout_argument_errors(native):
    """Every listed call returns < 0 with its message and touches no memory (the handle 16 is never read:
    the argument checks come first).  The BB_REWARD_NONE refusal needs a handle: tests/test_gpu_pid_rollout.py."""
    L = native.lib()
    for handle, over, msg in PID_ROLLOUT_ARGUMENT_ERRORS:
        a = None if over is None else _args(native, **over)
        assert L.bb_pid_rollout(handle, None if a is None else C.byref(a), 1, None) < 0, msg
        assert msg in native.last_error(), (msg, native.last_error())


def test_pid_rollout_argument_errors_without_gpu(native):
    assert "bb_pid_rollout" in native.EXPORTS and native.ABI_VERSION == 21
    check_pid_rollout_argument_errors(native)


def test_pid_rollout_args_mirror_matches_the_header(tmp_path, native):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    py = native.PIDRolloutArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ballbot_mi355x.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(bb_pid_rollout_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(bb_pid_rollout_args, {f}));' for f, _ in py._fields_]
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split(None, 1) for line in
               subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n"))
    assert int(got["size"]) == C.sizeof(py) == 32 + 8 * 22
    assert len(py._fields_) == 24
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f
    assert py.cfg.size == C.sizeof(native.PIDCfg) == 28 and py.n_steps.offset == 28
    assert tuple(native.PID_ROLLOUT_SUMMARY) == SUMMARY


# ------------------------------------------------------------------ the shared summary step
def make_summary_case(n=12, T=90, seed=4):
    """A recorded (reward, flags, angle_deg, pos2d) sequence of auto-resetting envs: env e % 3 == 0 never
    ends, e % 3 == 1 ends at the step limit (flags 1) every 20 + e steps, e % 3 == 2 ends by failure
    (flags 3) at step 7 + 4 e and at the step limit later; the steps after an ending go on with other
    values (the next episode), which the accumulators must not take."""
    rng = np.random.default_rng(seed)
    reward = rng.normal(0.02, 0.01, (T, n)).astype(np.float32)
    angle = np.abs(rng.normal(1.0, 2.0, (T, n))).astype(np.float32)
    pos2d = rng.normal(0, 0.3, (T, n, 2)).astype(np.float32)
    flags = np.zeros((T, n), np.uint8)
    for e in range(n):
        if e % 3 == 1:
            flags[20 + e - 1::20 + e, e] = 1
        if e % 3 == 2:
            flags[7 + 4 * e, e] = 3
            flags[7 + 4 * e + 25::25, e] = 1
    flags[5, 0] = 4  # a divergence reset ends nothing
    angle[T - 1] += 50.0  # larger than anything before: only the envs still alive may take it
    return reward, flags, angle, pos2d


def balance_restated(reward, flags, angle, pos2d, gamma):
    """balance()'s accumulator lines (ballbot_gym/controllers/pid.py) in numpy, in their order."""
    T, n = reward.shape
    alive = np.ones(n, bool)
    steps = np.zeros(n, np.int64)
    failed = np.zeros(n, bool)
    max_angle = np.zeros(n, np.float32)
    g_tau = np.zeros(n, np.float64)
    pos = np.zeros((n, 2), np.float32)
    for t in range(T):
        terminated, failure = (flags[t] & 1) != 0, (flags[t] & 2) != 0
        max_angle = np.where(alive, np.maximum(max_angle, angle[t]), max_angle)
        steps += alive
        g_tau += np.where(alive, reward[t].astype(np.float64) * (gamma ** t), 0.0)
        pos = np.where(alive[:, None], pos2d[t], pos)
        failed |= alive & terminated & failure
        alive = alive & ~terminated
    return alive, failed, steps, max_angle, g_tau, pos


@pytest.fixture(scope="module")
def summary_check():
    EXE.parent.mkdir(parents=True, exist_ok=True)
    srcs = [SRC, CSRC / "bb_pid.h"]
    if not EXE.exists() or any(EXE.stat().st_mtime < s.stat().st_mtime for s in srcs):
        subprocess.run(["hipcc", "-x", "c++", "-O2", "-ffp-contract=off", "-std=c++17", f"-I{CSRC}", "-o", str(EXE),
                        str(SRC)], check=True, capture_output=True)

    def run(tmp, weights, reward, flags, angle, pos2d):
        T, n = reward.shape
        inp, outp = tmp / "sum_in.bin", tmp / "sum_out.bin"
        with open(inp, "wb") as f:
            f.write(np.array([n, T, 0, 0], np.int32).tobytes())
            for a, dt in ((weights, np.float64), (reward, np.float32), (flags, np.uint8), (angle, np.float32),
                          (pos2d, np.float32)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
        subprocess.run([str(EXE), str(inp), str(outp)], check=True)
        raw = outp.read_bytes()
        assert len(raw) == n * (1 + 1 + 8 + 4 + 8 + 8)
        out, at = [], 0
        for dt, w in ((np.uint8, 1), (np.uint8, 1), (np.int64, 1), (np.float32, 1), (np.float64, 1), (np.float32, 2)):
            size = n * w * np.dtype(dt).itemsize
            out.append(np.frombuffer(raw[at:at + size], dt).reshape((n, 2) if w == 2 else (n,)))
            at += size
        return out

    return run


def test_summary_step_equals_balance_restated_bit_for_bit(summary_check, tmp_path):
    gamma = 0.999999
    reward, flags, angle, pos2d = make_summary_case()
    T, n = reward.shape
    weights = np.array([gamma ** t for t in range(T)], np.float64)  # Python's pow, as balance()
    alive, failed, steps, max_angle, g_tau, pos = summary_check(tmp_path, weights, reward, flags, angle, pos2d)
    r_alive, r_failed, r_steps, r_max, r_g, r_pos = balance_restated(reward, flags, angle, pos2d, gamma)
    # the case has all three kinds of env
    assert r_alive.any() and (~r_alive & ~r_failed).any() and r_failed.any()
    assert (r_steps[r_alive] == T).all() and (r_steps[~r_alive] < T).all()
    assert np.array_equal(alive != 0, r_alive) and np.array_equal(failed != 0, r_failed)
    assert set(np.unique(alive)) <= {0, 1} and set(np.unique(failed)) <= {0, 1}
    assert np.array_equal(steps, r_steps)
    assert max_angle.tobytes() == r_max.tobytes()
    assert g_tau.tobytes() == r_g.tobytes(), np.abs(g_tau - r_g).max()
    assert pos.tobytes() == r_pos.tobytes()
    assert (r_max[~r_alive] < 50).all() and (r_max[r_alive] > 50).all()  # frozen after the ending


def test_summary_step_propagates_a_nan_angle(summary_check, tmp_path):
    """torch.maximum's NaN: an alive env's max_angle becomes NaN and stays; an ended env's does not."""
    reward, flags, angle, pos2d = make_summary_case(n=3, T=30)
    angle[12, :] = np.nan  # env 2 failed at step 15: still alive; give env 1 an ending before it
    flags[:, 1] = 0
    flags[4, 1] = 1
    out = summary_check(tmp_path, np.ones(30), reward, flags, angle, pos2d)
    assert np.isnan(out[3][0]) and not np.isnan(out[3][1]) and np.isnan(out[3][2])


# ------------------------------------------------------------------ Python-side refusals
def test_rollout_and_fused_balance_refusals_without_gpu():
    from ballbot_gym.controllers import BatchedPID, balance

    pid = BatchedPID(4, *GAINS, dt=DT)  # unbound, on the CPU
    with pytest.raises(ValueError, match="bound to an env"):
        pid.rollout(8)
    with pytest.raises(ValueError, match="unknown trace"):
        pid.rollout(8, trace=("actions", "wheels"))

    class FakeEnv:  # a bound controller on the CPU: the env is never touched
        num_envs, device, opt_timestep = 4, torch.device("cpu"), DT

    bound = BatchedPID(FakeEnv(), *GAINS)
    with pytest.raises(ValueError, match="runs on a GPU"):
        bound.rollout(8)
    with pytest.raises(ValueError, match="callback"):
        balance(FakeEnv(), bound, 10, fused=True, callback=lambda t, e: None)
    with pytest.raises(ValueError, match="chunk"):
        balance(FakeEnv(), bound, 10, fused=True, chunk=0)
