"""PID balance control: the reference's PID (ballbot_gym/controllers/pid.py) and a batched form.

`PID` is the reference's class on CPU torch, one env at a time, for the install check
(scripts/test_pid.py) and as a classical baseline.  `BatchedPID` runs the same recurrence for N envs:
on a GPU through bb_pid_act (csrc/bb_pid.hip, one launch per call, graph-capturable), on CPU
tensors through `pid_rows`, the vectorised float32 torch restatement that `PID` is with N = 1.
`balance` is the loop of the reference's script on a BallbotVecEnv.  `BatchedPID.rollout` and
`balance(fused=True)` run K steps of that loop inside one launch (bb_pid_rollout, csrc/bb_kernels.hip:
pid_rollout_kernel), with the per-step loop's bits under the env's serial route.

Angles: only the third row of R enters, roll = atan2(R21, R22), pitch = atan2(-R20,
sqrt(R21^2 + R22^2)).  A rotation vector gives that row by Rodrigues in float64, rounded to float32.
The kernel takes the two angles in double and rounds once; the torch path uses float32 atan2 as the
reference does, so the two agree to about an ulp of the angle.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch

# float(cos / sin(deg2rad(0, 120, 240))) of the double values (reference pid.py:96-98)
_MIX_C = tuple(float(np.float32(np.cos(np.deg2rad(a)))) for a in (0, 120, 240))
_MIX_S = tuple(float(np.float32(np.sin(np.deg2rad(a)))) for a in (0, 120, 240))
_DONE_TERMINATED = 1  # BB_DONE_TERMINATED


def rotvec_third_row(rotvec: torch.Tensor) -> torch.Tensor:
    """f32[N, 3] rotation vectors -> f32[N, 3], the third row of R: Rodrigues in float64 with
    identity below 1e-14 rad, rounded to float32 (bb_pid.h: pid_third_row)."""
    v = rotvec.to(torch.float64)
    th = torch.sqrt((v * v).sum(1))
    small = th < 1e-14
    k = v / torch.where(small, torch.ones_like(th), th).unsqueeze(1)
    s, c1 = torch.sin(th), 1.0 - torch.cos(th)
    kx, ky, kz = k[:, 0], k[:, 1], k[:, 2]
    row = torch.stack([-s * ky + c1 * (kx * kz), s * kx + c1 * (ky * kz), 1.0 - c1 * (kx * kx + ky * ky)], 1)
    ident = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=v.device)
    return torch.where(small.unsqueeze(1), ident, row).to(torch.float32)


def pid_rows(row3: torch.Tensor, setpoint: torch.Tensor, integral: torch.Tensor, prev_err: torch.Tensor, dt: float,
             k_p: float, k_i: float, k_d: float):
    """The reference's PID.act (pid.py:61-101) for N rows in float32 torch.  row3 f32[N, 3] is the
    third row of each R; setpoint f32[N, 2] (pitch, roll); integral f32[N, 2] is advanced in place;
    prev_err f32[N, 2] is read.  -> (u f32[N, 2], err f32[N, 2], angle_deg f64[N])."""
    roll = torch.atan2(row3[:, 1], row3[:, 2])
    pitch = torch.atan2(-row3[:, 0], torch.sqrt(row3[:, 1] ** 2 + row3[:, 2] ** 2))
    err = torch.stack([setpoint[:, 0] - pitch, setpoint[:, 1] - roll], 1)
    integral += err * dt
    derivative = (err - prev_err) / dt
    u = k_p * err + k_i * integral + k_d * derivative
    angle = torch.acos(row3[:, 2].to(torch.float64).clamp(-1.0, 1.0)) * (180.0 / math.pi)
    return u, err, angle


def motor_mix(u: torch.Tensor, limit: float) -> torch.Tensor:
    """u f32[N, 2] (pitch, roll) -> the three motor commands (120 degree spacing), clamped to +-limit."""
    ctrl = torch.stack([u[:, 1] * c + u[:, 0] * s for c, s in zip(_MIX_C, _MIX_S)], 1)
    return torch.clamp(ctrl, min=-limit, max=limit)


class PID:
    """The reference's PID controller (install check and classical baseline), CPU torch.

    Attributes as in the reference: k_p, k_i, k_d, dt, integral, prev_err, err_hist and
    return_in_pitch_roll_space."""

    def __init__(self, dt, k_p, k_i, k_d):
        self.k_p = k_p
        self.k_i = k_i
        self.k_d = k_d
        self.dt = dt

        self.integral = torch.zeros(2)
        self.prev_err = torch.zeros(2)

        self.err_hist = []
        self.integral_hist = []
        self.derivative_hist = []

        self.return_in_pitch_roll_space = False

    def act(self, R_mat: torch.Tensor, setpoint_r=0, setpoint_p=0):
        """R_mat: float32 3x3 rotation matrix -> (ctrl, angle_in_degrees): three motor commands
        clamped to +-10, or u (pitch, roll) with return_in_pitch_roll_space."""
        with torch.no_grad():
            row3 = torch.as_tensor(R_mat, dtype=torch.float32)[2].reshape(1, 3)
            sp = torch.tensor([[float(setpoint_p), float(setpoint_r)]], dtype=torch.float32)
            u, err, angle = pid_rows(row3, sp, self.integral.view(1, 2), self.prev_err.view(1, 2), float(self.dt),
                                     float(self.k_p), float(self.k_i), float(self.k_d))
            self.prev_err = err.reshape(2)
            self.err_hist.append(self.prev_err.reshape(1, 2).numpy())
            angle_in_degrees = angle.item()
            if self.return_in_pitch_roll_space:
                return u.reshape(2), angle_in_degrees
            return motor_mix(u, 10.0).reshape(3), angle_in_degrees


class BatchedPID:
    """PID.act for N envs at once.

    `env_or_num_envs`: a BallbotVecEnv (num_envs, device and dt = env.opt_timestep come from it, and
    the controller is bound to env.done: a row whose env terminated in the last step is cleared before
    the next action, so an auto-reset env starts its episode with a fresh controller) or a number of
    envs (then `dt` is required; `device` defaults to the CPU).  `space`: "motor" (three commands
    clamped to +-limit) or "pitch_roll" (u, unclamped).

    `state` is f32[N, 4]: integral (pitch, roll), prev_err (pitch, roll).  The outputs of act() are
    buffers of the controller's own with stable pointers, rewritten by every call.  On a GPU one call
    is one kernel launch on the current stream (plus a fill when the setpoints change), with no sync
    and no host read."""

    def __init__(self, env_or_num_envs, k_p, k_i, k_d, dt: Optional[float] = None, device=None, limit: float = 10.0,
                 space: str = "motor"):
        if space not in ("motor", "pitch_roll"):
            raise ValueError(f'space must be "motor" or "pitch_roll", got {space!r}')
        self.env = None
        if hasattr(env_or_num_envs, "num_envs"):
            self.env = env_or_num_envs
            self.num_envs = int(self.env.num_envs)
            device = self.env.device if device is None else device
            dt = float(self.env.opt_timestep) if dt is None else dt
        else:
            self.num_envs = int(env_or_num_envs)
            device = "cpu" if device is None else device
        if dt is None:
            raise ValueError("BatchedPID needs dt when it is not given an env")
        if self.num_envs < 1:
            raise ValueError(f"num_envs must be >= 1, got {self.num_envs}")
        if not float(dt) > 0 or not float(limit) > 0:
            raise ValueError(f"dt and limit must be > 0, got {dt} and {limit}")
        self.device = torch.device(device)
        self.k_p, self.k_i, self.k_d, self.dt, self.limit = float(k_p), float(k_i), float(k_d), float(dt), float(limit)
        self.space = space
        n, dev = self.num_envs, self.device
        self.state = torch.zeros(n, 4, dtype=torch.float32, device=dev)
        self.actions = torch.zeros(n, 3 if space == "motor" else 2, dtype=torch.float32, device=dev)
        self.angle_deg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.setpoint = torch.zeros(n, 2, dtype=torch.float32, device=dev)  # (pitch, roll)
        self._setpoint_host = (0.0, 0.0)  # the floats the buffer was last filled with; None after tensors
        if self.device.type == "cuda":
            from .. import _native as N

            if "bb_pid_act" not in N.EXPORTS:
                raise RuntimeError("this build has no bb_pid_act")
            N.lib()  # a missing library is an error here, not at the first act()

    # ---------------------------------------------------------------- state
    def reset(self, mask: Optional[torch.Tensor] = None) -> None:
        """Clear the controller state of every env (mask None) or of the masked ones."""
        if mask is None:
            self.state.zero_()
        else:
            m = torch.as_tensor(mask, device=self.device).reshape(self.num_envs) != 0
            self.state.masked_fill_(m.unsqueeze(1), 0.0)

    def _set_setpoints(self, setpoint_r, setpoint_p) -> None:
        if not isinstance(setpoint_r, torch.Tensor) and not isinstance(setpoint_p, torch.Tensor):
            host = (float(setpoint_p), float(setpoint_r))
            if host != self._setpoint_host:  # unchanged floats add no launch (one act() is one graph node)
                self.setpoint[:, 0] = host[0]
                self.setpoint[:, 1] = host[1]
                self._setpoint_host = host
            return
        for col, v in ((0, setpoint_p), (1, setpoint_r)):
            if isinstance(v, torch.Tensor):
                self.setpoint[:, col] = v.to(device=self.device, dtype=torch.float32).reshape(self.num_envs)
            else:
                self.setpoint[:, col] = float(v)
        self._setpoint_host = None

    # ------------------------------------------------------------------ act
    def _orientation(self, obs) -> torch.Tensor:
        if isinstance(obs, dict):
            obs = obs["orientation"]
        if obs.dim() != 2 or obs.shape[0] != self.num_envs or obs.shape[1] not in (3, 15):
            raise ValueError(f"obs must be f32[{self.num_envs}, 15], an f32[{self.num_envs}, 3] orientation or an obs "
                             f"dict with \"orientation\", got shape {tuple(obs.shape)}")
        return obs[:, 9:12] if obs.shape[1] == 15 else obs

    def _check(self, t: torch.Tensor, what: str) -> torch.Tensor:
        if t.device != self.device:
            raise ValueError(f"{what} is on {t.device}, the controller on {self.device}")
        return t if t.dtype == torch.float32 else t.to(torch.float32)

    def act(self, obs, setpoint_r=0.0, setpoint_p=0.0, reset: Optional[torch.Tensor] = None):
        """-> (actions f32[N, 3] (or [N, 2] in pitch/roll space), angle_deg f32[N]).  `obs`: f32[N, 15],
        an f32[N, 3] orientation (rotation vectors) or an obs dict with "orientation"; setpoints in
        radians, floats or f32[N]; `reset`: rows to clear first (bool / uint8 [N])."""
        self._set_setpoints(setpoint_r, setpoint_p)
        return self._run(self._check(self._orientation(obs), "obs"), 0, reset)

    def act_R(self, R: torch.Tensor, setpoint_r=0.0, setpoint_p=0.0, reset: Optional[torch.Tensor] = None):
        """act() on rotation matrices f32[N, 3, 3] (PID.act's R_mat)."""
        if R.dim() != 3 or tuple(R.shape) != (self.num_envs, 3, 3):
            raise ValueError(f"R must be f32[{self.num_envs}, 3, 3], got shape {tuple(R.shape)}")
        self._set_setpoints(setpoint_r, setpoint_p)
        return self._run(self._check(R, "R").reshape(self.num_envs, 9), 1, reset)

    def predict(self, obs, deterministic: bool = True) -> torch.Tensor:
        """The policy interface of evaluate_policy and VideoRecorder: the actions for `obs` with the
        setpoints of the last act() (zero at the start).  Call reset() before an evaluation."""
        return self._run(self._check(self._orientation(obs), "obs"), 0, None)[0]

    def _run(self, rows: torch.Tensor, kind: int, reset):
        with torch.no_grad():
            if self.device.type != "cuda":
                return self._run_torch(rows, kind, reset)
            from .. import _native as N

            flags, mask = None, 0
            if self.env is not None:
                if reset is not None:
                    self.reset(reset)
                flags, mask = self.env.done, _DONE_TERMINATED
            elif reset is not None:
                flags = torch.as_tensor(reset, device=self.device).reshape(self.num_envs)
                flags = flags.view(torch.uint8) if flags.dtype == torch.bool else (flags != 0).view(torch.uint8)
                flags, mask = flags.contiguous(), 0xFF
            if rows.stride(1) != 1 or rows.stride(0) < rows.shape[1]:
                rows = rows.contiguous()
            cfg = N.PIDCfg(self.dt, self.k_p, self.k_i, self.k_d, self.limit, kind,
                           N.PID_MOTOR if self.space == "motor" else N.PID_PITCH_ROLL)
            p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            N.check(N.lib().bb_pid_act(C.byref(cfg), p(rows), int(rows.stride(0)), p(self.setpoint), p(flags), mask,
                                       p(self.state), self.num_envs, p(self.actions), p(self.angle_deg), stream),
                    "bb_pid_act")
            return self.actions, self.angle_deg

    # -------------------------------------------------------------- rollout
    # trace name -> (bb_pid_rollout_args field, trailing shape, dtype)
    TRACES = {"actions": ("buf_actions", (3,), torch.float32), "angle_deg": ("buf_angle_deg", (), torch.float32),
              "obs": ("buf_obs", (15,), torch.float32), "reward": ("buf_reward", (), torch.float32),
              "done": ("buf_flags", (), torch.uint8), "terminal_obs": ("buf_terminal_obs", (15,), torch.float32),
              "pos2d": ("buf_pos2d", (2,), torch.float32)}

    def _rollout_setpoints(self, k: int, setpoint_r, setpoint_p):
        """-> the [K, N, 2] schedule, or None after filling the controller's own [N, 2] buffer."""
        n = self.num_envs
        sched = [isinstance(v, torch.Tensor) and v.dim() == 2 for v in (setpoint_p, setpoint_r)]
        for v in (setpoint_p, setpoint_r):
            if isinstance(v, torch.Tensor) and tuple(v.shape) not in ((n,), (k, n)):
                raise ValueError(f"a setpoint must be a float, f32[{n}] or f32[{k}, {n}], got shape {tuple(v.shape)}")
        if not any(sched):
            self._set_setpoints(setpoint_r, setpoint_p)
            return None
        seq = torch.empty(k, n, 2, dtype=torch.float32, device=self.device)
        for col, v in ((0, setpoint_p), (1, setpoint_r)):
            seq[:, :, col] = v.to(device=self.device, dtype=torch.float32) if isinstance(v, torch.Tensor) else float(v)
        self.setpoint.copy_(seq[-1])  # where K act() calls would have left the controller's setpoints
        self._setpoint_host = None
        return seq

    def _launch_rollout(self, k: int, setpoint_r, setpoint_p, traces: Dict[str, torch.Tensor], summary=None) -> None:
        """One bb_pid_rollout launch of k steps; summary: the seven tensors of PID_ROLLOUT_SUMMARY, in order."""
        if self.env is None:
            raise ValueError("rollout() needs a controller bound to an env (BatchedPID(env, ...))")
        if self.device.type != "cuda":
            raise ValueError("rollout() runs on a GPU; this controller is on the CPU (use act() and env.step())")
        if self.space != "motor":
            raise ValueError('rollout() steps the env on motor commands: the controller must have space="motor"')
        if int(k) < 1:
            raise ValueError(f"k_steps must be >= 1, got {k}")
        from .. import _native as N

        with torch.no_grad():
            env, k = self.env, int(k)
            seq = self._rollout_setpoints(k, setpoint_r, setpoint_p)
            p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
            args = N.PIDRolloutArgs()
            args.cfg = N.PIDCfg(self.dt, self.k_p, self.k_i, self.k_d, self.limit, N.PID_ROTVEC, N.PID_MOTOR)
            args.n_steps = k
            args.setpoint, args.setpoint_seq = (None, p(seq)) if seq is not None else (p(self.setpoint), None)
            args.state, args.obs, args.done = p(self.state), p(env.obs), p(env.done)
            args.reward, args.terminal_obs, args.pos2d = p(env.reward), p(env.terminal_obs), p(env.pos2d)
            for name, t in traces.items():
                setattr(args, self.TRACES[name][0], p(t))
            if summary is not None:
                for name, t in zip(N.PID_ROLLOUT_SUMMARY, summary):
                    setattr(args, name, p(t))
            env.run_pid_rollout(args)

    def rollout(self, k_steps: int, setpoint_r=0.0, setpoint_p=0.0, trace=(), out: Optional[dict] = None) -> dict:
        """k_steps x (act, env.step) of the bound env in ONE launch (bb_pid_rollout), on the env's own
        obs / done / reward / terminal_obs / pos2d buffers and this controller's `state`: afterwards the
        env and the controller's state and setpoints are where k_steps act() + step() calls would have left
        them, bit for bit under the env's serial route, so the two forms can be mixed freely.  (The
        `actions` / `angle_deg` output buffers of act() are not rewritten: trace them.)  Setpoints in
        radians: floats, f32[N], or f32[K, N] for a schedule (row t at step t).  `trace` names the
        per-step buffers to keep, from "actions" [K,N,3], "angle_deg" [K,N], "obs" [K,N,15], "reward"
        [K,N], "done" [K,N] uint8, "terminal_obs" [K,N,15], "pos2d" [K,N,2]; -> the dict of them.  `out`
        (a dict returned before, same K and names) is refilled instead of allocating.  An env that
        records episode logs needs "terminal_obs" and "done".  No sync, no host read."""
        names = (trace,) if isinstance(trace, str) else tuple(trace)
        for name in names:
            if name not in self.TRACES:
                raise ValueError(f"unknown trace {name!r}; choose from {sorted(self.TRACES)}")
        k, n = int(k_steps), self.num_envs
        reuse = out is not None and set(out) == set(names) and all(int(t.shape[0]) == k for t in out.values())
        if not reuse:
            out = {name: torch.empty((max(k, 0), n) + self.TRACES[name][1], dtype=self.TRACES[name][2],
                                     device=self.device) for name in names}
        self._launch_rollout(k, setpoint_r, setpoint_p, out)
        return out

    def _run_torch(self, rows: torch.Tensor, kind: int, reset):
        if reset is not None:
            self.reset(reset)
        row3 = rows[:, 6:9] if kind == 1 else rotvec_third_row(rows)
        u, err, angle = pid_rows(row3, self.setpoint, self.state[:, 0:2], self.state[:, 2:4], self.dt, self.k_p,
                                 self.k_i, self.k_d)
        self.state[:, 2:4] = err
        self.actions.copy_(motor_mix(u, self.limit) if self.space == "motor" else u)
        self.angle_deg.copy_(angle.to(torch.float32))
        return self.actions, self.angle_deg


def balance(env, controller, n_steps: int, setpoint_r=0.0, setpoint_p=0.0, gamma: float = 0.999999,
            callback=None, fused: bool = False, chunk: int = 500) -> Dict[str, np.ndarray]:
    """The loop of the reference's scripts/test_pid.py:38-65 on a BallbotVecEnv: reset, then n_steps of
    controller.act and env.step.  Each env is followed until its first episode ends; everything is
    accumulated on the device and read once at the end.  `callback(step, env)`, if given, runs after
    every step (the install check renders its video frames there).  `fused`: the same loop as
    ceil(n_steps / chunk) bb_pid_rollout launches with the accumulators inside (a controller bound to
    a GPU env, motor space; no callback) -- the same dict, bit for bit under the env's serial route;
    `chunk` bounds how long one launch holds the GPU.  -> per env
      "steps"     steps survived (n_steps when the episode never ended),
      "failed"    the episode ended on the failure flag (tilt past max_allowed_tilt),
      "max_angle_deg" the largest tilt the controller saw,
      "G_tau"     sum_t gamma^t reward_t (float64),
      "pos2d"     the last base position of the episode."""
    if fused and callback is not None:
        raise ValueError("balance(fused=True) runs whole chunks of steps per launch: a per-step callback needs "
                         "fused=False")
    if fused and int(chunk) < 1:
        raise ValueError(f"chunk must be >= 1, got {chunk}")
    obs, _ = env.reset()
    controller.reset()
    n, dev = env.num_envs, env.device
    if fused:
        total, chunk = int(n_steps), int(chunk)
        alive = torch.ones(n, dtype=torch.uint8, device=dev)
        steps = torch.zeros(n, dtype=torch.int64, device=dev)
        failed = torch.zeros(n, dtype=torch.uint8, device=dev)
        max_angle = torch.zeros(n, dtype=torch.float32, device=dev)
        g_tau = torch.zeros(n, dtype=torch.float64, device=dev)
        pos = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        # gamma^t by Python's pow, as the unfused loop's `gamma ** t`: the kernel never calls pow
        weights = torch.tensor([gamma ** t for t in range(total)], dtype=torch.float64).to(dev)
        for t0 in range(0, total, chunk):
            k = min(chunk, total - t0)
            sp = [v[t0:t0 + k] if isinstance(v, torch.Tensor) and v.dim() == 2 else v for v in (setpoint_r, setpoint_p)]
            controller._launch_rollout(k, sp[0], sp[1], {},
                                       (weights[t0:t0 + k], alive, steps, failed, max_angle, g_tau, pos))
        packed = torch.cat([steps.double().unsqueeze(1), failed.double().unsqueeze(1), max_angle.double().unsqueeze(1),
                            g_tau.unsqueeze(1), pos.double()], 1).cpu().numpy()  # the one host read
        return {"steps": packed[:, 0].astype(np.int64), "failed": packed[:, 1] != 0,
                "max_angle_deg": packed[:, 2].astype(np.float32), "G_tau": packed[:, 3],
                "pos2d": packed[:, 4:6].astype(np.float32)}
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    steps = torch.zeros(n, dtype=torch.int64, device=dev)
    failed = torch.zeros(n, dtype=torch.bool, device=dev)
    max_angle = torch.zeros(n, dtype=torch.float32, device=dev)
    g_tau = torch.zeros(n, dtype=torch.float64, device=dev)
    pos = torch.zeros(n, 2, dtype=torch.float32, device=dev)
    for t in range(int(n_steps)):
        actions, angle = controller.act(obs, setpoint_r=setpoint_r, setpoint_p=setpoint_p)
        max_angle = torch.where(alive, torch.maximum(max_angle, angle), max_angle)
        obs, reward, terminated, _, info = env.step(actions)
        steps += alive
        g_tau += torch.where(alive, reward.double() * (gamma ** t), 0.0)
        pos = torch.where(alive.unsqueeze(1), info["pos2d"], pos)
        failed |= alive & terminated & info["failure"]
        alive = alive & ~terminated
        if callback is not None:
            callback(t, env)
    packed = torch.cat([steps.double().unsqueeze(1), failed.double().unsqueeze(1), max_angle.double().unsqueeze(1),
                        g_tau.unsqueeze(1), pos.double()], 1).cpu().numpy()  # the one host read
    return {"steps": packed[:, 0].astype(np.int64), "failed": packed[:, 1] != 0,
            "max_angle_deg": packed[:, 2].astype(np.float32), "G_tau": packed[:, 3],
            "pos2d": packed[:, 4:6].astype(np.float32)}
