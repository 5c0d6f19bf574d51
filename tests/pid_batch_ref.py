"""Numpy restatement of bb_pid_act for N rows (test helper): the reference's PID.act recurrence
(ballbot_gym/controllers/pid.py:61-101) in float32, with the angles taken in float64 from the
float32 third row of R and rounded once, as csrc/bb_pid.h states them.  Written independently of the
kernel: the rotation matrix is pid_ref.rotvec_to_R's full Rodrigues product, not the row formula.

bound() is the one tolerance of the controller's tests, derived in the issue that added them:
an angle error d reaches a motor command through k_p, through the integral (at most T dt d after T
steps) and through the derivative (2 d / dt), mixed by at most |cos| + |sin| <= sqrt(2):
    B(m) = sqrt(2) (k_p + k_i dt T + 2 k_d / dt) m spacing(float32(max |angle|))
with m = 1 against this file (two double atan2 implementations can flip the float rounding by one
ulp) and m = 2 against float32 atan2 (within an ulp; the kernel within half)."""
import numpy as np

from pid_ref import rotvec_to_R

F = np.float32
MIX_C = [F(np.cos(np.deg2rad(a))) for a in (0, 120, 240)]
MIX_S = [F(np.sin(np.deg2rad(a))) for a in (0, 120, 240)]


def third_rows(rotvec):
    """f32[N, 3] rotation vectors -> f32[N, 3]: row 2 of the float64 Rodrigues matrix, rounded."""
    return np.stack([rotvec_to_R(rv)[2] for rv in np.asarray(rotvec, F)]).astype(F)


def angles(row3):
    """f32[N, 3] third rows -> (pitch f32[N], roll f32[N], angle_deg f64[N]), float64 inside."""
    r = np.asarray(row3, F).astype(np.float64)
    roll = np.arctan2(r[:, 1], r[:, 2])
    pitch = np.arctan2(-r[:, 0], np.sqrt(r[:, 1] ** 2 + r[:, 2] ** 2))
    return pitch.astype(F), roll.astype(F), np.degrees(np.arccos(np.clip(r[:, 2], -1.0, 1.0)))


class BatchRef:
    def __init__(self, n, dt, k_p, k_i, k_d, limit=10.0):
        self.dt, self.k_p, self.k_i, self.k_d, self.limit = F(dt), F(k_p), F(k_i), F(k_d), F(limit)
        self.state = np.zeros((n, 4), F)  # integral (pitch, roll), prev_err (pitch, roll)

    def act(self, row3, setpoint=None, reset=None):
        """-> (motor f32[N, 3] clamped, u f32[N, 2] (pitch, roll), angle_deg f64[N])."""
        n = len(self.state)
        if reset is not None:
            self.state[np.asarray(reset) != 0] = 0
        pitch, roll, deg = angles(row3)
        sp = np.zeros((n, 2), F) if setpoint is None else np.asarray(setpoint, F)
        err = np.stack([sp[:, 0] - pitch, sp[:, 1] - roll], 1).astype(F)
        integ = (self.state[:, :2] + (err * self.dt).astype(F)).astype(F)
        deriv = ((err - self.state[:, 2:]).astype(F) / self.dt).astype(F)
        u = ((self.k_p * err).astype(F) + (self.k_i * integ).astype(F)).astype(F)
        u = (u + (self.k_d * deriv).astype(F)).astype(F)
        self.state[:, :2], self.state[:, 2:] = integ, err
        with np.errstate(invalid="ignore"):
            motor = np.stack([((u[:, 1] * c).astype(F) + (u[:, 0] * s).astype(F)).astype(F)
                              for c, s in zip(MIX_C, MIX_S)], 1)
            clamped = np.where(motor < -self.limit, -self.limit, np.where(motor > self.limit, self.limit, motor))
        return clamped.astype(F), u, deg


def bound(m, k_p, k_i, k_d, dt, T, max_angle):
    """B(m) for T steps of a case whose largest |angle| (radians) is max_angle."""
    ulp = float(np.spacing(F(max_angle)))
    return float(np.sqrt(2.0) * (k_p + k_i * dt * T + 2.0 * k_d / dt) * m * ulp)
