"""The fp64 reference of the world-view image: what csrc/bb_view.hip is held to.

TEST INFRASTRUCTURE ONLY.  The image is this project's own definition, so this file *is* the
definition, carried out in numpy float64.  It takes the surfaces' ray parameters from
tests/render_ref.py (sphere_entry, segment_entry, _Field, _tiles: local-frame quadratics and brute
force over the heightfield's triangles) and adds what the depth cameras do not have:

  camera    MuJoCo's free camera: lookat = base origin + lookat_offset, forward
            f = (cos e cos a, cos e sin a, sin e), up u = (-sin e cos a, -sin e sin a, cos e),
            right = f x u, origin = lookat - distance f; pixel (i, j), row 0 on top, looks along
            right xc + up yc + f, xc = (2 (j + 1/2) / W - 1) (W / H) tan(fovy / 2),
            yc = (1 - 2 (i + 1/2) / H) tan(fovy / 2).  d is that direction normalised.
  clip      nearest front hit in (1.4142e-3 len, 14.142 len), len the direction's length.
  normal    the unit outward normal n at the hit: sphere and capsules away from the nearest point
            of the centre / segment; the cylinder's side away from its axis, its discs along it
            (the face nearer to the hit point); the ground's hit triangle, turned to face the ray.
            The triangle is the one of the 3x3 cells around the hit point whose plane passes
            closest to it among those that contain it.
  colour    base (0.25 + 0.45 max(0, n_z) + 0.30 max(0, -n.d)), uint8 int(255 c + 0.5); base
            colours in BASE / checker() / ball_tone(); background unshaded.
  class     per pixel, what the base colour hangs on besides the surface id: the ground's checker
            parity, the ball's sign, and the hit triangle.

stable_reference() renders five samples (centre and +-3e-5 in normalised image coordinates along
x and y) and marks a pixel stable when all five agree in surface id, colour class and triangle and
both second differences of the depth are <= 1e-6.  Everything is decided by this file alone,
never by the code under test.
"""
from __future__ import annotations

import numpy as np

from render_ref import HF_N, SHIFT, CURVE, ZNEAR, _Field, _tiles, segment_entry, sphere_entry

ZFAR = 14.142135623730951  # ballbot.xml:8 zfar * extent
NONE, GROUND, BALL, TOWER, STICK0, WHEEL0 = 0, 1, 2, 3, 4, 6
BACKGROUND = np.array([0.55, 0.70, 0.90])
GROUND_EVEN, GROUND_ODD = np.array([0.42, 0.45, 0.48]), np.array([0.30, 0.33, 0.36])
BALL_POS, BALL_NEG = np.array([0.90, 0.45, 0.10]), np.array([0.20, 0.12, 0.08])
BASE = {TOWER: (0.18, 0.80, 0.44), 4: (0.18, 0.80, 0.44), 5: (0.18, 0.80, 0.44),
        6: (1.0, 0.0, 0.0), 7: (0.0, 1.0, 0.0), 8: (0.0, 0.0, 1.0)}

DEFAULT_CAM = dict(azimuth=90.0, elevation=-20.0, distance=2.5, lookat_offset=(0.0, 0.0, 0.2), fovy=45.0)


def cam(**kw):
    c = dict(DEFAULT_CAM)
    c.update(kw)
    return c


def free_camera(base, azimuth, elevation, distance, lookat_offset, **_):
    """(origin, R) of MuJoCo's free camera; R's columns are right, up, -forward (camera -> world)."""
    a, e = np.deg2rad(azimuth), np.deg2rad(elevation)
    f = np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
    u = np.array([-np.sin(e) * np.cos(a), -np.sin(e) * np.sin(a), np.cos(e)])
    right = np.cross(f, u)
    lookat = np.asarray(base, np.float64) + np.asarray(lookat_offset, np.float64)
    return lookat - distance * f, np.stack([right, u, -f], axis=1)


def view_rays(R, H, W, fovy, offset=(0.0, 0.0)):
    """Unit world directions [H*W, 3] and the camera-frame lengths [H*W] of the pixel rays."""
    th = np.tan(np.deg2rad(fovy) / 2)
    j = np.arange(W) + 0.5 + offset[0]
    i = np.arange(H) + 0.5 + offset[1]
    xc = (2 * j / W - 1) * (W / H) * th
    yc = (1 - 2 * i / H) * th
    dc = np.empty((H, W, 3))
    dc[..., 0] = xc[None, :]
    dc[..., 1] = yc[:, None]
    dc[..., 2] = -1.0
    dc = dc.reshape(-1, 3)
    ln = np.sqrt((dc * dc).sum(1))
    return (dc @ np.asarray(R, np.float64).T) / ln[:, None], ln


def quat_matrix(q):
    """Rotation matrix (body -> world) of the quaternion (w, x, y, z), normalised first."""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def view_scene(prims, qpos):
    """The scene of one env: the primitives of oracle_lib.render_scene (the camera fields are not
    used) plus the base origin and the ball's rotation from qpos."""
    s = {k: prims[k] for k in ("ball", "ball_r", "pa", "pb", "rad", "cyl", "half")}
    s["base"] = np.asarray(qpos[0:3], np.float64).copy()
    s["RB"] = quat_matrix(qpos[13:17])
    return s


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _segment_normal(p, pa, pb, r, cylinder):
    ax = pb - pa
    length = np.sqrt(ax @ ax)
    w, hh, mid = ax / length, length / 2, (pa + pb) / 2
    rel = p - mid
    z = rel @ w
    if not cylinder:
        return _unit(rel - np.clip(z, -hh, hh)[:, None] * w)
    radial = rel - z[:, None] * w
    side = np.abs(np.sqrt((radial * radial).sum(1)) - r) < np.abs(np.abs(z) - hh)
    return np.where(side[:, None], _unit(radial), np.sign(z)[:, None] * w)


def _triangles(field, p):
    """(triangle index 2 (r HF_N + c) + upper, upward unit normal) of the ground points p [m, 3]."""
    m = p.shape[0]
    c0 = np.floor((p[:, 0] + field.sx) / field.dx).astype(int)
    r0 = np.floor((p[:, 1] + field.sy) / field.dy).astype(int)
    best = np.full(m, np.inf)
    tri = np.full(m, -1)
    nrm = np.zeros((m, 3))
    pad = 1e-9
    for dr in (0, -1, 1):
        for dc in (0, -1, 1):
            r, c = r0 + dr, c0 + dc
            ok = (r >= 0) & (r <= HF_N - 2) & (c >= 0) & (c <= HF_N - 2)
            rr, cc = np.clip(r, 0, HF_N - 2), np.clip(c, 0, HF_N - 2)
            zA, zB = field.z[rr, cc], field.z[rr + 1, cc]
            zC, zD = field.z[rr, cc + 1], field.z[rr + 1, cc + 1]
            uu = (p[:, 0] - field.xs[cc]) / field.dx
            vv = (p[:, 1] - field.ys[rr]) / field.dy
            inside = ok & (uu >= -pad) & (vv >= -pad) & (uu <= 1 + pad) & (vv <= 1 + pad)
            for upper in (0, 1):
                if upper:
                    gx, gy = (zD - zB) / field.dx, (zD - zC) / field.dy
                    zp = zD + gx * (uu - 1) * field.dx + gy * (vv - 1) * field.dy
                    cont = inside & (uu + vv >= 1 - pad)
                else:
                    gx, gy = (zC - zA) / field.dx, (zB - zA) / field.dy
                    zp = zA + gx * uu * field.dx + gy * vv * field.dy
                    cont = inside & (uu + vv <= 1 + pad)
                res = np.where(cont, np.abs(zp - p[:, 2]), np.inf)
                got = res < best
                best[got] = res[got]
                tri[got] = 2 * (rr[got] * HF_N + cc[got]) + upper
                nrm[got] = _unit(np.stack([-gx, -gy, np.ones(m)], 1))[got]
    assert (best < 1e-7).all(), float(best.max())  # every ground hit lies on a triangle
    return tri, nrm


def checker(p):
    """Parity of the world-xy checker of 0.5 m squares at the points p."""
    return (np.floor(p[:, 0] / 0.5) + np.floor(p[:, 1] / 0.5)).astype(np.int64) & 1


def ball_tone(RB, n):
    """1 where the outward normal, in the ball's body frame, has a negative coordinate product."""
    nb = n @ RB  # rows: RB^T n
    return (nb[:, 0] * nb[:, 1] * nb[:, 2] < 0).astype(np.int64)


def render(scene, hf, size_z, H, W, camera=None, offset=(0.0, 0.0)):
    """One sample of the image: dict of depth [H, W] (metres along the optical axis, ZFAR where
    nothing is hit), ids int8, cls and tri (colour class and hit triangle, -1 off the ground),
    n [H, W, 3], c float [H, W, 3] and rgb uint8 [H, W, 3]."""
    camera = camera or DEFAULT_CAM
    o, R = free_camera(scene["base"], **camera)
    d, ln = view_rays(R, H, W, camera["fovy"], offset)
    tmin = ZNEAR * ln
    best = ZFAR * ln
    ids = np.zeros(H * W, np.int8)

    def see(t, sid):
        got = (t > tmin) & (t < best)
        best[got] = t[got]
        ids[got] = sid

    see(sphere_entry(o, d, scene["ball"], scene["ball_r"]), BALL)
    for k in range(6):
        see(segment_entry(o, d, scene["pa"][k], scene["pb"][k], scene["rad"][k], bool(scene["cyl"][k])), TOWER + k)
    field = _Field(hf, size_z, scene["half"], np.float64)
    hit = np.zeros(H * W, bool)
    for idx in _tiles(H, W):
        field.cast(o, d, tmin, best, hit, idx)
    ids[hit] = GROUND

    p = o[None, :] + best[:, None] * d
    n = np.zeros((H * W, 3))
    base = np.tile(BACKGROUND, (H * W, 1))
    cls = np.zeros(H * W, np.int64)
    tri = np.full(H * W, -1, np.int64)
    g = ids == GROUND
    if g.any():
        tri[g], up = _triangles(field, p[g])
        n[g] = np.where(((up * d[g]).sum(1) > 0)[:, None], -up, up)
        cls[g] = checker(p[g])
        base[g] = np.where(cls[g][:, None] == 1, GROUND_ODD, GROUND_EVEN)
    b = ids == BALL
    if b.any():
        n[b] = _unit(p[b] - scene["ball"])
        cls[b] = ball_tone(scene["RB"], n[b])
        base[b] = np.where(cls[b][:, None] == 1, BALL_NEG, BALL_POS)
    for k in range(6):
        s = ids == TOWER + k
        if s.any():
            n[s] = _segment_normal(p[s], scene["pa"][k], scene["pb"][k], scene["rad"][k], bool(scene["cyl"][k]))
            base[s] = BASE[TOWER + k]
    shade = 0.25 + 0.45 * np.maximum(0, n[:, 2]) + 0.30 * np.maximum(0, -(n * d).sum(1))
    c = np.where((ids == NONE)[:, None], base, base * shade[:, None])
    rgb = np.floor(255 * c + 0.5).astype(np.uint8)
    return {"depth": (best / ln).reshape(H, W), "ids": ids.reshape(H, W), "cls": cls.reshape(H, W),
            "tri": tri.reshape(H, W), "n": n.reshape(H, W, 3), "d": d.reshape(H, W, 3), "c": c.reshape(H, W, 3),
            "rgb": rgb.reshape(H, W, 3)}


def stable_reference(scene, hf, size_z, H, W, camera=None):
    """The reference of one image: rgb uint8 [H, W, 3], ids, the stable mask, and what an unstable
    pixel may show: the five samples' ids [5, H, W] and the min / max of their rgb."""
    ex, ey = SHIFT * W / 2, SHIFT * H / 2
    s = [render(scene, hf, size_z, H, W, camera, off) for off in ((0, 0), (ex, 0), (-ex, 0), (0, ey), (0, -ey))]
    same = np.ones((H, W), bool)
    for t in s[1:]:
        same &= (t["ids"] == s[0]["ids"]) & (t["cls"] == s[0]["cls"]) & (t["tri"] == s[0]["tri"])
    d0 = s[0]["depth"]
    stable = same & (np.abs(s[1]["depth"] + s[2]["depth"] - 2 * d0) <= CURVE) \
        & (np.abs(s[3]["depth"] + s[4]["depth"] - 2 * d0) <= CURVE)
    five = np.stack([t["rgb"] for t in s]).astype(np.int16)
    return {"rgb": s[0]["rgb"], "ids": s[0]["ids"], "stable": stable, "ids5": np.stack([t["ids"] for t in s]),
            "lo": five.min(0), "hi": five.max(0), "depth": d0, "n": s[0]["n"], "d": s[0]["d"], "c": s[0]["c"]}


# ------------------------------------------------------------------ cases
N_ENVS = 8
CLOSE = [cam(lookat_offset=(0.0, 0.0, -0.12), distance=0.4, elevation=-10.0, azimuth=az) for az in (30.0, 150.0, 270.0)]
CAMERAS = {"default": cam(), "close30": CLOSE[0], "close150": CLOSE[1], "close270": CLOSE[2]}
# (family, H, W, precision, camera) of every kernel test; the CPU test checks the reference's own
# conditions on the same images
CASES = (
    ("tilt", 24, 32, "fp64", "default"), ("edge", 17, 23, "fp32", "default"), ("lift", 33, 47, "fp64", "default"),
    ("tilt", 33, 47, "fp32", "close30"), ("edge", 24, 32, "fp64", "close150"), ("lift", 17, 23, "fp64", "close270"),
    ("lift", 24, 32, "fp32", "close150"), ("edge", 17, 23, "fp64", "close270"),
    ("tilt", 5, 3, "fp64", "default"), ("edge", 5, 3, "fp32", "close30"), ("tilt", 1, 1, "fp32", "default"),
    ("lift", 1, 1, "fp64", "close270"),
)


def case_poses(family, fields, q0, precision):
    """qpos [N_ENVS, 17] of a case: render_ref's pose family over the bank, rounded to float32 for
    an fp32 case (the state an fp32 handle holds)."""
    from render_ref import poses

    Q = poses(family, fields, q0, n=N_ENVS)
    return Q.astype(np.float32).astype(np.float64) if precision == "fp32" else Q


def references(oracle, fields, Q, H, W, camera):
    """stable_reference of every env of a case; env e stands on fields[e % len(fields)]."""
    return [stable_reference(view_scene(oracle.render_scene(Q[e], 0), Q[e]), *fields[e % len(fields)], H, W, camera)
            for e in range(Q.shape[0])]
