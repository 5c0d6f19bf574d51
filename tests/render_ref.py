"""A plain numpy ray caster for the depth cameras: the reference that both
oracle/bb_oracle.c:bbo_render_depth and csrc/bb_render.hip are held to.

TEST INFRASTRUCTURE ONLY.  It shares the *scene* with the oracle (camera pose,
ball, six segments: bbo_render_scene, kinematics held by forward parity and
test_oracle.py::_cam_pose) and nothing of the surface mathematics:

  primitives   intersected in the primitive's own frame (axis on z): the circle
               quadratic of the side limited to |z| <= half height, discs
               (cylinder) or the outer hemispheres of two spheres (capsule) as
               caps.  Of all candidate points the nearest whose outward normal
               faces the ray is the entry; it is seen if it lies beyond
               znear * len.  A convex body has one entry per line, so an origin
               inside it (entry behind) or an entry nearer than the clip leaves
               the primitive unseen.
  heightfield  no DDA: every triangle of every cell in the xy bounding box of a
               tile's ray segments, as a plane z(x, y) over its half cell, two
               sided, nearest hit in (tmin, best).  Triangulation of the collision
               prisms: cell (r, c) -> (r,c)(r+1,c)(r,c+1) and (r+1,c)(r,c+1)(r+1,c+1).
  pixels       centres at (j + 0.5, i + 0.5) + offset, fovy 90, x scaled by W/H,
               row 0 on top, depth = t / len clipped to 1.

render() returns the depth and a surface id per pixel.  stable_reference()
renders five samples (centre and +-3e-5 in normalised image coordinates along x
and y) and marks a pixel stable when all five see the same surface and both
second differences of the depth are <= 1e-6: the depth is then locally linear
and no silhouette lies within the shift, a few hundred times the float error of
a camera pose.  Everything is decided by this file alone, never by the code
under test.
"""
from __future__ import annotations

import numpy as np

HF_N = 293
ZNEAR = 1e-4 * 14.142135623730951  # ballbot.xml:8 znear * extent
NONE, GROUND, BALL, TOWER, STICK0, WHEEL0 = 0, 1, 2, 3, 4, 6  # stick k = 4 + k, wheel k = 6 + k
SHIFT = 3e-5        # stable-pixel shift, normalised image coordinates
CURVE = 1e-6        # stable-pixel bound on the second differences
_LEAF = 30_000      # rays x cells handled in one brute-force block


def pixel_rays(R, H, W, offset=(0.0, 0.0), dtype=np.float64):
    """Unit world directions [H*W, 3] and the camera-frame lengths [H*W] of the pixel rays."""
    f = np.dtype(dtype).type
    j = (np.arange(W, dtype=dtype) + f(0.5)) + f(offset[0])
    i = (np.arange(H, dtype=dtype) + f(0.5)) + f(offset[1])
    xc = (f(2) * j / f(W) - f(1)) * (f(W) / f(H))
    yc = f(1) - f(2) * i / f(H)
    dc = np.empty((H, W, 3), dtype)
    dc[..., 0] = xc[None, :]
    dc[..., 1] = yc[:, None]
    dc[..., 2] = f(-1)
    dc = dc.reshape(-1, 3)
    ln = np.sqrt((dc * dc).sum(1))
    d = (dc @ np.asarray(R, dtype).T) / ln[:, None]
    return d, ln


def _entry(best, t, ok):
    return np.where(ok & (t < best), t, best)


def sphere_entry(o, d, c, r):
    """Ray parameter of the front-face point of a sphere (inf: none); |d| = 1."""
    p = o - c
    b = d @ p
    disc = b * b - (p @ p - r * r)
    s = np.sqrt(np.maximum(disc, 0))
    best = np.full(d.shape[0], np.inf, d.dtype)
    for sg in (-1, 1):
        t = -b + sg * s
        n = p[None, :] + t[:, None] * d  # outward normal (unnormalised)
        best = _entry(best, t, (disc >= 0) & ((n * d).sum(1) < 0))
    return best


def segment_entry(o, d, pa, pb, r, cylinder):
    """Ray parameter of the front-face point of a capped cylinder or a capsule on the
    segment pa-pb (inf: none), in the frame whose z axis is the segment; |d| = 1."""
    dt = d.dtype
    ax = pb - pa
    length = np.sqrt(ax @ ax)
    w = ax / length
    e = np.zeros(3, dt)
    e[int(np.argmin(np.abs(w)))] = 1
    u = np.cross(w, e)
    u = u / np.sqrt(u @ u)
    v = np.cross(w, u)
    B = np.stack([u, v, w]).astype(dt)
    hh = length / 2
    p = B @ (o - (pa + pb) / 2)
    q = d @ B.T
    px, py, pz = p
    qx, qy, qz = q[:, 0], q[:, 1], q[:, 2]
    best = np.full(d.shape[0], np.inf, dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        # side: (px + t qx)^2 + (py + t qy)^2 = r^2, |z| <= hh, normal (x, y, 0)
        A = qx * qx + qy * qy
        Bq = px * qx + py * qy
        disc = Bq * Bq - A * (px * px + py * py - r * r)
        s = np.sqrt(np.maximum(disc, 0))
        for sg in (-1, 1):
            t = (-Bq + sg * s) / A
            x, y, z = px + t * qx, py + t * qy, pz + t * qz
            best = _entry(best, t, (disc >= 0) & (A > 0) & (np.abs(z) <= hh) & (x * qx + y * qy < 0))
        for sg in (-1, 1):
            if cylinder:  # disc z = sg hh, normal (0, 0, sg)
                t = (sg * hh - pz) / qz
                x, y = px + t * qx, py + t * qy
                best = _entry(best, t, (qz != 0) & (x * x + y * y <= r * r) & (sg * qz < 0))
            else:  # the half of the sphere at (0, 0, sg hh) that points away from the segment
                oz = pz - sg * hh
                b = px * qx + py * qy + oz * qz
                dd = b * b - (px * px + py * py + oz * oz - r * r)
                ss = np.sqrt(np.maximum(dd, 0))
                for s2 in (-1, 1):
                    t = -b + s2 * ss
                    x, y, z = px + t * qx, py + t * qy, oz + t * qz
                    best = _entry(best, t, (dd >= 0) & (sg * z >= 0) & (x * qx + y * qy + z * qz < 0))
    return best


class _Field:
    def __init__(self, hf, size_z, half, dtype):
        f = np.dtype(dtype).type
        self.dt = dtype
        self.z = np.asarray(hf, np.float32).reshape(HF_N, HF_N).astype(dtype) * f(size_z)
        self.zmin, self.zmax = self.z.min(), self.z.max()
        self.sx, self.sy = f(half[0]), f(half[1])
        self.dx, self.dy = f(2) * self.sx / f(HF_N - 1), f(2) * self.sy / f(HF_N - 1)
        self.xs = -self.sx + np.arange(HF_N, dtype=dtype) * self.dx
        self.ys = -self.sy + np.arange(HF_N, dtype=dtype) * self.dy
        # a hit is accepted this far outside its half cell (cell units): rounding of the hit
        # point must not open a gap between two triangles; overlapping costs nothing (nearest wins)
        self.pad = f(256) * np.finfo(dtype).eps

    def window(self, o, d, t0, t1, zlo, zhi):
        """Cells (r0, r1, c0, c1, inclusive) under the parts of the segments [t0, t1] that lie in
        the slab zlo..zhi, or None."""
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (zlo - o[2]) / d[:, 2], (zhi - o[2]) / d[:, 2]
        lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
        flat = d[:, 2] == 0
        inside = (o[2] >= zlo) & (o[2] <= zhi)
        lo = np.where(flat, -np.inf if inside else np.inf, lo)
        hi = np.where(flat, np.inf if inside else -np.inf, hi)
        s0, s1 = np.maximum(t0, lo), np.minimum(t1, hi)
        live = s0 <= s1
        if not live.any():
            return None
        s0, s1, dl = s0[live], s1[live], d[live]
        x = np.concatenate([o[0] + s0 * dl[:, 0], o[0] + s1 * dl[:, 0]])
        y = np.concatenate([o[1] + s0 * dl[:, 1], o[1] + s1 * dl[:, 1]])
        c0 = int(np.floor((x.min() + self.sx) / self.dx)) - 1
        c1 = int(np.floor((x.max() + self.sx) / self.dx)) + 1
        r0 = int(np.floor((y.min() + self.sy) / self.dy)) - 1
        r1 = int(np.floor((y.max() + self.sy) / self.dy)) + 1
        if c1 < 0 or r1 < 0 or c0 > HF_N - 2 or r0 > HF_N - 2:
            return None
        return max(r0, 0), min(r1, HF_N - 2), max(c0, 0), min(c1, HF_N - 2)

    def cast(self, o, d, tmin, best, hit, idx):
        """Brute force of the rays idx (a tile of the image) against their window; splits the tile
        while rays x cells is large.  Updates best / hit in place."""
        pad_z = self.dt(1e-6)
        t0, t1 = tmin[idx], best[idx]
        win = self.window(o, d[idx], t0, t1, self.zmin - pad_z, self.zmax + pad_z)
        for _ in range(2):  # tighten the slab to the heights of the window found
            if win is None:
                return
            r0, r1, c0, c1 = win
            zz = self.z[r0:r1 + 2, c0:c1 + 2]
            win = self.window(o, d[idx], t0, t1, zz.min() - pad_z, zz.max() + pad_z)
        if win is None:
            return
        r0, r1, c0, c1 = win
        if idx.size * (r1 - r0 + 1) * (c1 - c0 + 1) > _LEAF and idx.size > 16:
            h = idx.size // 2
            self.cast(o, d, tmin, best, hit, idx[:h])
            self.cast(o, d, tmin, best, hit, idx[h:])
            return
        dd = d[idx][:, None, None, :]
        z = self.z
        zA, zB = z[r0:r1 + 1, c0:c1 + 1][None], z[r0 + 1:r1 + 2, c0:c1 + 1][None]
        zC, zD = z[r0:r1 + 1, c0 + 1:c1 + 2][None], z[r0 + 1:r1 + 2, c0 + 1:c1 + 2][None]
        x0, y0 = self.xs[c0:c1 + 1][None, None, :], self.ys[r0:r1 + 1][None, :, None]
        ox, oy = o[0] - x0, o[1] - y0  # origin relative to the cell's corner A
        tbest = np.full(idx.size, np.inf, self.dt)
        one = self.dt(1)
        # lower triangle A B C: z = zA + gx x + gy y; upper B C D: the plane through D with the
        # slopes of its own edges, written about A as well
        for lower in (True, False):
            if lower:
                gx, gy, z0 = (zC - zA) / self.dx, (zB - zA) / self.dy, zA
            else:
                gx, gy = (zD - zB) / self.dx, (zD - zC) / self.dy
                z0 = zD - gx * self.dx - gy * self.dy
            den = dd[..., 2] - gx * dd[..., 0] - gy * dd[..., 1]
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (z0 + gx * ox + gy * oy - o[2]) / den
                uu = (ox + t * dd[..., 0]) / self.dx
                vv = (oy + t * dd[..., 1]) / self.dy
                diag = (uu + vv <= one + self.pad) if lower else (uu + vv >= one - self.pad)
            ok = (den != 0) & (uu >= -self.pad) & (vv >= -self.pad) & (uu <= one + self.pad) & (vv <= one + self.pad)
            ok &= diag
            ok &= (t > t0[:, None, None]) & (t < t1[:, None, None])
            tbest = np.minimum(tbest, np.where(ok, t, np.inf).reshape(idx.size, -1).min(1))
        got = tbest < best[idx]
        best[idx[got]] = tbest[got]
        hit[idx[got]] = True


def _tiles(H, W, n=8):
    """Pixel indices grouped in n x n tiles (rays of a tile share a small window of the field)."""
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    key = ((ii // n) * ((W + n - 1) // n) + jj // n).ravel()
    order = np.argsort(key, kind="stable")
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    return np.split(order, cuts)


def render(scene, hf, size_z, H, W, offset=(0.0, 0.0), dtype=np.float64):
    """(depth dtype[H, W], surface id int8[H, W]) of a scene (oracle_lib.render_scene), every
    input rounded to dtype first and every operation carried out in it."""
    dt = np.dtype(dtype).type
    o = np.asarray(scene["o"], dtype)
    d, ln = pixel_rays(scene["R"], H, W, offset, dtype)
    tmin = dt(ZNEAR) * ln
    best = ln.copy()  # z-depth 1
    ids = np.zeros(H * W, np.int8)

    def see(t, sid):
        got = (t > tmin) & (t < best)
        best[got] = t[got]
        ids[got] = sid

    see(sphere_entry(o, d, np.asarray(scene["ball"], dtype), dt(scene["ball_r"])), BALL)
    for k in range(6):
        see(segment_entry(o, d, np.asarray(scene["pa"][k], dtype), np.asarray(scene["pb"][k], dtype),
                          dt(scene["rad"][k]), bool(scene["cyl"][k])), TOWER + k)
    field = _Field(hf, size_z, scene["half"], dt)
    hit = np.zeros(H * W, bool)
    for idx in _tiles(H, W):
        field.cast(o, d, tmin, best, hit, idx)
    ids[hit] = GROUND
    return np.minimum(best / ln, dt(1)).reshape(H, W), ids.reshape(H, W)


def stable_reference(scene, hf, size_z, H, W):
    """The float64 reference of one image: depth d [H, W], ids, the stable mask and the
    min / max of the five samples (what an unstable pixel may show)."""
    ex, ey = SHIFT * W / 2, SHIFT * H / 2
    d0, id0 = render(scene, hf, size_z, H, W)
    dxp, ixp = render(scene, hf, size_z, H, W, (ex, 0))
    dxm, ixm = render(scene, hf, size_z, H, W, (-ex, 0))
    dyp, iyp = render(scene, hf, size_z, H, W, (0, ey))
    dym, iym = render(scene, hf, size_z, H, W, (0, -ey))
    same = (ixp == id0) & (ixm == id0) & (iyp == id0) & (iym == id0)
    stable = same & (np.abs(dxp + dxm - 2 * d0) <= CURVE) & (np.abs(dyp + dym - 2 * d0) <= CURVE)
    five = np.stack([d0, dxp, dxm, dyp, dym])
    return {"d": d0, "ids": id0, "stable": stable, "lo": five.min(0), "hi": five.max(0)}


# ------------------------------------------------------------------ pose families
FAMILIES = ("tilt", "lift", "edge", "ball", "below")
SIZES = ((64, 64), (24, 40), (40, 24), (17, 23), (5, 3), (1, 1))
SIZE_Z = (2.0, 2.0, 0.5, 2.0)  # bank slots: flat, hills seed 7, hills seed 11 (low), GPU perlin
N_ENVS = 32


def bank():
    """The test bank's host-made slots: flat, hills seed 7 (size_z 2), hills seed 11 (size_z 0.5)."""
    from ballbot_gym.terrain import generate_hills_terrain

    return [np.zeros(HF_N * HF_N, np.float32), generate_hills_terrain(HF_N, seed=7).astype(np.float32).ravel(),
            generate_hills_terrain(HF_N, seed=11).astype(np.float32).ravel()]


def perlin_field():
    """The field of the GPU perlin slot (the first seed of np_random(0)), generated on the host."""
    from ballbot_gym.envs.config import np_random
    from ballbot_gym.terrain.perlin import generate_perlin_terrain

    return generate_perlin_terrain(HF_N, seed=int(np_random(0).integers(0, 10000))).astype(np.float32).ravel()


def _height(hf, size_z, x, y):
    """Highest of the four samples around (x, y): where a ball can rest."""
    g = np.asarray(hf).reshape(HF_N, HF_N)
    c = int(np.clip(np.floor((x + 5.0) / (10.0 / (HF_N - 1))), 0, HF_N - 2))
    r = int(np.clip(np.floor((y + 5.0) / (10.0 / (HF_N - 1))), 0, HF_N - 2))
    return float(g[r:r + 2, c:c + 2].max()) * size_z


def _quat(rotvec):
    from scipy.spatial.transform import Rotation as Rot

    x, y, z, w = Rot.from_rotvec(rotvec).as_quat()
    return np.array([w, x, y, z])


def _place(q0, xy, z_ground, yaw, tilt_vec, wheels, lift=0.0):
    """qpos of the robot standing on its ball at xy on ground of height z_ground, the base
    turned by yaw about z after tilt_vec (a horizontal rotation vector) about the ball's centre."""
    from scipy.spatial.transform import Rotation as Rot

    q = q0.copy()
    ballc0 = q0[10:13] + np.array([0.0, 0.0, -0.14])  # the ball geom's offset in its body
    rot = Rot.from_rotvec([0, 0, yaw]) * Rot.from_rotvec(tilt_vec)
    shift = np.array([xy[0], xy[1], z_ground + lift])
    q[0:3] = ballc0 + rot.apply(q0[0:3] - ballc0) + shift
    x, y, z, w = rot.as_quat()
    q[3:7] = [w, x, y, z]
    q[7:10] = wheels
    q[10:13] = q0[10:13] + shift
    return q


def poses(family, fields, q0, n=N_ENVS, seed=0):
    """qpos [n, 17] of a pose family; env e stands on fields[e % len(fields)] = (hf, size_z).
    Fixed seeds; wheel angles uniform in +-pi everywhere."""
    rng = np.random.default_rng(1000 + 17 * FAMILIES.index(family) + seed)
    out = np.zeros((n, 17))
    corners = [(4.95, 4.95), (-4.95, 4.95), (4.95, -4.95), (-4.95, -4.95)]
    for e in range(n):
        hf, size_z = fields[e % len(fields)]
        wheels = rng.uniform(-np.pi, np.pi, 3)
        yaw = rng.uniform(-np.pi, np.pi)
        ang = rng.uniform(-np.pi, np.pi)
        tilt = rng.uniform(0, 0.35) * np.array([np.cos(ang), np.sin(ang), 0.0])
        xy = rng.uniform(-3.0, 3.0, 2)
        k = e // len(fields)  # the k-th pose on this field
        lift = 0.0
        if family == "lift":
            lift, tilt = (0.3, 1.5)[k % 2], 0.5 * tilt
        elif family == "edge":
            tilt = 0.3 * tilt
            if k < 4:
                xy = np.array(corners[k])
            elif k == 4:  # outside the field: rays enter through the box side or miss it
                xy = np.array([5.2, rng.uniform(-4, 4)]) * rng.choice([-1, 1])
            elif k == 5:
                xy = np.array([rng.uniform(-4, 4), 5.2 * rng.choice([-1, 1])])
            else:
                xy = rng.uniform(4.5, 4.95, 2) * rng.choice([-1, 1], 2)
        elif family == "below":
            lift, tilt = -0.3, 0.3 * tilt
        q = _place(q0, xy, _height(hf, size_z, *xy), yaw, tilt, wheels, lift)
        if family == "below":  # sink the base only: the camera under the surface, the ball on it
            q[10:13] -= [0, 0, lift]
        if family == "ball":  # the ball on its free joint, relative to camera k % 2
            from scipy.spatial.transform import Rotation as Rot

            cam = k % 2
            Rb = Rot.from_quat([q[4], q[5], q[6], q[3]])
            Rc = (Rb * Rot.from_euler("XYZ", [180, -30 if cam == 0 else 30, 0], degrees=True)
                  * Rot.from_euler("XYZ", [180, 0, 0], degrees=True))
            oc = q[0:3] + Rb.apply([0.17 if cam == 0 else -0.17, -0.01, -0.06])
            mode = (k // 2) % 4
            if mode == 0:    # 5-30 cm in front of the camera (surface to origin), somewhere in view
                depth = 0.09 + rng.uniform(0.05, 0.30)
                pc = np.array([rng.uniform(-0.5, 0.5) * depth, rng.uniform(-0.5, 0.5) * depth, -depth])
            elif mode == 1:  # touching the frustum's edge: its silhouette crosses the image border
                depth = 0.09 + rng.uniform(0.05, 0.30)
                pc = np.array([depth + 0.09 * np.sqrt(2.0) * rng.uniform(-0.9, 0.9), 0.0, -depth])
                if rng.random() < 0.5:
                    pc = pc[[1, 0, 2]]
            elif mode == 2:  # containing the camera: culled
                pc = rng.uniform(-0.04, 0.04, 3)
            else:            # 3 m away
                pc = np.array([0.0, 0.0, -3.0])
            q[10:13] = oc + Rc.apply(pc) - np.array([0.0, 0.0, -0.14])
        out[e] = q
    return out


# (family, H, W, precision) of every kernel test; the CPU test runs the same families and sizes.
# 64x64 in one family only, the small sizes in tilt and edge only (the reference is the cost).
CASES = (
    ("tilt", 64, 64, "fp64"), ("lift", 24, 40, "fp64"), ("edge", 40, 24, "fp64"), ("ball", 24, 40, "fp64"),
    ("below", 17, 23, "fp64"), ("tilt", 17, 23, "fp32"), ("edge", 17, 23, "fp64"), ("edge", 24, 40, "fp32"),
    ("tilt", 5, 3, "fp64"), ("edge", 5, 3, "fp32"), ("tilt", 1, 1, "fp32"), ("edge", 1, 1, "fp64"),
    # x reaches +-5 (79 deg): the only views of the sticks, the far wheels and the rays that pass the tower
    ("tilt", 12, 60, "fp64"),
)
