"""The fp64 reference of the onboard RGB-D image: what csrc/bb_rgbd.hip is held to.

TEST INFRASTRUCTURE ONLY.  The colour is this project's own definition, so this file *is* the
definition of the (4, H, W) frame, carried out in numpy float64.  It takes the camera (o, R) and
the primitives from oracle_lib.render_scene(q, cam), the ball's rotation from view_ref.quat_matrix,
the surfaces' ray parameters from tests/render_ref.py and the colour pieces from tests/view_ref.py
(all imported by name; neither file is edited):

  ray       the depth camera's: render_ref.pixel_rays (fovy 90, aspect W / H, row 0 on top).
  hit       nearest front-face hit with t in (ZNEAR len, ZFAR len); the colour image is not cut at
            1 m, only the depth plane is.
  D         min(t / len, 1), 1 where nothing is hit: render_ref.render's quantity.
  R, G, B   base colour (BASE, checker(), ball_tone(), background unshaded) times
            0.25 + 0.45 max(0, n_z) + 0.30 max(0, -n.d), as a count q = int(255 c + 0.5) and the
            value float32(q) / float32(255).  Normals as in view_ref (_segment_normal, _triangles,
            the ground turned to face the ray).

stable_reference() renders five samples (centre and +-3e-5 in normalised image coordinates along
x and y) and marks a pixel stable when all five agree in surface id, colour class and triangle and
both second differences of the (unclipped) depth are <= 1e-6: view_ref.stable_reference's rule.
Everything is decided by this file alone, never by the code under test.
"""
from __future__ import annotations

import functools

import numpy as np

import render_ref as RR
from render_ref import CURVE, SHIFT, ZNEAR, _Field, _tiles, pixel_rays, segment_entry, sphere_entry
from view_ref import (BACKGROUND, BALL, BALL_NEG, BALL_POS, BASE, GROUND, GROUND_EVEN, GROUND_ODD, NONE, TOWER, ZFAR,
                      _segment_normal, _triangles, _unit, ball_tone, checker, quat_matrix)

# (family, H, W, n_envs, precision of the GPU state) of every kernel test; the CPU test checks the
# reference's own conditions on the same families and sizes
CASES = (
    ("tilt", 24, 40, 16, "fp64"), ("lift", 24, 40, 16, "fp64"),
    ("edge", 17, 23, 32, "fp32"),  # 32 to reach the poses outside the field
    ("ball", 17, 23, 32, "fp64"),  # 32 to reach all four ball modes
    ("below", 17, 23, 16, "fp64"),
    ("tilt", 12, 60, 32, "fp64"), ("tilt", 5, 3, 8, "fp32"), ("edge", 1, 1, 8, "fp32"), ("tilt", 64, 64, 8, "fp64"),
)


def to_float(q):
    """A colour count as the frame stores it: float32(q) / float32(255), correctly rounded."""
    return np.asarray(q, np.float32) / np.float32(255)


def render(scene, RB, hf, size_z, H, W, offset=(0.0, 0.0)):
    """One sample of the image of a scene (oracle_lib.render_scene) with the ball rotation RB: dict of
    depth [H, W] (unclipped, ZFAR where nothing is hit), D (clipped to 1), ids int8, cls and tri (colour
    class and hit triangle, -1 off the ground), n and d [H, W, 3], c float [H, W, 3] and the counts
    q uint8 [H, W, 3]."""
    o = np.asarray(scene["o"], np.float64)
    d, ln = pixel_rays(scene["R"], H, W, offset, np.float64)
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
        cls[b] = ball_tone(RB, n[b])
        base[b] = np.where(cls[b][:, None] == 1, BALL_NEG, BALL_POS)
    for k in range(6):
        s = ids == TOWER + k
        if s.any():
            n[s] = _segment_normal(p[s], scene["pa"][k], scene["pb"][k], scene["rad"][k], bool(scene["cyl"][k]))
            base[s] = BASE[TOWER + k]
    shade = 0.25 + 0.45 * np.maximum(0, n[:, 2]) + 0.30 * np.maximum(0, -(n * d).sum(1))
    c = np.where((ids == NONE)[:, None], base, base * shade[:, None])
    q = np.floor(255 * c + 0.5).astype(np.uint8)
    depth = best / ln
    return {"depth": depth.reshape(H, W), "D": np.minimum(depth, 1.0).reshape(H, W), "ids": ids.reshape(H, W),
            "cls": cls.reshape(H, W), "tri": tri.reshape(H, W), "n": n.reshape(H, W, 3), "d": d.reshape(H, W, 3),
            "c": c.reshape(H, W, 3), "q": q.reshape(H, W, 3)}


def stable_reference(scene, RB, hf, size_z, H, W):
    """The reference of one image: counts q uint8 [H, W, 3], ids, the stable mask, and what an unstable
    pixel may show: the five samples' ids [5, H, W] and the min / max of their counts."""
    ex, ey = SHIFT * W / 2, SHIFT * H / 2
    s = [render(scene, RB, hf, size_z, H, W, off) for off in ((0, 0), (ex, 0), (-ex, 0), (0, ey), (0, -ey))]
    same = np.ones((H, W), bool)
    for t in s[1:]:
        same &= (t["ids"] == s[0]["ids"]) & (t["cls"] == s[0]["cls"]) & (t["tri"] == s[0]["tri"])
    d0 = s[0]["depth"]
    stable = same & (np.abs(s[1]["depth"] + s[2]["depth"] - 2 * d0) <= CURVE) \
        & (np.abs(s[3]["depth"] + s[4]["depth"] - 2 * d0) <= CURVE)
    five = np.stack([t["q"] for t in s]).astype(np.int16)
    return {"q": s[0]["q"], "ids": s[0]["ids"], "stable": stable, "ids5": np.stack([t["ids"] for t in s]),
            "lo": five.min(0), "hi": five.max(0), "depth": d0, "D": s[0]["D"], "cls": s[0]["cls"], "n": s[0]["n"],
            "d": s[0]["d"], "c": s[0]["c"]}


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def fields():
    """render_ref's 4-slot bank: flat, hills seed 7 (size_z 2), hills seed 11 (size_z 0.5), perlin."""
    return tuple((h, z) for h, z in zip(RR.bank() + [RR.perlin_field()], RR.SIZE_Z))


def case_poses(oracle, family, n, precision="fp64"):
    """qpos [n, 17] of a case: render_ref's pose family over the bank, rounded to float32 for an
    fp32 case (the state an fp32 handle holds)."""
    Q = RR.poses(family, fields(), oracle.reset_state(0.01)[0], n=n)
    return Q.astype(np.float32).astype(np.float64) if precision == "fp32" else Q


@functools.lru_cache(maxsize=None)
def case_references(oracle, family, H, W, n, precision="fp64"):
    """{(env, cam): stable_reference} of a case, computed once per session and shared by the tests
    that need it (nobody writes into it); env e stands on fields()[e % 4]."""
    Q = case_poses(oracle, family, n, precision)
    F = fields()
    out = {}
    for e in range(n):
        hf, size_z = F[e % len(F)]
        RB = quat_matrix(Q[e][13:17])
        for cam in (0, 1):
            out[e, cam] = stable_reference(oracle.render_scene(Q[e], cam), RB, hf, size_z, H, W)
    return out
