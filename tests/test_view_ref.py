"""The world-view image's fp64 reference (tests/view_ref.py): analytic pins of the reference
itself, and the conditions the GPU test (test_gpu_view.py) rests on, asserted here on the same
images so that the GPU test cannot hide behind them:

  * in every case image at least 95 % of the pixels are stable;
  * over the close-up cases every surface 2-8 (ball, tower, both sticks, three wheels) covers at
    least 20 pixels in at least one image.

Measured (single run): the smallest stable share of a case is 0.974 (lift 33x47 at the default
camera); the largest coverage over the close-ups is ball 309, tower 30, sticks 61 / 60, wheels 61
pixels each.  At the default 2.5 m the ball and the wheels cover 1-3 pixels, hence the close-ups
(look-at offset (0, 0, -0.12), distance 0.4, elevation -10, azimuths 30 / 150 / 270)."""
import functools

import numpy as np
import pytest

import render_ref as RR
import view_ref as VR

FAR = np.array([0.0, 0.0, 50.0])  # beyond the far clip of any camera used here


def _scene(**kw):
    """Every primitive parked beyond the clip unless given; base at the origin."""
    s = {"base": np.zeros(3), "RB": np.eye(3), "ball": FAR.copy(), "ball_r": 0.09,
         "pa": np.tile(FAR, (6, 1)), "pb": np.tile(FAR + [0.1, 0, 0], (6, 1)), "rad": np.full(6, 0.01),
         "cyl": np.array([True, False, False, False, False, False]), "half": (5.0, 5.0)}
    s.update(kw)
    return s


FLAT = np.zeros(RR.HF_N * RR.HF_N, np.float32)


def test_default_camera_pose():
    o, R = VR.free_camera(np.array([0.3, -0.2, 0.1]), **VR.DEFAULT_CAM)
    lookat = np.array([0.3, -0.2, 0.3])
    assert np.abs(o - (lookat + [0.0, -2.3492, 0.8551])).max() < 5e-5
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
    d, ln = VR.view_rays(R, 33, 47, 45.0)  # odd sizes: the centre pixel looks along the axis
    c = (33 // 2) * 47 + 47 // 2
    assert abs(ln[c] - 1) < 1e-15
    assert np.abs(o + 2.5 * d[c] - lookat).max() < 1e-14  # the look-at point projects to the image centre
    # the corner pixels: fovy 45 spans the image's height, the width scales by W / H
    top = d[47 // 2] @ R  # camera frame
    assert abs(np.degrees(np.arctan2(top[1], -top[2])) - 22.5 * (1 - 1 / 33)) < 0.35


def test_sphere_alone_centre_normal_faces_the_camera():
    base = np.array([0.4, 0.7, 3.0])
    sc = _scene(base=base, ball=base + [0.0, 0.0, 0.2])  # the ball at the look-at point
    r = VR.render(sc, FLAT, 2.0, 33, 47)
    i, j = 16, 23
    assert r["ids"][i, j] == VR.BALL
    assert np.abs(r["n"][i, j] + r["d"][i, j]).max() < 1e-12  # n = -d
    assert abs(r["depth"][i, j] - (2.5 - 0.09)) < 1e-12
    # shade = 0.25 + 0.45 max(0, n_z) + 0.30: n_z = sin 20 deg
    want = 0.25 + 0.45 * np.sin(np.radians(20.0)) + 0.30
    tone = VR.BALL_POS if r["cls"][i, j] == 0 else VR.BALL_NEG
    assert np.abs(r["c"][i, j] - tone * want).max() < 1e-12
    assert (r["ids"] != VR.GROUND).sum() > 0 and (r["rgb"][r["ids"] == VR.NONE] == [140, 179, 230]).all()


@pytest.mark.parametrize("xy,odd", [((0.3, 0.8), True), ((0.3, 0.2), False), ((-0.3, 0.2), True), ((-0.7, -1.2), True),
                                    ((-0.7, -0.7), False)])
def test_flat_ground_from_straight_above(xy, odd):
    sc = _scene(base=np.array([xy[0], xy[1], 0.0]))
    r = VR.render(sc, FLAT, 2.0, 33, 47, VR.cam(elevation=-90.0, lookat_offset=(0.0, 0.0, 0.0), distance=1.0))
    i, j = 16, 23
    assert r["ids"][i, j] == VR.GROUND and r["cls"][i, j] == int(odd)
    base = VR.GROUND_ODD if odd else VR.GROUND_EVEN
    assert np.abs(r["c"][i, j] - base * 1.0).max() < 1e-12  # 0.25 + 0.45 + 0.30
    assert (r["rgb"][i, j] == np.floor(255 * base + 0.5)).all()
    assert abs(r["depth"][i, j] - 1.0) < 1e-12 and (r["ids"] == VR.GROUND).all()


def test_ball_tone_follows_the_ball_rotation():
    base = np.array([0.0, 0.0, 3.0])
    sc = _scene(base=base, ball=base + [0.0, 0.0, 0.2])
    near = VR.cam(distance=0.5)
    a = VR.render(sc, FLAT, 2.0, 17, 23, near)
    sc["RB"] = VR.quat_matrix([0.0, 0.0, 0.0, 1.0])  # half a turn about z: x and y flip, the product keeps its sign
    b = VR.render(sc, FLAT, 2.0, 17, 23, near)
    sc["RB"] = VR.quat_matrix([0.0, 1.0, 0.0, 0.0])  # half a turn about x: y and z flip
    c = VR.render(sc, FLAT, 2.0, 17, 23, near)
    sc["RB"] = VR.quat_matrix([np.cos(np.pi / 4), 0.0, 0.0, np.sin(np.pi / 4)])  # a quarter turn about z: the tones swap
    d = VR.render(sc, FLAT, 2.0, 17, 23, near)
    ball = a["ids"] == VR.BALL
    assert ball.sum() > 5 and len(np.unique(a["cls"][ball])) == 2
    assert np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["cls"], c["cls"])
    clear = ball & (np.abs(a["n"].prod(-1)) > 1e-9)  # the image's middle column has n_x = 0: +0 and -0 are both >= 0
    assert clear.sum() > 5 and (d["cls"][clear] != a["cls"][clear]).all()


def test_cylinder_disc_and_side_normals():
    base = np.array([0.0, 0.0, 3.0])
    pa, pb = _scene()["pa"], _scene()["pb"]
    pa[0], pb[0] = base + [0, 0, 0.0], base + [0, 0, 0.4]  # upright, the look-at point at mid height
    sc = _scene(base=base, pa=pa, pb=pb, rad=np.array([0.1] + [0.01] * 5))
    r = VR.render(sc, FLAT, 2.0, 33, 47)
    assert r["ids"][16, 23] == VR.TOWER and np.abs(r["n"][16, 23] - [0, -1, 0]).max() < 1e-12
    top = VR.render(sc, FLAT, 2.0, 33, 47, VR.cam(elevation=-89.0, distance=1.0))
    assert top["ids"][16, 23] == VR.TOWER and np.abs(top["n"][16, 23] - [0, 0, 1]).max() < 1e-12


@functools.lru_cache(maxsize=None)
def _fields():
    return tuple((h, z) for h, z in zip(RR.bank() + [RR.perlin_field()], RR.SIZE_Z))


@functools.lru_cache(maxsize=None)
def _case(oracle, case):
    family, H, W, precision, camera = case
    Q = VR.case_poses(family, _fields(), oracle.reset_state(0.01)[0], precision)
    return VR.references(oracle, _fields(), Q, H, W, VR.CAMERAS[camera])


@pytest.mark.parametrize("case", VR.CASES, ids=lambda c: "-".join(map(str, c)))
def test_case_images_are_mostly_stable(oracle, case):
    for e, ref in enumerate(_case(oracle, case)):
        assert ref["stable"].mean() >= 0.95, (case, e, float(ref["stable"].mean()))


def test_close_ups_show_every_surface(oracle):
    cover = {sid: 0 for sid in range(2, 9)}
    for case in VR.CASES:
        if case[4] != "default":
            for ref in _case(oracle, case):
                for sid in cover:
                    cover[sid] = max(cover[sid], int((ref["ids"] == sid).sum()))
    assert min(cover.values()) >= 20, cover
