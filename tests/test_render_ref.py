"""The oracle's depth renderer (oracle/bb_oracle.c:bbo_render_depth) against the
independent numpy ray caster tests/render_ref.py, and analytic pins of that
ray caster itself.

The oracle's ray_* functions are the algorithm of csrc/bb_render.hip in double,
so a fault they share cancels in test_gpu_render.py; render_ref.py derives the
surfaces on its own (local-frame quadratics, brute force over the triangles),
and this file holds the oracle to it at the pose families and image sizes of
the kernel tests (render_ref.CASES):

  stable pixels    |oracle - reference| <= 1.2e-7: both compute in fp64, the
                   oracle's output is float32 (one ulp below 1).
  unstable pixels  the oracle lies within the reference's five samples +- 1e-6.
  caps             unstable pixels are <= 1 % of an image of >= 256 pixels, <= 2
                   of a smaller one and <= 0.2 % over all images of a family.

Measured (single run): the worst stable-pixel difference is 3.0e-8 in every
family, no unstable pixel leaves its five samples, and the unstable share is
tilt 0.06 %, lift 0.02 %, edge 0.02 %, ball 0.07 %, below 0.02 %."""
import numpy as np
import pytest

import render_ref as RR

ULP = 1.2e-7


@pytest.fixture(scope="module")
def fields():
    return [(h, z) for h, z in zip(RR.bank() + [RR.perlin_field()], RR.SIZE_Z)]


@pytest.mark.parametrize("family", RR.FAMILIES)
def test_oracle_matches_reference(oracle, fields, family):
    q0 = oracle.reset_state(0.01)[0]
    Q = RR.poses(family, fields, q0)
    total = pixels = 0
    for H, W in sorted({(h, w) for f, h, w, _ in RR.CASES if f == family}):
        unstable = []
        for e in range(RR.N_ENVS):
            hf, size_z = fields[e % len(fields)]
            for cam in (0, 1):
                ref = RR.stable_reference(oracle.render_scene(Q[e], cam), hf, size_z, H, W)
                got = oracle.render_depth(Q[e], hf, cam, H, W, size_z)
                st = ref["stable"]
                err = np.abs(got - ref["d"])
                assert (err[st] <= ULP).all(), (family, (H, W), e, cam, float(err[st].max()))
                out = np.maximum(ref["lo"] - got, got - ref["hi"])[~st]
                assert (out <= 1e-6).all(), (family, (H, W), e, cam, float(out.max()))
                unstable.append(int((~st).sum()))
        u = np.asarray(unstable)
        assert u.max() <= (0.01 * H * W if H * W >= 256 else 2), (family, (H, W), int(u.argmax()), int(u.max()))
        total += int(u.sum())
        pixels += H * W * u.size
    assert total <= 0.002 * pixels, (family, total, pixels)


# ------------------------------------------------------------------ analytic pins
FAR = np.array([0.0, 0.0, 50.0])  # behind the camera and beyond the clip


def _scene(**kw):
    """A camera at the origin looking down -z over ground far below; every primitive parked
    behind it unless given."""
    s = {"o": np.zeros(3), "R": np.eye(3), "ball": FAR.copy(), "ball_r": 0.09,
         "pa": np.tile(FAR, (6, 1)), "pb": np.tile(FAR + [0.1, 0, 0], (6, 1)), "rad": np.full(6, 0.01),
         "cyl": np.array([True, False, False, False, False, False]), "half": (5.0, 5.0)}
    s.update(kw)
    return s


def _render(scene, H=65, W=65, z_cam=10.0, **kw):
    scene = dict(scene)
    lift = np.array([0.0, 0.0, z_cam])
    for k in ("o", "ball", "pa", "pb"):
        scene[k] = scene[k] + lift
    return RR.render(scene, np.zeros(RR.HF_N * RR.HF_N, np.float32), 2.0, H, W, **kw)


def _grid(H=65, W=65):
    j, i = np.meshgrid(np.arange(W), np.arange(H))
    return (2 * (j + 0.5) / W - 1) * (W / H), 1 - 2 * (i + 0.5) / H


def _sphere_depth(xc, yc, c, r):
    """z-depth of a sphere at c (camera frame) along the pixel rays, nan where it is missed."""
    d = np.stack([xc, yc, -np.ones_like(xc)], -1)
    ln = np.linalg.norm(d, axis=-1)
    d = d / ln[..., None]
    b = d @ c
    disc = b * b - (c @ c - r * r)
    with np.errstate(invalid="ignore"):
        return (b - np.sqrt(disc)) / ln


def test_ball_on_the_optical_axis():
    D, r = 0.6, 0.09
    depth, ids = _render(_scene(ball=np.array([0.0, 0.0, -D]), ball_r=r))
    assert abs(depth[32, 32] - (D - r)) < 1e-14 and ids[32, 32] == RR.BALL
    xc, yc = _grid()
    rho = np.hypot(xc, yc)  # tan of the angle to the axis; the silhouette is the cone asin(r / D)
    edge = np.tan(np.arcsin(r / D))
    clear = np.abs(rho - edge) > 1e-9
    assert ((ids == RR.BALL) == (rho < edge))[clear].all()
    px = (ids == RR.BALL).sum()
    assert abs(px - np.pi * (edge * 32.5) ** 2) < 2 * np.pi * edge * 32.5  # the disc of that radius, in pixels
    theta = np.arctan(rho)
    t = D * np.cos(theta) - np.sqrt(np.maximum(r * r - (D * np.sin(theta)) ** 2, 0))
    assert np.abs(depth - t * np.cos(theta))[ids == RR.BALL].max() < 1e-13
    assert (depth[ids == RR.NONE] == 1.0).all() and (ids != RR.GROUND).all()


@pytest.mark.parametrize("cylinder", [True, False])
def test_segment_end_on(cylinder):
    r = 0.05
    pa, pb = _scene()["pa"], _scene()["pb"]
    pa[0], pb[0] = [0, 0, -0.5], [0, 0, -0.8]
    cyl = np.array([cylinder] + [False] * 5)
    depth, ids = _render(_scene(pa=pa, pb=pb, rad=np.array([r] + [0.01] * 5), cyl=cyl))
    xc, yc = _grid()
    rho = np.hypot(xc, yc)
    if cylinder:  # the near disc at z-depth 0.5 hides side and far disc
        edge, want = r / 0.5, np.full_like(xc, 0.5)
    else:  # the near sphere; the side lies inside its cone
        edge, want = np.tan(np.arcsin(r / 0.5)), _sphere_depth(xc, yc, np.array([0, 0, -0.5]), r)
        assert abs(depth[32, 32] - 0.45) < 1e-14
    clear = np.abs(rho - edge) > 1e-9
    assert ((ids == RR.TOWER) == (rho < edge))[clear].all() and (ids == RR.TOWER).sum() > 20
    assert np.abs(depth - want)[ids == RR.TOWER].max() < 1e-13


@pytest.mark.parametrize("cylinder", [True, False])
def test_segment_side_on(cylinder):
    r, hx, D = 0.05, 0.3, 0.5
    pa, pb = _scene()["pa"], _scene()["pb"]
    pa[0], pb[0] = [-hx, 0, -D], [hx, 0, -D]
    cyl = np.array([cylinder] + [False] * 5)
    depth, ids = _render(_scene(pa=pa, pb=pb, rad=np.array([r] + [0.01] * 5), cyl=cyl))
    xc, yc = _grid()
    # side: the circle of radius r about (y, z) = (0, -D) in the plane across the axis; the ray
    # (xc, yc, -1) s has z-depth s
    with np.errstate(invalid="ignore"):
        s = (D - np.sqrt(D * D - (1 + yc * yc) * (D * D - r * r))) / (1 + yc * yc)
    side = np.isfinite(s) & (np.abs(xc * s) <= hx)
    want = np.where(side, s, np.nan)
    if not cylinder:  # the end spheres where the side is missed (the discs of the cylinder face away)
        for sg in (-1, 1):
            c = np.array([sg * hx, 0, -D])
            ds = _sphere_depth(xc, yc, c, r)
            cap = ~side & np.isfinite(ds) & (sg * xc * ds >= hx)
            want = np.where(cap, ds, want)
    seen = np.isfinite(want)
    assert (ids[seen] == RR.TOWER).all() and (ids[~seen] == RR.NONE).all() and seen.sum() > 100
    assert np.abs(depth - want)[seen].max() < 1e-13
    assert abs(depth[32, 32] - (D - r)) < 1e-14
    # along the middle row the capsule reaches the tangent of its end sphere, the cylinder its edge
    reach = np.tan(np.arctan(hx / D) + np.arcsin(r / np.hypot(hx, D))) if not cylinder else hx / (D - r)
    row = ids[32] == RR.TOWER
    assert (row == (np.abs(xc[32]) < reach)).all()


def test_ray_tangent_to_a_cap():
    """One ray (a 1x1 image) aimed just inside and just outside the tangent cone of a capsule's end
    sphere: seen at the tangent length sqrt(|c|^2 - r^2), then missed."""
    r, c = 0.05, np.array([0.3, 0.0, -0.5])
    pa, pb = _scene()["pa"], _scene()["pb"]
    pa[0], pb[0] = [-0.3, 0, -0.5], c
    ang = np.arctan(0.3 / 0.5) + np.arcsin(r / np.linalg.norm(c))
    for delta, seen in ((-1e-7, True), (1e-7, False)):
        a = ang + delta
        R = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]])  # -z turned towards +x
        depth, ids = _render(_scene(pa=pa, pb=pb, rad=np.array([r] + [0.01] * 5), R=R, cyl=np.zeros(6, bool)), H=1, W=1)
        assert (ids[0, 0] == RR.TOWER) == seen, (delta, ids)
        if seen:  # within sqrt(2 r |c| delta) of the tangent point
            assert abs(depth[0, 0] - np.sqrt(c @ c - r * r)) < 2 * np.sqrt(2 * r * np.linalg.norm(c) * 1e-7)
        else:
            assert depth[0, 0] == 1.0


def test_inside_and_clipped_primitives_are_not_seen():
    pa, pb = _scene()["pa"], _scene()["pb"]
    pa[1], pb[1] = [0, 0, 0], [-0.2, 0, 0]  # the camera on the end of its own stick
    depth, ids = _render(_scene(pa=pa, pb=pb, ball=np.array([0.02, -0.03, 0.04])))  # and inside the ball
    assert (ids == RR.NONE).all() and (depth == 1.0).all()
    # a stick whose front face is nearer than the clip is not seen at all, back face included
    pa[1], pb[1] = [-0.1, 0, -0.0105], [0.1, 0, -0.0105]
    depth, ids = _render(_scene(pa=pa, pb=pb))
    assert (ids == RR.NONE).all() and (depth == 1.0).all()
    pa[1], pb[1] = [-0.1, 0, -0.012], [0.1, 0, -0.012]
    depth, ids = _render(_scene(pa=pa, pb=pb))
    assert ids[32, 32] == RR.STICK0 and abs(depth[32, 32] - 0.002) < 1e-15


def test_heightfield_plane_and_fold():
    """Flat ground under a tilted camera is the analytic plane; a ridge fold is seen from both
    sides (two-sided triangles) and no ray slips between two triangles."""
    a = 0.7
    R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])  # looking down by pi/2 - a
    sc = _scene(R=R)
    depth, ids = _render(sc, H=33, W=47, z_cam=0.4)
    xc, yc = _grid(33, 47)
    dz = (np.stack([xc, yc, -np.ones_like(xc)], -1) @ R.T)[..., 2]
    with np.errstate(divide="ignore"):
        want = np.where(dz < 0, np.minimum(-0.4 / dz, 1.0), 1.0)
    assert np.abs(depth - want).max() < 1e-14 and ((ids == RR.GROUND) == (want < 1.0)).all()
    hf = np.zeros((RR.HF_N, RR.HF_N), np.float32)
    hf[:, 150] = 0.2  # a ridge along y, 0.4 m high at size_z 2, next to the camera column
    x_ridge = -5.0 + 150 * 10.0 / (RR.HF_N - 1)
    # beside the ridge looking down on it, and inside it looking up at the underside of its faces
    for o, R, far in (([x_ridge + 0.1, 0.0, 0.6], np.eye(3), 0.6), ([x_ridge, 0.0, 0.1], np.diag([1.0, -1.0, -1.0]), 0.3)):
        depth, ids = RR.render(_scene(o=np.array(o), R=R), hf.ravel(), 2.0, 33, 47)
        assert (ids == RR.GROUND).all() and depth.max() <= far + 1e-7 and depth.min() > 0.0  # 0.2 is a float32
        assert depth.min() < far - 0.05  # the ridge's faces, not only the plane
