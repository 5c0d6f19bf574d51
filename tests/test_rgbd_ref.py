"""The onboard RGB-D image's fp64 reference (tests/rgbd_ref.py): an analytic pin of the reference
itself, its D plane against render_ref.render, and the conditions the GPU test (test_gpu_rgbd.py)
rests on, asserted here on the same images so that the GPU test cannot hide behind them:

  * the D plane equals render_ref.render's depth to 1e-12 in every image;
  * stable share per image >= 0.95 at every size from 17x23 up, >= 13 of 15 pixels at 5x3;
  * over the 12x60 case the ground, the ball, both sticks and the three wheels cover >= 500 pixels
    each, and both ball tones and both checker parities appear;
  * the lift family has >= 25 % of its pixels on a surface beyond 1 m, so the far colour path runs.

Measured (single run): the smallest stable share of an image is 0.982 at 17x23 and 24x40 (ball
17x23; lift 24x40 0.983), 0.990 at 12x60, 0.996 at 64x64, and 14 of 15 pixels at 5x3.  Coverage
over 12x60: ground 26701, ball 6074, sticks 832 / 780, wheels 1756 / 3446 / 734 pixels; ball tones
3186 / 2888, checker parities 12878 / 13823.  Lift: 0.320 of the pixels lie on a surface beyond 1 m.

The tower (id 3) is in view in none of the four families counted (tilt 12x60, and tilt, lift and
ball at 24x40, 32 envs each: 0 pixels in each): the cameras sit on its sticks and look away from
it.  So nothing here or on the GPU asserts the tower's colour from these cameras; bb_view.hip's
close-ups hold the same code path (tests/test_gpu_view.py)."""
import numpy as np
import pytest

import render_ref as RR
import rgbd_ref as GR
import view_ref as VR


def _refs(oracle, case):
    family, H, W, n, _ = case
    return GR.case_references(oracle, family, H, W, n)  # fp64 poses throughout on the CPU


@pytest.mark.parametrize("case", GR.CASES, ids=lambda c: "-".join(map(str, c[:4])))
def test_case_images(oracle, case):
    family, H, W, n, _ = case
    Q = GR.case_poses(oracle, family, n)
    F = GR.fields()
    worst = 1.0
    for (e, cam), ref in _refs(oracle, case).items():
        hf, size_z = F[e % len(F)]
        depth, _ = RR.render(oracle.render_scene(Q[e], cam), hf, size_z, H, W)
        assert np.abs(ref["D"] - depth).max() <= 1e-12, (case, e, cam)
        assert (ref["ids"] != 0)[ref["D"] < 1].all()
        share = float(ref["stable"].mean())
        worst = min(worst, share)
        if H * W >= 17 * 23:
            assert share >= 0.95, (case, e, cam, share)
        elif (H, W) == (5, 3):
            assert int(ref["stable"].sum()) >= 13, (case, e, cam, int(ref["stable"].sum()))
    print(f"RGBD-REF {'-'.join(map(str, case[:4])):20s} smallest stable share {worst:.3f}")


def test_coverage_of_the_wide_case(oracle):
    refs = _refs(oracle, ("tilt", 12, 60, 32, "fp64"))
    ids = np.stack([r["ids"] for r in refs.values()])
    cls = np.stack([r["cls"] for r in refs.values()])
    cover = {sid: int((ids == sid).sum()) for sid in range(9)}
    for sid in (1, 2, 4, 5, 6, 7, 8):
        assert cover[sid] >= 500, cover
    tones = [int(((ids == VR.BALL) & (cls == k)).sum()) for k in (0, 1)]
    parity = [int(((ids == VR.GROUND) & (cls == k)).sum()) for k in (0, 1)]
    assert min(tones) > 0 and min(parity) > 0, (tones, parity)
    print(f"RGBD-REF coverage {cover} ball tones {tones} checker parities {parity}")


def test_lift_reaches_beyond_one_metre(oracle):
    refs = _refs(oracle, ("lift", 24, 40, 16, "fp64"))
    far = np.stack([(r["ids"] != 0) & (r["depth"] > 1.0) for r in refs.values()])
    assert far.mean() >= 0.25, float(far.mean())
    print(f"RGBD-REF lift: {far.mean():.3f} of the pixels on a surface beyond 1 m")


@pytest.mark.parametrize("family,H,W", [("tilt", 12, 60), ("tilt", 24, 40), ("lift", 24, 40), ("ball", 24, 40)])
def test_tower_is_never_in_view(oracle, family, H, W):
    """One sample per image is enough to count a surface."""
    Q = GR.case_poses(oracle, family, 32)
    F = GR.fields()
    seen = 0
    for e in range(32):
        hf, size_z = F[e % len(F)]
        for cam in (0, 1):
            r = GR.render(oracle.render_scene(Q[e], cam), VR.quat_matrix(Q[e][13:17]), hf, size_z, H, W)
            seen += int((r["ids"] == VR.TOWER).sum())
    assert seen == 0, seen


def test_upright_robot_on_flat_ground(oracle):
    """Analytic pin: the ground's normal is +z, so every ground pixel's colour is the checker base
    times 0.25 + 0.45 + 0.30 (-d_z), and the stored value is float32(int(255 c + 0.5)) / 255."""
    q = oracle.reset_state(0.01)[0]
    hf, size_z = GR.fields()[0]
    assert not np.asarray(hf).any()
    for cam in (0, 1):
        r = GR.render(oracle.render_scene(q, cam), VR.quat_matrix(q[13:17]), hf, size_z, 24, 40)
        g = r["ids"] == VR.GROUND
        assert g.sum() > 100
        o = oracle.render_scene(q, cam)["o"]
        d = r["d"][g]
        t = -o[2] / d[:, 2]  # the plane z = 0
        p = o[None, :] + t[:, None] * d
        odd = (np.floor(p[:, 0] / 0.5) + np.floor(p[:, 1] / 0.5)).astype(int) & 1
        base = np.where(odd[:, None] == 1, VR.GROUND_ODD, VR.GROUND_EVEN)
        want = base * (0.25 + 0.45 + 0.30 * (-d[:, 2]))[:, None]
        assert np.abs(r["c"][g] - want).max() < 1e-12
        assert (r["q"][g] == np.floor(255 * want + 0.5)).all()
        f = GR.to_float(r["q"])
        assert f.dtype == np.float32 and f.min() >= 0 and f.max() <= 1
        assert (r["q"][r["ids"] == 0] == [140, 179, 230]).all()
