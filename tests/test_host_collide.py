"""The ball x heightfield contact list against a reference written from the geometry alone (CPU only).

tests/collide_ref.py takes each heightfield prism as five half-spaces: Euclidean projection when the
sphere's centre is outside, minimum face depth when it is inside.  The oracle's sphere_prism
(oracle/bb_oracle.c) and the product's (bb_physics.h) are one closed form from one hand (closest
point over the prism's 8 boundary triangles), so comparing them with each other pins neither; this
pins both, per slot: count, order, the cap of 50 and its overflow flag, dist, and the normal where
the reference calls it well-posed (collide_ref.BOUNDS; where the centre lies on a prism face the
normal is ill-defined and only dist and the count are held).

The case set (collide_ref.ball_cases: five fields x 6 lateral placements x 11 heights x 2) is shared
with tests/test_gpu_collide.py, which holds the device form (t16::collide_team) to the same lists.

Measured here (660 cases; bounds in parentheses):

  against the reference          contacts  count mismatches  worst dist         worst normal      dist only  dropped
  oracle bbo_forward, fp64       17,494    0                 1.6e-15 (1.8e-14)  1.7e-8 (1.8e-8)   128        0
  host collide_ground<double>    17,494    0                 1.6e-15 (1.8e-14)  1.7e-8 (1.8e-8)   128        0
  host collide_ground<float>     17,377    0                 4.1e-6  (9.7e-6)   3.9e-3 (9.7e-3)   285        5

The fp64 normal sits close to its bound on one geometry (twice in the set): the centre 6e-6 m outside
a prism's vertical face and 2 m above its bottom.  The closed form's closest point on that face's
triangle is good to about 1e-13 along the face, and the normal divides by the 6e-6; everywhere else
the worst normal is 7.8e-10.  The bound is 16 eps 5.1 over the margin floor of 1e-6 and stays.
"""
import numpy as np
import pytest

import collide_ref as R
import hostcheck_lib as H


@pytest.fixture(scope="module")
def cases():
    return R.ball_cases()


def test_case_set_census(cases):
    """The set reaches every regime of the pass: no contact, one round of the device's loop, several
    rounds, the cap, and centres outside the field whose bounding box still overlaps it."""
    cen = R.census(cases)
    print(f"\ncase set: {sum(len(t['ref']) for t in cases)} cases, {cen}")
    for k in ("0", "1-12", "13-49", "capped", "outside with contacts"):
        assert cen[k] >= 8, (k, cen)


def test_reference_single_prism():
    """sphere_prism_ref on hand-checked cases: a flat prism of the grid's size, bottom at -0.1."""
    s, r = 0.03, 0.09
    V = np.array([[0.0, 0.0, 0.0], [0.0, s, 0.0], [s, 0.0, 0.0]])
    d, n, m = R.sphere_prism_ref([0.01, 0.01, 0.05], V, -0.1, r)  # above the top face
    assert abs(d - (0.05 - r)) < 1e-16 and np.allclose(n, [0, 0, 1], atol=1e-15) and abs(m - 0.05) < 1e-16
    d, n, m = R.sphere_prism_ref([0.005, 0.005, -0.02], V, -0.1, r)  # inside: x = 0 and y = 0 faces tie at 0.005
    assert abs(d - (-0.005 - r)) < 1e-16 and m < 1e-16
    d, n, m = R.sphere_prism_ref([0.004, 0.01, -0.02], V, -0.1, r)  # inside, the x = 0 face is nearest
    assert abs(d - (-0.004 - r)) < 1e-16 and np.allclose(n, [-1, 0, 0], atol=1e-15) and abs(m - 0.004) < 1e-16
    d, n, m = R.sphere_prism_ref([-0.03, -0.04, 0.0], V, -0.1, r)  # beside the vertical edge through the origin
    assert abs(d - (0.05 - r)) < 1e-16 and np.allclose(n, [-0.6, -0.8, 0], atol=1e-15)
    d, n, m = R.sphere_prism_ref([-0.03, 0.01, 0.04], V, -0.1, r)  # off the top edge x = 0
    assert abs(d - (0.05 - r)) < 1e-16 and np.allclose(n, [-0.6, 0, 0.8], atol=1e-15)
    assert R.sphere_prism_ref([-0.06, -0.08, 0.0], V, -0.1, r) is None  # 0.1 from the edge
    d, n, m = R.sphere_prism_ref([0.01, 0.01, -0.15], V, -0.1, r)  # below the bottom face
    assert abs(d - (0.05 - r)) < 1e-16 and np.allclose(n, [0, 0, -1], atol=1e-15)


def test_oracle_contact_list_matches_reference(oracle, cases):
    """bbo_forward's ground contacts (con_dist, con_frame[0:3]) per slot, fp64."""
    tally = R.Tally("fp64")
    for t in cases:
        for i, ref in enumerate(t["ref"]):
            fo = oracle.forward(t["q"][i], np.zeros(15), np.zeros(3), np.zeros(15), t["hf"], t["size_z"])
            ground = [k for k in range(fo.ncon) if fo.con_body1[k] == 0 and fo.con_body2[k] == 7]
            assert len(ground) == fo.nground == fo.ncon, (t["name"], i)  # the ball is alone
            g = np.array([[*fo.con_frame[9 * k:9 * k + 3], fo.con_dist[k]] for k in ground]).reshape(-1, 4)
            tally.check(ref, g, fo.ground_overflow & 1, f"{t['name']} case {i} ({t['kind'][i]})")
    tally.finish("oracle vs reference")
    assert tally.dropped == 0  # nothing in the set is within 1e-9 of touching


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_host_build_contact_list_matches_reference(cases, prec):
    """kinematics + collide_ground<T> of the host build per slot."""
    tally = R.Tally(prec)
    for t in cases:
        for i, ref in enumerate(t["ref"]):
            g, ov, c = H.collide_ground(t["q"][i], t["hf"], t["size_z"], fp64=prec == "fp64")
            assert np.abs(c - t["c"][i]).max() <= (0.0 if prec == "fp64" else 5.1 * 1.2e-7), (t["name"], i)
            tally.check(ref, g, ov, f"{t['name']} case {i} ({t['kind'][i]})")
    tally.finish("host build vs reference")


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("bad", [float("nan"), 1e11, -1e11])
def test_host_build_diverged_ball_position(cases, prec, bad):
    """A NaN or far-off ball position (a diverged stage state) gives no contact and forms no cell
    index: an index from it would read far outside the field."""
    t = cases[1]
    for axis in (10, 11, 12):
        q = t["q"][40].copy()
        q[axis] = bad
        g, ov, _ = H.collide_ground(q, t["hf"], t["size_z"], fp64=prec == "fp64")
        assert len(g) == 0 and ov == 0
