"""The base-tree contact primitives of bb_bodycon.h against a Minkowski-hull reference (CPU only).

capsule_prism, cylinder_prism, sphere_cylinder and sphere_capsule were compared with the oracle
alone, which runs the same algorithm: a missing axis, a wrong sign or a wrong case split shared by
both passed.  tests/bodycon_ref.py builds the answer from the geometry (the hull of the vertex
differences; a cylinder bracketed between inscribed and circumscribed 256-gons), and
tests/bodycon_check.py holds the templates to it: here their host build, in
tests/test_gpu_bodycon.py the gfx950 kernels of tests/hostcheck/bodycon_check.hip, at n = 1, 63, 64,
65 and the full set, fp64 and fp32 (the fp32 reference gets the float-rounded inputs as doubles).

The bound is B = 16 eps(T) L, L the case's largest coordinate magnitude (bodycon_ref.C_BOUND: 11
roundings at magnitude L, taken as 16): at L = 5 m, 1.8e-14 (fp64) and 9.5e-6 (fp32).

  hit / no-hit    the reference's wherever |dist_ref| > B; a no-hit leaves all seven outputs alone
  capsule         |dist - dist_ref| <= B, the normal within B / gap where gap > 100 B, pos by the
                  header's convention and against the reference's deepest point where it is unique.
                  Class A (the lower end within 2 cm of the prism's bottom, intersecting): one-sided,
                  depth >= depth_ref - B -- the kernel's axis set has no dir x bottom-edge axis
  cylinder        lo - B <= depth <= hi + B and "apart" wherever the outer polygon is apart.  Class B
                  (rim_edge: 1e-3 < |n*.a| < 1 - 1e-3 with a prism edge or face in the feature):
                  depth >= lo - B only -- the axis set has no rim x edge axis
  spheres         dist within B (+ the polish's convergence figure outside the cylinder), normal, pos
  the case set    <= 10 % of a primitive's contacts dist-only, <= 15 % of the cylinder contacts
                  rim_edge, class A exactly the 200 cases built for it, every wave all three routes
  the reference   the hull's depth against a SAT over all 5 face normals and all 9 edge directions
                  on the 682 intersecting capsule cases: worst 2.3e-17

Measured, host build (worst figures; bounds at L = 5 in parentheses):

  capsule, 1498 cases (routes 305 / 682 / 511), 985 contacts
              dist              normal    pos       dist only  class A in excess
    fp64      1.2e-15 (1.8e-14) 1.5e-12   2.7e-15   10         30 of 160, up to 11.3 mm
    fp32      6.8e-7  (9.5e-6)  1.5e-4    2.1e-6    66         30 of 160, up to 11.3 mm
  cylinder, 80 poses, 49 contacts (5 rim_edge), 31 apart (6 rim_edge)
              below lo  above hi  class B in excess              separated shapes in contact
    fp64      4.3e-16   5.1e-16   5 of 5: 1.2, 1.3, 1.7, 8.2, 11.6 mm  0 of 6
    fp32      4.2e-7    3.9e-7    the same                       0 of 6
  sphere_cylinder, 140 cases, 112 contacts: dist 4.2e-16 / 1.8e-7, normal 1.5e-13 / 6.6e-5,
    pos 7.1e-15 / 3.1e-6 (fp64 / fp32); dist only 6 / 9; the polish's figure at most 1.0e-12 / 3.2e-9
  sphere_capsule, 60 cases, 40 contacts: dist 2.4e-16 / 1.6e-7, normal 5.4e-14 / 1.7e-5,
    pos 2.2e-15 / 7.0e-7; dist only 4 / 4

What the first runs found, outside classes A and B, and fixed in bb_bodycon.h (and the oracle):
  - cylinder_prism, fp32: pos of every cap contact lay r = 0.11 m along the axis off the cap, and pos
    of a wall contact at the cylinder's end instead of beside the prism.  The thresholds that tell
    "n is along / across the axis" were 1e-9, below fp32's rounding residue of n.a.
  - sphere_cylinder: a centre exactly on the axis and nearer the wall than a cap gave n = (0, 0, 0).
  With the header as it was, the set fails on cylinder case 2 [fp32] (a wall contact, pos's surface
  point 0.198 m off) and on sphere_cylinder case 24 [fp64] (|n| = 0).
A rim x edge contact whose normal is within 1e-3 of the axis or of the wall's plane is neither in
class B by that definition nor exact (seen: 6.9e-6 and 6.6e-4 m above the bracket); the generator
draws such a pose again, by the reference alone, so the set holds classified cases only.

Deliberate breaks of a scratch copy, each failing on its first affected case (host build, both
precisions):
  - capsule_prism's `dm = -mn + max(e0, e1)` made `-mn - max(e0, e1)`: capsule case 0 (plain wheel,
    intersecting), dist 7.13 for -0.0352
  - cylinder_prism without `test(g.a, true)`: cylinder case 11 (cap), depth 53.5 mm for 49.0 mm
"""
import numpy as np
import pytest

import bodycon_check as K
import bodycon_ref as R

PRECS = ["fp64", "fp32"]


@pytest.fixture(scope="module")
def lib():
    return K.Lib()


@pytest.mark.parametrize("prec", PRECS)
def test_case_set_conditions(prec):
    print(f"\ncase set [{prec}]: {K.check_case_set(prec)}")


def test_hull_matches_full_sat():
    """The reference against a second construction, once: on every intersecting capsule case the
    hull's depth is the minimum over all 5 face normals and all 9 dir x edge axes, to rounding."""
    cs, ref = R.cases()["capsule"], R.references("fp64")["capsule"]
    worst, n = 0.0, 0
    for row, o in zip(cs["inp"], ref):
        if not o["inside"]:
            continue
        V = R.prism_vertices(row[:9].reshape(3, 3), row[9])
        c, a, hh = row[10:13], row[13:16], row[16]
        rel = V - c  # as the reference forms it: no rounding at the coordinates' magnitude
        e = abs(R.full_sat_depth(rel, -hh * a, hh * a) - o["depth"])
        assert e <= R.bound("fp64", np.abs(rel).max() + hh), (n, e)
        worst, n = max(worst, e), n + 1
    print(f"\nhull vs full SAT: {n} intersecting cases, worst {worst:.2e}")
    assert n >= 500


def test_reference_hand_cases():
    """bodycon_ref on cases checked by hand: a flat prism of 0.03 m legs, bottom at -0.1."""
    s = 0.03
    V = R.prism_vertices([[0, 0, 0], [0, s, 0], [s, 0, 0]], -0.1)
    o = R.capsule_prism(V, [0.01, 0.01, 0.05], [1.0, 0, 0], 0.02, 0.01)  # level, 0.05 above the top
    assert not o["inside"] and abs(o["dist"] - 0.04) < 1e-16 and np.allclose(o["normal"], [0, 0, 1], atol=1e-15)
    o = R.capsule_prism(V, [0.005, 0.005, 0.0], [0, 0, 1.0], 0.02, 0.01)  # upright, its lower end 0.02 deep
    assert o["inside"] and abs(o["depth"] - 0.005) < 1e-16  # out through x = 0 or y = 0, 0.005 away
    o = R.capsule_prism(V, [0.004, 0.01, 0.0], [0, 0, 1.0], 0.02, 0.01)
    assert abs(o["depth"] - 0.004) < 1e-16 and np.allclose(o["normal"], [-1, 0, 0], atol=1e-15) and abs(o["gap"] - 0.006) < 1e-15
    assert list(o["deep"]) == [0, 1]  # both ends are as deep along -x
    o = R.cylinder_prism(V, [0.01, 0.01, 0.13], [0, 0, 1.0], 0.14, 0.11)  # standing on the top, 0.01 deep
    assert abs(o["lo"] - 0.01) < 1e-15 and abs(o["hi"] - 0.01) < 1e-15 and o["feature"] == "cap" and not o["rim_edge"]
    o = R.cylinder_prism(V, [0.01, 0.01, 0.10], [1.0, 0, 0], 0.14, 0.11)  # lying on the top, 0.01 deep
    assert o["lo"] <= 0.01 + 1e-15 <= o["hi"] + 2e-15 and o["hi"] - o["lo"] < 8.4e-6
    o = R.cylinder_prism(V, [0.01, 0.01, 0.16], [0, 0, 1.0], 0.14, 0.11)
    assert o["apart_inner"] and o["apart_outer"] and abs(o["sep"] - 0.02) < 1e-15
    o = R.sphere_cylinder([0.2, 0, 0], 0.09, [0, 0, 0], [0, 0, 1.0], 0.14, 0.11)  # beside the wall
    assert abs(o["dist_lo"] - 0.0) < 1e-15 and o["tol"] < 1e-12 and np.allclose(o["normal"], [-1, 0, 0], atol=1e-12)
    o = R.sphere_cylinder([0.15, 0, 0.18], 0.09, [0, 0, 0], [0, 0, 1.0], 0.14, 0.11)  # off the rim: 0.04, 0.04
    assert abs(o["dist_lo"] - (0.04 * np.sqrt(2) - 0.09)) < 1e-12
    o = R.sphere_cylinder([0.1, 0, 0.0], 0.09, [0, 0, 0], [0, 0, 1.0], 0.14, 0.11)  # inside, 0.01 from the wall
    assert o["inside"] and o["dist_lo"] <= -0.01 - 0.09 <= o["dist_hi"] + 1e-15
    o = R.sphere_capsule([0, 0.05, 0.2], 0.09, [0, 0, 0], [0, 0, 1.0], 0.1, 0.01)  # beyond the end
    assert abs(o["dist"] - (np.hypot(0.05, 0.1) - 0.1)) < 1e-15


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_capsule_prism(lib, prec, n):
    w = K.check_capsule(lib, 0, prec, n)
    if n is None:
        print(f"\ncapsule_prism, host build [{prec}]: {w}")
        assert w["contacts"] >= 900 and w["dist_only"] <= K.MAX_DIST_ONLY * w["contacts"]


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_cylinder_prism(lib, prec, n):
    w = K.check_cylinder(lib, 0, prec, n)
    if n is None:
        print(f"\ncylinder_prism, host build [{prec}]: {w}")
        assert w["contacts"] >= 40 and w["pos_checked"] >= 20


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["sphere_cylinder", "sphere_capsule"])
def test_sphere(lib, kind, prec, n):
    w = K.check_sphere(lib, 0, prec, kind, n)
    if n is None:
        print(f"\n{kind}, host build [{prec}]: {w}")
        assert w["contacts"] >= 30 and w["dist_only"] <= K.MAX_DIST_ONLY * w["contacts"]
