"""The base-tree contact primitives of bb_bodycon.h on the device, against the Minkowski-hull reference.

The same checks as tests/test_host_bodycon.py (its docstring has the assertions, the bound B and the
case set), through the same helper (tests/bodycon_check.py), on the gfx950 kernels of
tests/hostcheck/bodycon_check.hip: one case per lane, 64-lane workgroups, the capsule cases ordered so
that every wave holds all three routes of capsule_prism -- the face early-out, the intersecting
segment's SAT and the separated segment's distance, which on the device is the noinline, by-value
capsule_prism_apart_call under a partial exec mask, code that no host check runs.  n = 1, 63, 64, 65
and the full set; a no-hit lane and a lane past n leave their outputs at the sentinel.

And device against host build: the same hit flags everywhere, dist within B.

Measured on an MI355X (worst figures, fp64 / fp32; B = 16 eps L is 1.8e-14 / 9.5e-6 at L = 5 m; the
counts, the class A and class B figures and the case-set census are the host build's, to the digit):

                    dist                  normal             pos                vs host build, dist
  capsule_prism     8.5e-16 / 6.1e-7      1.5e-12 / 1.0e-4   2.7e-15 / 1.2e-6   1.8e-15 / 4.8e-7
  cylinder_prism    5.1e-16 / 4.2e-7 (*)  1.2e-15 / 2.5e-8   8.7e-16 / 3.5e-7   8.9e-16 / 4.8e-7
  sphere_cylinder   2.9e-16 / 1.7e-7      1.5e-13 / 6.6e-5   7.1e-15 / 3.1e-6   4.4e-16 / 1.8e-7
  sphere_capsule    2.2e-16 / 1.6e-7      5.4e-14 / 1.7e-5   2.2e-15 / 7.0e-7   4.4e-16 / 3.7e-8
  (*) outside the reference's bracket [lo, hi]; the normal is a cap contact's, pos the surface point's
  class A: 30 of 160 too deep, up to 11.3 mm; class B: 5 of 5 too deep, 1.2 to 11.6 mm, no contact
  reported on the 6 separated rim x edge poses; hit flags equal the host build's everywhere
"""
import pytest

import bodycon_check as K

torch = pytest.importorskip("torch")  # its HIP runtime is loaded before the check program's
pytestmark = pytest.mark.gpu

PRECS = ["fp64", "fp32"]


@pytest.fixture(scope="module")
def lib():
    return K.Lib()


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_capsule_prism(lib, prec, n):
    w = K.check_capsule(lib, 1, prec, n)
    if n is None:
        print(f"\ncapsule_prism, device [{prec}]: {w}")
        assert w["contacts"] >= 900 and w["dist_only"] <= K.MAX_DIST_ONLY * w["contacts"]


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", PRECS)
def test_cylinder_prism(lib, prec, n):
    w = K.check_cylinder(lib, 1, prec, n)
    if n is None:
        print(f"\ncylinder_prism, device [{prec}]: {w}")
        assert w["contacts"] >= 40 and w["pos_checked"] >= 20


@pytest.mark.parametrize("n", K.SIZES)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["sphere_cylinder", "sphere_capsule"])
def test_sphere(lib, kind, prec, n):
    w = K.check_sphere(lib, 1, prec, kind, n)
    if n is None:
        print(f"\n{kind}, device [{prec}]: {w}")
        assert w["contacts"] >= 30 and w["dist_only"] <= K.MAX_DIST_ONLY * w["contacts"]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", list(K.KIND))
def test_device_matches_host_build(lib, kind, prec):
    print(f"\n{kind} [{prec}]: device vs host build, worst dist {K.check_against(lib, prec, kind):.2e}")
