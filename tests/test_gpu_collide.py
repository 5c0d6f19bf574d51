"""The step kernels' collision passes on the device, held to contact-list references.

tests/hostcheck/collide_check.hip runs bb_team16.h's passes the way the kernels do (one 16-lane team
per state, four teams per 64-lane workgroup) and copies out everything they produce.  The host
build (tests/hostcheck) runs the serial collide_ground instead, so no host check reaches this code,
and the rest of the suite sees it only through contact counts and qacc after a full Newton solve.

A  t16::collide_team against tests/collide_ref.py (the prism as five half-spaces, written from the
   geometry alone) on the 660 cases of collide_ref.ball_cases, per slot and in order: count, the cap
   of 50, the overflow flag, dist, and the normal where the reference calls it well-posed; and
   against the host build's list on the same inputs.  Bounds: collide_ref.BOUNDS, from the formats.
B  four very different trip counts in one wave (0 prisms, no hit, one round, many rounds), all live
   and with rows 0b0101: each team's list is bit for bit the one it gives when its state fills all
   four teams, and exited teams write nothing.
C  t16::collide_body_team against the oracle, fp64.  The oracle shares the capsule / cylinder x prism
   forms, so this pins what the team pass adds: the two-pass compaction, the order, the per-pair cap
   of 50 and the LDS / spill split -- not the formulas.  The formulas have their own independent
   reference: tests/test_gpu_bodycon.py (device) and tests/test_host_bodycon.py (host build) hold
   the four primitives of bb_bodycon.h to a Minkowski-hull construction (tests/bodycon_ref.py).
D  t16::body_candidates is one-sided: "no" only where the oracle has no base-tree contact.  A false
   "no" would silently drop base-tree contacts in the fast kernel.

Measured on an MI355X (bounds in parentheses; the host build's figures are in test_host_collide.py):

  A, device vs reference   contacts  count mismatches  worst dist         worst normal      dist only  dropped
  fp64                     17,494    0                 1.6e-15 (1.8e-14)  7.9e-9 (1.8e-8)   128        0
  fp32                     17,377    0                 4.1e-6  (9.7e-6)   3.0e-3 (9.7e-3)   285        5 of 660
  A, device vs host build  same counts and flags everywhere; worst dist 1.4e-15 / 2.4e-6, worst normal
                           9.3e-9 / 9.2e-4 (fp64 / fp32)
  census of the 660 cases  0: 70, 1-12: 159, 13-49: 232, capped: 199 (overflow 195), centre outside
                           the field with contacts: 68
  C  384 states (flat, hills, two flanks of the hills), 323 with contacts, 170 past the 32 LDS slots,
     12,049 contacts, no count, pair or overflow mismatch; worst dist 1.8e-15, pos 6.5e-13,
     normal 1.3e-10
  D  4,703 states: 822 "no", none of them with an oracle contact; 617 "yes" with no contact (its cost)

The fp64 normal's worst figure comes from the closed form, not from the device: the host build and
the oracle reach 1.7e-8 on the same contact.  A centre 6e-6 m outside a prism's vertical face, 2 m
above its bottom: the closest point on that face's triangle is good to about 1e-13 along the face,
and the normal divides by the 6e-6.

C found one thing when it was first run: dist differed from the oracle's by up to 2.3e-9 where the
tower's end cap is the contact feature.  cylinder_prism tested the cylinder's own axis with a radial
term sqrt(1 - (a.a)^2), a rounding residue (up to 2e-8, times r) that a fused multiply-add rounds
differently.  The term is exactly 0 and is now taken as such, in the product and in the oracle.

Each of three deliberate breaks of a scratch copy fails on its first affected case: the reject's
`<= r * r` made `< 0.9 * r * r` (A: flat case 0, 0 contacts for 6), the ballot's slot with `<= tl`
(A: flat case 0, slot 0), body_candidates without the last wheel (D: a "no" with 2 contacts).
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import collide_ref as R
import hostcheck_lib as H

torch = pytest.importorskip("torch")  # its HIP runtime is loaded before the check program's
pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "hostcheck" / "collide_check.hip"
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
NQ = 17
FULL, MIXED = 0b1111, 0b0101
SENTINEL = -12345.0  # what a team that did not run, and a slot that was not filled, must leave in place
BF_N, BF_P, BF_DIST, BF_CODE = 0, 3, 6, 7  # bb_physics.h


class Lib:
    def __init__(self):
        out = ROOT / "tests" / "_build" / "libcollide_check.so"
        out.parent.mkdir(parents=True, exist_ok=True)
        srcs = [SRC] + sorted(CSRC.glob("*.h"))
        if not (out.exists() and all(out.stat().st_mtime >= s.stat().st_mtime for s in srcs)):
            subprocess.run(["hipcc", "-O2", "-fPIC", "-shared", "--offload-arch=gfx950", "-std=c++17", "-w",
                            f"-I{CSRC}", "-o", str(out), str(SRC)], check=True)
        self.L = C.CDLL(str(out))
        sizes = (C.c_int * 5)()
        self.L.cc_sizes(sizes)
        self.MAXG, self.NGF, self.MAXB, self.MAXB_LDS, self.NBF = sizes
        assert (self.MAXG, self.NGF, self.NBF) == (R.MAXG, 4, 8)

    @staticmethod
    def _p(a):
        t = {np.dtype(np.float64): C.c_double, np.dtype(np.float32): C.c_float, np.dtype(np.int32): C.c_int}[a.dtype]
        return a.ctypes.data_as(C.POINTER(t))

    def ground(self, q, hf, size_z, prec, rows=FULL):
        """-> ng[n], overflow[n], g[n, MAXG, NGF] of collide_team, one team per row of q."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, NQ)
        n, dt = len(q), np.float64 if prec == "fp64" else np.float32
        hf = np.ascontiguousarray(hf, np.float32)
        ng, ov = np.full(n, int(SENTINEL), np.int32), np.full(n, int(SENTINEL), np.int32)
        g = np.full((n, self.MAXG, self.NGF), SENTINEL, dt)
        fn = self.L.cc_ground_f64 if prec == "fp64" else self.L.cc_ground_f32
        rc = fn(self._p(q), n, self._p(hf), C.c_double(size_z), rows, self._p(ng), self._p(ov), self._p(g))
        assert rc == 0, "the check program's launch failed"
        return ng, ov, g

    def body(self, q, hf, size_z, prec="fp64", rows=FULL):
        """-> candidates[n], nb[n], overflow[n], bc[n, MAXB, NBF] (LDS slots, then the spill block)."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, NQ)
        n, dt = len(q), np.float64 if prec == "fp64" else np.float32
        hf = np.ascontiguousarray(hf, np.float32)
        hz = float(hf.max()) * size_z
        cand, nb, ov = (np.full(n, int(SENTINEL), np.int32) for _ in range(3))
        bc = np.full((n, self.MAXB_LDS, self.NBF), SENTINEL, dt)
        spill = np.full((n, self.MAXB - self.MAXB_LDS, self.NBF), SENTINEL, dt)
        fn = self.L.cc_body_f64 if prec == "fp64" else self.L.cc_body_f32
        rc = fn(self._p(q), n, self._p(hf), C.c_double(size_z), C.c_double(hz), rows, self._p(cand), self._p(nb),
                self._p(ov), self._p(bc), self._p(spill))
        assert rc == 0, "the check program's launch failed"
        return cand, nb, ov, np.concatenate([bc, spill], axis=1)


@pytest.fixture(scope="module")
def lib():
    return Lib()


@pytest.fixture(scope="module")
def cases():
    return R.ball_cases()


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_ball_terrain_list_matches_reference(lib, cases, prec):
    """A: collide_team per slot against the half-space reference, and against the host build."""
    cen = R.census(cases)
    print(f"\ncase set: {sum(len(t['ref']) for t in cases)} cases, {cen}")
    for k in ("0", "1-12", "13-49", "capped", "outside with contacts"):
        assert cen[k] >= 8, (k, cen)
    b = R.BOUNDS[prec]
    tally = R.Tally(prec)
    host_dist = host_normal = 0.0
    for t in cases:
        ng, ov, g = lib.ground(t["q"], t["hf"], t["size_z"], prec)
        assert np.all(g[np.arange(lib.MAXG)[None, :] >= ng[:, None]] == SENTINEL), "a slot past ng was written"
        for i, ref in enumerate(t["ref"]):
            what = f"{t['name']} case {i} ({t['kind'][i]}, centre {t['c'][i]})"
            gi = g[i, :ng[i]].astype(np.float64)
            tally.check(ref, gi, ov[i], what)
            if np.any(ref["gaps"] < b["flip"]):
                continue
            hg, hov, _ = H.collide_ground(t["q"][i], t["hf"], t["size_z"], fp64=prec == "fp64")
            assert (len(gi), ov[i]) == (len(hg), hov), f"{what}: device {len(gi)}/{ov[i]}, host build {len(hg)}/{hov}"
            if len(gi):
                ed = np.abs(gi[:, 3] - hg[:, 3])
                assert ed.max() <= b["dist"], f"{what}: dist differs from the host build's by {ed.max():.2e}"
                host_dist = max(host_dist, ed.max())
                well = ref["margin"][:len(gi)] >= b["floor"]
                if well.any():
                    en = np.abs(gi[well, :3] - hg[well, :3]).max()
                    assert en <= b["normal"], f"{what}: normal differs from the host build's by {en:.2e}"
                    host_normal = max(host_normal, en)
    print(f"device vs host build [{prec}]: worst dist {host_dist:.2e}, worst normal {host_normal:.2e}")
    tally.finish("device collide_team vs reference")


# ------------------------------------------------------------------ B
def _mixed_states(cases):
    """Four states on the hills field with very different trip counts through collide_team's round loop."""
    t = cases[1]
    n = np.array([len(r["dist"]) for r in t["ref"]])
    inside = np.abs(t["c"][:, :2]).max(axis=1) < 4.5
    inside &= np.array([r["flip"] for r in t["ref"]]) > 1e-4  # no decision near rounding in either precision
    shallow = int(np.nonzero((n >= 1) & (n <= 12) & inside)[0][0])   # one round of 16 prisms or a few
    deep = int(np.nonzero((n > R.MAXG) & inside)[0][0])              # more hits than the cap, many rounds
    high = t["c"][deep] + np.array([0.0, 0.0, 0.3])                  # bounding box over the field, no hit
    away = np.array([5.2, 0.3, 0.5])                                 # bounding box off the field: no prism
    q = {"away": R.ball_qpos(away), "high": R.ball_qpos(high), "shallow": t["q"][shallow], "deep": t["q"][deep]}
    expect = {"away": 0, "high": 0, "shallow": min(n[shallow], R.MAXG), "deep": R.MAXG}
    return t, q, expect


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_ball_terrain_mixed_teams(lib, cases, prec):
    """B: the ballot runs while other teams of the wave have left the loop, or never entered it."""
    t, q, expect = _mixed_states(cases)
    alone = {}
    for name, qq in q.items():  # the state in all four teams
        ng, ov, g = lib.ground(np.tile(qq, (4, 1)), t["hf"], t["size_z"], prec)
        assert np.all(ng == expect[name]), (name, ng)
        for r in range(1, 4):
            assert ov[r] == ov[0] and np.array_equal(g[r].view(np.uint8), g[0].view(np.uint8)), (name, r)
        alone[name] = (ng[0], ov[0], g[0])
    assert alone["deep"][1] == 1 and alone["shallow"][1] == 0
    for order in (["deep", "away", "shallow", "high"], ["away", "deep", "high", "shallow"]):
        for rows in (FULL, MIXED):
            ng, ov, g = lib.ground(np.array([q[k] for k in order]), t["hf"], t["size_z"], prec, rows)
            for r, name in enumerate(order):
                if (rows >> r) & 1:
                    assert (ng[r], ov[r]) == alone[name][:2], (order, rows, name, ng[r], ov[r])
                    assert np.array_equal(g[r].view(np.uint8), alone[name][2].view(np.uint8)), (order, rows, name)
                else:
                    assert ng[r] == int(SENTINEL) and ov[r] == int(SENTINEL) and np.all(g[r] == SENTINEL), (order, r)


# ------------------------------------------------------------------ C and D
@pytest.fixture(scope="module")
def body_sets(oracle):
    """Per terrain: (hf, q[n, 17], the oracle's ForwardOut per state) for the base-tree states of
    test_gpu_parity: rolled and lowered bases, and toppled robots lying on the terrain."""
    import test_gpu_parity as P
    from ballbot_gym.terrain import generate_hills_terrain

    out = {}
    for terrain in ("flat", "hills"):
        hf = oracle.flat_hfield() if terrain == "flat" else generate_hills_terrain(293, seed=7).astype(np.float32)
        q1, _ = P._body_contact_states(oracle, 64, 11)
        q2, _ = P._toppled_states(oracle, 32, terrain, np.random.default_rng(21))
        q = np.concatenate([q1, q2])
        out[terrain] = (hf, q, [_oracle(oracle, qq, hf) for qq in q])
    # those states lie within 0.6 m of the origin, where the hills field is flat too: the same poses
    # on two of its flanks (slopes of 0.45 and 2.1), where a prism's neighbours are higher than
    # the prism under a geom and the conservative prunes have something to decide
    H = hf.reshape(293, 293)
    for name, (ri, ci) in (("hills flank 0.45", (32, 197)), ("hills flank 2.1", (71, 201))):
        q = out["hills"][1].copy()
        x, y, z = ci * 10.0 / 292 - 5.0, ri * 10.0 / 292 - 5.0, float(H[ri, ci]) * 2.0
        q[:, [0, 10]] += x
        q[:, [1, 11]] += y
        q[:, [2, 12]] += z
        out[name] = (hf, q, [_oracle(oracle, qq, hf) for qq in q])
    return out


def _oracle(oracle, q, hf):
    return oracle.forward(q, np.zeros(15), np.zeros(3), np.zeros(15), hf, 2.0)


def test_base_tree_list_matches_oracle(lib, body_sets):
    """C: collide_body_team per slot against the oracle's base-tree contacts (fp64).  Not an independent
    reference (the primitives have theirs in test_gpu_bodycon.py): it pins the compaction, the order,
    the per-pair cap and the LDS / spill split.  dist and pos within 1e-9, the project's bound for the capsule-prism forms
    (test_host_geometry.py; DESIGN §5 measured 1.1e-11); normals within 1e-6 where |dist| >= 1e-3."""
    touched = past = total = 0
    worst = dict(dist=0.0, pos=0.0, normal=0.0)
    for terrain, (hf, q, fos) in body_sets.items():
        cand, nb, ov, bc = lib.body(q, hf, 2.0)
        for i, fo in enumerate(fos):
            what = f"{terrain} state {i}"
            assert nb[i] == fo.nbody, f"{what}: {nb[i]} contacts, oracle {fo.nbody}"
            assert (ov[i] & 2) == (fo.ground_overflow & 2), f"{what}: overflow {ov[i]}, oracle {fo.ground_overflow}"
            assert np.all(bc[i, nb[i]:] == SENTINEL), f"{what}: a slot past nb was written"
            touched += fo.nbody > 0
            past += fo.nbody > lib.MAXB_LDS
            total += fo.nbody
            for s in range(fo.nbody):
                k = fo.ncon - fo.nbody + s  # the oracle lists wheel, then ground, then base-tree contacts
                code = int(bc[i, s, BF_CODE])
                assert (code // 8, code % 8) == (fo.con_body1[k], fo.con_body2[k]), f"{what} slot {s}: pair {code}"
                ed = abs(bc[i, s, BF_DIST] - fo.con_dist[k])
                ep = np.abs(bc[i, s, BF_P:BF_P + 3] - np.array(fo.con_pos[3 * k:3 * k + 3])).max()
                worst["dist"], worst["pos"] = max(worst["dist"], ed), max(worst["pos"], ep)
                assert ed <= 1e-9 and ep <= 1e-9, f"{what} slot {s}: dist off by {ed:.2e}, pos by {ep:.2e}"
                if abs(fo.con_dist[k]) >= 1e-3:
                    en = np.abs(bc[i, s, BF_N:BF_N + 3] - np.array(fo.con_frame[9 * k:9 * k + 3])).max()
                    worst["normal"] = max(worst["normal"], en)
                    assert en <= 1e-6, f"{what} slot {s}: normal off by {en:.2e}"
    n = sum(len(v[1]) for v in body_sets.values())
    print(f"\nbase-tree lists: {n} states, {touched} with contacts, {past} past the LDS slots, {total} contacts, "
          f"worst {worst}")
    assert touched >= n // 4 and past >= 4


def test_body_candidates_is_one_sided(lib, oracle, body_sets):
    """D: body_candidates == false only where the oracle has no base-tree contact, on C's states, the
    same states with the base raised in 5 mm steps until the oracle's count reaches 0 (the edge where
    a conservative test can go wrong) and two steps beyond, and upright robots.  On the flanks the
    robots lie deep in the slope, so the base first rises in 50 mm steps while it still touches."""
    yes_empty = states = noes = 0
    for terrain, (hf, q0, fos) in body_sets.items():
        qs, nbody = [], []
        flank = "flank" in terrain
        for q, fo in zip(q0, fos):
            qs.append(q)
            nbody.append(fo.nbody)

            def raised(mm):
                qq = q.copy()
                qq[2] = q[2] + 0.001 * mm
                qs.append(qq)
                nbody.append(_oracle(oracle, qq, hf).nbody)
                return nbody[-1]

            mm, left = 0, fo.nbody
            if flank and left > 0:  # parts lie deep in the flank: 50 mm steps up to the last one that touches
                while mm < 3000 and raised(mm + 50) > 0:
                    mm += 50
            while left > 0 and mm < 3000:  # 5 mm steps until the oracle's count reaches 0
                mm += 5
                left = raised(mm)
            assert left == 0, (terrain, mm)
            raised(mm + 5)  # and two states just clear of the terrain
            raised(mm + 15)
        rng = np.random.default_rng(31)
        for _ in range(32):  # upright over the ball (the reset pose), tilted by up to 8 degrees
            q, _, _ = oracle.reset_state(0.01)
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            a = np.radians(rng.uniform(0, 8))
            q[3:7] = [np.cos(a / 2), *(np.sin(a / 2) * ax)]
            qs.append(q)
            nbody.append(_oracle(oracle, q, hf).nbody)
        qs, nbody = np.array(qs), np.array(nbody)
        cand, _, _, _ = lib.body(qs, hf, 2.0)
        assert set(np.unique(cand)) <= {0, 1}
        for i in np.nonzero((cand == 0) & (nbody > 0))[0]:
            raise AssertionError(f"{terrain} state {i}: body_candidates says no, the oracle has {nbody[i]} contacts")
        states += len(qs)
        noes += int((cand == 0).sum())
        yes_empty += int(((cand == 1) & (nbody == 0)).sum())
    assert noes > 0  # the answer is not a constant
    print(f"\nbody_candidates: {states} states, {noes} no, {yes_empty} yes with no contact (its cost)")
