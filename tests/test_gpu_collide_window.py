"""t16::collide_team with the bound on its cell window (prism_window, csrc/bb_physics.h) on the device.

tests/hostcheck/collide_window_check.hip runs the pass the way the kernels do (one 16-lane team per state,
four teams per 64-lane workgroup), once with the bound forward hands in (the field's top, T(max h) * size_z
formed in the precision under test) and once through the signature without it, and copies out everything
the pass produces.  ng, the overflow flag and every slot of g must be the same bits in fp64 and fp32, and
unfilled slots keep their sentinel.

A  the 660 cases of collide_ref.ball_cases (five fields: flat, hills, stepped, terraced, the top of the
   range), which tests/test_gpu_collide.py holds to the half-space reference without the bound
B  the adversarial cases of tests/hostcheck/prism_window_check.cpp restated for the device: flat, a
   sinusoid and hills at size_z 0.3, 1 and 2; penetrations from 1e-4 m to r, a ball 1 mm above the
   ground, a grazing ball (centre at top + r within a few ulps of either format), centres on grid lines
   and vertices within +-1 ulp, at the field's edge, outside it, and a NaN centre
C  one workgroup whose four teams have very different trip counts (no prism, airborne, one round, many
   rounds), all live and with rows 0b0101, on the hills field and on flat ground, where the bound cuts
   the shallow state to one round and leaves the deep one its many: each team's list is the list it
   gives when its state fills all four teams, and exited teams write nothing
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import collide_ref as R

torch = pytest.importorskip("torch")  # its HIP runtime is loaded before the check program's
pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "hostcheck" / "collide_window_check.hip"
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
NQ, N = 17, R.HF_N
FULL, MIXED = 0b1111, 0b0101
SENTINEL = -12345.0  # what a team that did not run, and a slot that was not filled, must leave in place
DX = 2 * R.HF_SX / (N - 1)


class Lib:
    def __init__(self):
        out = ROOT / "tests" / "_build" / "libcollide_window_check.so"
        out.parent.mkdir(parents=True, exist_ok=True)
        srcs = [SRC] + sorted(CSRC.glob("*.h"))
        if not (out.exists() and all(out.stat().st_mtime >= s.stat().st_mtime for s in srcs)):
            subprocess.run(["hipcc", "-O2", "-fPIC", "-shared", "--offload-arch=gfx950", "-std=c++17", "-w",
                            f"-I{CSRC}", "-o", str(out), str(SRC)], check=True)
        self.L = C.CDLL(str(out))
        sizes = (C.c_int * 3)()
        self.L.cw_sizes(sizes)
        self.MAXG, self.NGF, window = sizes
        assert (self.MAXG, self.NGF) == (R.MAXG, 4)
        assert window == 1, "the check program was built without the window"

    @staticmethod
    def _p(a):
        t = {np.dtype(np.float64): C.c_double, np.dtype(np.float32): C.c_float, np.dtype(np.int32): C.c_int}[a.dtype]
        return a.ctypes.data_as(C.POINTER(t))

    def ground(self, q, hf, size_z, prec, bounded, rows=FULL):
        """-> ng[n], overflow[n], g[n, MAXG, NGF] of collide_team, one team per row of q; bounded: with the
        field's top as the bound, formed as forward forms TerrainRef::hz."""
        q = np.ascontiguousarray(q, np.float64).reshape(-1, NQ)
        n, dt = len(q), np.float64 if prec == "fp64" else np.float32
        hf = np.ascontiguousarray(hf, np.float32)
        top = np.full(n, float(dt(hf.max()) * dt(size_z)), np.float64)
        ng, ov = np.full(n, int(SENTINEL), np.int32), np.full(n, int(SENTINEL), np.int32)
        g = np.full((n, self.MAXG, self.NGF), SENTINEL, dt)
        fn = self.L.cw_ground_f64 if prec == "fp64" else self.L.cw_ground_f32
        rc = fn(self._p(q), n, self._p(hf), C.c_double(size_z), self._p(top), int(bounded), rows, self._p(ng),
                self._p(ov), self._p(g))
        assert rc == 0, "the check program's launch failed"
        return ng, ov, g


@pytest.fixture(scope="module")
def lib():
    return Lib()


@pytest.fixture(scope="module")
def cases():
    return R.ball_cases()


def _same(lib, q, hf, size_z, prec, what):
    """Both forms on the states q: the same bits; -> ng, overflow of the bounded form."""
    ng, ov, g = lib.ground(q, hf, size_z, prec, True)
    ng0, ov0, g0 = lib.ground(q, hf, size_z, prec, False)
    assert np.all(g[np.arange(lib.MAXG)[None, :] >= ng[:, None]] == SENTINEL), f"{what}: a slot past ng was written"
    bad = np.nonzero((ng != ng0) | (ov != ov0))[0]
    assert len(bad) == 0, f"{what}: state {bad[0]} (qpos {q[bad[0], 10:13]}): {ng[bad[0]]}/{ov[bad[0]]} contacts/" \
                          f"overflow with the bound, {ng0[bad[0]]}/{ov0[bad[0]]} without"
    diff = np.nonzero(np.any(g.view(np.uint8).reshape(len(q), -1) != g0.view(np.uint8).reshape(len(q), -1), axis=1))[0]
    assert len(diff) == 0, f"{what}: state {diff[0]} (qpos {q[diff[0], 10:13]}): the lists differ"
    return ng, ov


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_case_set_lists_bit_equal(lib, cases, prec):
    """A: the 660 cases, the bounded pass against the pass without the bound."""
    total = capped = 0
    for t in cases:
        ng, ov = _same(lib, t["q"], t["hf"], t["size_z"], prec, t["name"])
        total += int(ng.sum())
        capped += int((ov == 1).sum())
    print(f"\n{prec}: {sum(len(t['q']) for t in cases)} cases, {total} contacts, {capped} capped")
    assert total > 10000 and capped > 100


# ------------------------------------------------------------------ B
def _fields():
    from ballbot_gym.terrain import generate_hills_terrain
    from ballbot_gym.terrain.sinusoidal import generate_sinusoidal_terrain

    return [("flat", np.zeros(N * N, np.float32)),
            ("sinusoid", np.asarray(generate_sinusoidal_terrain(N, amplitude=0.5, frequency=0.1), np.float32).ravel()),
            ("hills", np.asarray(generate_hills_terrain(N, seed=7), np.float32).ravel())]


def _adversarial(hf, size_z, seed):
    """Ball centres c[n, 3] (module docstring, B) on one field."""
    rng = np.random.default_rng(seed)
    H = hf.reshape(N, N).astype(np.float64) * size_z
    r = R.BALL_R
    top = float(H.max())

    def ground(x, y):  # the nearest vertex's height
        i = np.clip(np.rint((np.array([y, x]) + R.HF_SX) / DX).astype(int), 0, N - 1)
        return H[i[0], i[1]]

    cs = []
    for _ in range(6):
        x, y = rng.uniform(-4.8, 4.8, 2)
        z0 = ground(x, y)
        for d in (1e-4, 2e-4, 5e-4, 1e-3, 2e-3, 4e-3, 8e-3, 0.015, 0.03, 0.05, 0.07, 0.0899, 0.09):
            cs.append([x, y, z0 + r - d])
        cs.append([x, y, z0 + r + 1e-3])
        for ft in (np.float32, np.float64):  # grazing: centre at top + r within a few ulps of either format
            z = ft(top + r)
            for k in range(-3, 4):
                cs.append([x, y, float(z + ft(k) * np.spacing(z))])
        cc, rr = rng.integers(3, 289, 2)
        for ft in (np.float32, np.float64):  # on a vertex and on grid lines, within +-1 ulp
            xv, yv = ft(DX * cc - R.HF_SX), ft(DX * rr - R.HF_SX)
            for kx in (-1, 0, 1):
                for ky in (-1, 0, 1):
                    xx, yy = float(xv + ft(kx) * np.spacing(xv)), float(yv + ft(ky) * np.spacing(yv))
                    d = (2e-4, 2e-3, 0.03)[(kx + ky) % 3]
                    cs += [[xx, yy, ground(xx, yy) + r - d], [xx, y, ground(xx, y) + r - d],
                           [x, yy, ground(x, yy) + r - d]]
        for d in (2e-4, 2e-3, 0.03):  # at the field's edge, inside and outside it, and off the field
            sg, off = rng.choice([-1.0, 1.0]), rng.uniform(-0.12, 0.12)
            xe = sg * R.HF_SX + off
            cs += [[xe, y, ground(xe, y) + r - d], [x, xe, ground(x, xe) + r - d], [xe, -xe, ground(xe, -xe) + r - d],
                   [sg * R.HF_SX, y, ground(sg * R.HF_SX, y) + r - d],
                   [sg * (R.HF_SX + r), y, ground(sg * R.HF_SX, y) + r - d], [sg * (R.HF_SX + 0.2), y, z0 + r - d]]
    cs.append([np.nan, 0.3, r])
    cs.append([0.1, 0.3, np.nan])
    return np.array(cs, np.float64)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_adversarial_lists_bit_equal(lib, prec):
    """B: the host check's adversarial cases, the bounded pass against the pass without the bound."""
    states = total = empty = 0
    for fi, (name, hf) in enumerate(_fields()):
        for si, size_z in enumerate((0.3, 1.0, 2.0)):
            c = _adversarial(hf, size_z, 100 + 10 * fi + si)
            q = np.array([R.ball_qpos(ci) for ci in c])
            ng, _ = _same(lib, q, hf, size_z, prec, f"{name} size_z {size_z}")
            states += len(q)
            total += int(ng.sum())
            empty += int((ng == 0).sum())
    print(f"\n{prec}: {states} states, {total} contacts, {empty} states without a contact")
    assert total > 1000 and empty > 20  # the set holds both kinds


# ------------------------------------------------------------------ C
def _flat_mixed():
    r = R.BALL_R
    q = {"away": R.ball_qpos([5.2, 0.3, 0.5]), "high": R.ball_qpos([0.31, -1.27, r + 0.3]),
         "shallow": R.ball_qpos([0.31, -1.27, r - 0.002]), "deep": R.ball_qpos([-2.13, 0.77, r - 0.05])}
    return dict(hf=np.zeros(N * N, np.float32), size_z=2.0), q


@pytest.mark.parametrize("terrain", ["hills", "flat"])
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_mixed_teams_with_the_bound(lib, cases, prec, terrain):
    """C: the ballot runs while other teams of the wave have left the loop, or never entered it."""
    if terrain == "hills":
        import test_gpu_collide as GC

        t, q, _ = GC._mixed_states(cases)
    else:
        t, q = _flat_mixed()
    alone = {}
    for name, qq in q.items():  # the state in all four teams, and the same without the bound
        ng, ov, g = lib.ground(np.tile(qq, (4, 1)), t["hf"], t["size_z"], prec, True)
        ng0, ov0, g0 = lib.ground(np.tile(qq, (4, 1)), t["hf"], t["size_z"], prec, False)
        assert np.array_equal(ng, ng0) and np.array_equal(ov, ov0), (name, ng, ng0)
        assert np.array_equal(g.view(np.uint8), g0.view(np.uint8)), name
        alone[name] = (ng[0], ov[0], g[0])
    assert alone["away"][0] == 0 and alone["high"][0] == 0, alone
    assert 1 <= alone["shallow"][0] <= 16 and alone["deep"][0] == R.MAXG and alone["deep"][1] == 1, alone
    for order in (["deep", "away", "shallow", "high"], ["away", "deep", "high", "shallow"]):
        for rows in (FULL, MIXED):
            ng, ov, g = lib.ground(np.array([q[k] for k in order]), t["hf"], t["size_z"], prec, True, rows)
            for r, name in enumerate(order):
                if (rows >> r) & 1:
                    assert (ng[r], ov[r]) == alone[name][:2], (order, rows, name, ng[r], ov[r])
                    assert np.array_equal(g[r].view(np.uint8), alone[name][2].view(np.uint8)), (order, rows, name)
                else:
                    assert ng[r] == int(SENTINEL) and ov[r] == int(SENTINEL) and np.all(g[r] == SENTINEL), (order, r)
