"""The fused broadcast-FMA of bb_team16.h (fmac_bcast / fnmac_bcast: one v_fmac_f64_dpp) against the
plain broadcast move + FMA it replaces, bit for bit, on one workgroup of 64 lanes (four teams).

tests/hostcheck/dpp_fmac_check.hip is built twice: as shipped, and with -DBB_NO_FMAC_DPP (the plain
pair everywhere).  Within the shipped build the primitive is compared with fma(bcast<J>(x), own, acc)
for all 16 J and both signs; between the two builds the register-row Cholesky and its two sweeps are
compared on random SPD systems.  "Mixed rows" leaves rows 0 and 2 of the wave live and rows 1 and 3
exited, the state of a wave whose teams converged at different Newton iterations.
"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

torch = pytest.importorskip("torch")  # its HIP runtime is loaded before the check program's
pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "hostcheck" / "dpp_fmac_check.hip"
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
NV, TL = 15, 16
FULL, MIXED = 0b1111, 0b0101
SENTINEL = -12345.0  # what the lanes of exited rows must leave in place


def _build(name, flags):
    out = ROOT / "tests" / "_build" / f"libdpp_fmac_{name}.so"
    out.parent.mkdir(parents=True, exist_ok=True)
    srcs = [SRC] + sorted(CSRC.glob("*.h"))
    if not (out.exists() and all(out.stat().st_mtime >= s.stat().st_mtime for s in srcs)):
        subprocess.run(["hipcc", "-O2", "-fPIC", "-shared", "--offload-arch=gfx950", "-std=c++17", "-w",
                        f"-I{CSRC}", *flags, "-o", str(out), str(SRC)], check=True)
    L = C.CDLL(str(out))
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    L.dc_prim.argtypes = [dp, dp, dp, C.c_int, C.c_int, C.c_int, dp]
    L.dc_solve_f64.argtypes = [dp, dp, C.c_int, dp]
    L.dc_solve_f32.argtypes = [fp, fp, C.c_int, fp]
    return L


@pytest.fixture(scope="module")
def libs():
    fused, plain = _build("fused", []), _build("plain", ["-DBB_NO_FMAC_DPP"])
    assert fused.dc_fused_build() == 1 and plain.dc_fused_build() == 0
    return fused, plain


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double if a.dtype == np.float64 else C.c_float))


def _prim_inputs(seed):
    """acc, x, own for the 64 lanes: random doubles over 600 decades with +-0, denormals and 1e+-300
    mixed in, so that products and sums round, underflow, overflow and cancel."""
    rng = np.random.default_rng(seed)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.5e-310, -1e-308, 1e300, -1e300, 1e-300, -1e-300, 1.0, -1.0])
    out = []
    for _ in range(3):
        v = rng.choice([-1.0, 1.0], 64) * 10.0 ** rng.uniform(-300, 300, 64) * rng.uniform(1, 10, 64)
        idx = rng.choice(64, 24, replace=False)
        v[idx] = rng.choice(special, 24)
        out.append(np.ascontiguousarray(v))
    return out


def _prim(lib, acc, x, own, rows, fused, hazard):
    out = np.full(2 * TL * 64, SENTINEL)
    assert lib.dc_prim(_ptr(acc), _ptr(x), _ptr(own), rows, int(fused), int(hazard), _ptr(out)) == 0
    return out.reshape(2 * TL, 64)


def _live(rows):
    return np.repeat([(rows >> t) & 1 == 1 for t in range(4)], TL)


def _assert_same_bits(a, b, what):
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    bad = np.argwhere(a.view(bits) != b.view(bits))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {i}: {a[i]!r} vs {b[i]!r}")


@pytest.mark.parametrize("seed", [0, 1])
def test_primitive_full_wave(libs, seed):
    """All 16 J, both signs, all four rows live."""
    fused_lib, _ = libs
    acc, x, own = _prim_inputs(seed)
    got = _prim(fused_lib, acc, x, own, FULL, True, False)
    ref = _prim(fused_lib, acc, x, own, FULL, False, False)
    _assert_same_bits(got, ref, "fmac_bcast vs fma(bcast)")
    # and both are what they say: lane J of each row, times own, added to or taken from acc.  With
    # all three in [1, 2), numpy's product (< 4, half an ulp 4.4e-16) and sum (< 6, half an ulp
    # 4.4e-16) are within 9e-16 of the single rounding; another lane's x is off by about 0.1
    rng = np.random.default_rng(7 + seed)
    a1, x1, o1 = (np.ascontiguousarray(rng.uniform(1, 2, 64)) for _ in range(3))
    g1 = _prim(fused_lib, a1, x1, o1, FULL, True, False)
    for J in range(TL):
        xb = np.repeat(x1.reshape(4, TL)[:, J], TL)
        assert np.abs(g1[2 * J] - (a1 + xb * o1)).max() <= 9e-16, J
        assert np.abs(g1[2 * J + 1] - (a1 - xb * o1)).max() <= 9e-16, J


@pytest.mark.parametrize("hazard", [False, True])
def test_primitive_mixed_rows(libs, hazard):
    """Rows 0 and 2 live, rows 1 and 3 exited; with `hazard`, x is the result of the VALU instruction
    immediately before each fused one (the wait states the wrapper must supply itself)."""
    fused_lib, _ = libs
    acc, x, own = _prim_inputs(2)
    if hazard:  # x is multiplied by [1, 2) 32 times: start it where it stays finite for most lanes
        x = np.ascontiguousarray(np.where(np.abs(x) > 1e280, x * 1e-100, x))
    got = _prim(fused_lib, acc, x, own, MIXED, True, hazard)
    ref = _prim(fused_lib, acc, x, own, MIXED, False, hazard)
    _assert_same_bits(got, ref, "mixed rows")
    live = _live(MIXED)
    assert np.all(got[:, ~live] == SENTINEL)
    assert not np.any(got[:, live] == SENTINEL)
    if hazard:  # the chain really went through the primitive's results: it differs from the unchained run
        assert not np.array_equal(got[2:, live], _prim(fused_lib, acc, x, own, MIXED, True, False)[2:, live])


def _spd_systems(cond, seed):
    """Four random SPD 15x15 matrices (one per team) of the given condition number, and gradients."""
    rng = np.random.default_rng(seed)
    H = np.empty((4, NV, NV))
    for t in range(4):
        Q, _ = np.linalg.qr(rng.normal(size=(NV, NV)))
        ev = 10.0 ** np.linspace(0, np.log10(cond), NV)
        A = (Q * ev) @ Q.T
        H[t] = 0.5 * (A + A.T)
    return np.ascontiguousarray(H), np.ascontiguousarray(rng.normal(size=(4, NV)))


def _solve(lib, H, g, rows, dtype):
    Hd, gd = np.ascontiguousarray(H, dtype), np.ascontiguousarray(g, dtype)
    out = np.full(64 * (3 * NV + 1), SENTINEL, dtype)
    fn = lib.dc_solve_f64 if dtype == np.float64 else lib.dc_solve_f32
    assert fn(_ptr(Hd), _ptr(gd), rows, _ptr(out)) == 0
    return out.reshape(64, 3 * NV + 1)


@pytest.mark.parametrize("rows", [FULL, MIXED], ids=["full", "mixed"])
@pytest.mark.parametrize("cond", [1e2, 1e10])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_solve_fused_equals_plain(libs, dtype, cond, rows):
    """chol_rows + chol_solve_rows: the factor's rows, the inverse pivots, the replicated solution
    and each lane's own component, the fused build against the -DBB_NO_FMAC_DPP build."""
    fused_lib, plain_lib = libs
    H, g = _spd_systems(cond, seed=int(np.log10(cond)))
    got, ref = _solve(fused_lib, H, g, rows, dtype), _solve(plain_lib, H, g, rows, dtype)
    _assert_same_bits(got, ref, "solve")
    live = _live(rows)
    assert np.all(got[~live] == dtype(SENTINEL))
    if dtype == np.float64 and cond == 1e2:
        # and it is the solve: s = -H^-1 g.  A backward-stable Cholesky solve of a 15x15 system is
        # within about n cond eps = 15 * 1e2 * 1.1e-16 = 2e-13 of it, relative to |s|; 1e-11 leaves
        # room for the hardware reciprocal square root's correction step
        for t in range(4):
            if not (rows >> t) & 1:
                continue
            s_ref = -np.linalg.solve(H[t], g[t])
            for tl in range(TL):
                s = got[t * TL + tl, 2 * NV:3 * NV]
                assert np.abs(s - s_ref).max() <= 1e-11 * np.abs(s_ref).max(), (t, tl)
                if tl < NV:
                    assert got[t * TL + tl, 3 * NV] == s[tl]
