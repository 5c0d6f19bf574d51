"""The ball-terrain pass's cell window (csrc/bb_physics.h: prism_window, kPrismWindow; bb_team16.h: collide_team;
bb_step.h: forward hands in TerrainRef::hz) through the whole step on the GPU.

The product library against the build of the same source with the window and every pre-phase form compiled out
(_native.SERIAL_FLAGS, -DBB_NO_PRISM_WINDOW among them: _native.SERIAL_LIB_PATH), bit for bit, in fp64 and fp32 at
1, 3, 17 and 65 envs (a lone team, partial waves, more than one workgroup): one bb_step, then one 20-step
bb_step_multi launch; final state, warm start, step counters, the five output arrays of both calls and every counter
of bb_get_stats.

  flat    tests/test_gpu_prephase.py's states (settled and moving, with an env that auto-resets inside the window,
          one that hands over to the full step and one started from a NaN qpos), the regular envs lowered by a
          further 0 to 30 mm (robot and ball together), so that the window runs from a cell or two to the whole
          sub-grid under the ball: here the bound is 0 and cuts the most
  perlin  tests/test_gpu_pre_batch.py's bank with one generator per env, the ball pressed 0.2 mm to 30 mm into its
          env's terrain, and envs whose base lies on the terrain (hand-overs): here the bound is the terrain's top
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_gpu_pre_batch as PB  # noqa: E402
import test_gpu_prephase as PP  # noqa: E402

ENV_COUNTS = PP.ENV_COUNTS
K = PP.K
LOWER = (0.0, 0.0002, 0.001, 0.002, 0.004, 0.008, 0.015, 0.03)  # m, further into the flat ground


@pytest.fixture(scope="module")
def libs():
    from ballbot_gym import _native as N

    assert "-DBB_NO_PRISM_WINDOW" in N.SERIAL_FLAGS
    assert N.SERIAL_LIB_PATH.exists(), f"{N.SERIAL_LIB_PATH} not built (__graft_entry__.build())"
    return N._load(N.LIB_PATH), N._load(N.SERIAL_LIB_PATH)


def _actions(n, seed):
    rng = np.random.default_rng(seed)
    a1 = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    aK = rng.uniform(-1, 1, (K, n, 3)).astype(np.float32)
    return torch.tensor(a1, device="cuda:0"), torch.tensor(aK, device="cuda:0")


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_flat_product_equals_serial_build(libs, oracle, n, precision, monkeypatch):
    qs, vs, ws, steps, kind = PP._states(oracle, n)
    for e in np.nonzero(kind == 0)[0]:
        qs[e, 2] -= LOWER[e % len(LOWER)]
        qs[e, 12] -= LOWER[e % len(LOWER)]
    st = (qs, vs, ws, steps, kind)
    acts1, actsK = _actions(n, 700 + n)
    got, ref = (PP._run(lib, n, precision, st, acts1, actsK, monkeypatch) for lib in libs)
    PB._assert_same(got, ref)
    done1, doneK = got["step"][2], got["multi"][2]
    for e in np.nonzero(kind == 1)[0]:
        assert doneK[3, e] & 1 and not doneK[2, e] & 1, f"env {e}: no episode end at its step limit"
    for e in np.nonzero(kind == 3)[0]:
        assert done1[e] & 4 and doneK[0, e] & 4, f"env {e}: no divergence reset from the NaN qpos"


@pytest.mark.parametrize("precision", ["fp64", "fp32"])
@pytest.mark.parametrize("n", ENV_COUNTS)
def test_perlin_product_equals_serial_build(libs, oracle, n, precision, monkeypatch):
    acts1, actsK = _actions(n, 900 + n)
    got = PB._run_perlin(libs[0], oracle, n, precision, None, acts1, actsK, monkeypatch)
    ref = PB._run_perlin(libs[1], oracle, n, precision, got["st"], acts1, actsK, monkeypatch)
    assert np.array_equal(got["ncon"], ref["ncon"])
    PB._assert_same(got, ref)
    ng, nb = got["ncon"][:, 0], got["ncon"][:, 1]
    print(f"\n{n} perlin envs {precision}: ball-terrain contacts {sorted(ng.tolist())}, base-tree contacts on "
          f"{int((nb > 0).sum())} envs")
    if n >= 17:  # the pressed envs have ball-terrain contacts on both sides of one round's 16 prisms' worth
        fast = nb == 0
        assert (ng[fast] >= 1).any() and (ng[fast] >= 14).any(), sorted(ng[fast].tolist())
