"""GPU depth cameras: bb_render_depth against tests/render_ref.py,
an independent float64 ray caster (local-frame quadratics, brute force over the
heightfield's triangles; test_render_ref.py holds the oracle's renderer to it and
pins it analytically), plus the reference's frame cadence (every
ceil((1/90)/0.002) = 6 steps, relative_image_timestamp).

Cases (render_ref.CASES): five pose families (tilt, lift, edge with the corners and
5.2 m outside the field, ball displaced / culled / far, camera below the surface),
one 32-env camera env each with a different pose in every env, over a 4-slot bank
(flat, hills seed 7 at size_z 2, hills seed 11 at size_z 0.5, GPU perlin) pinned
round-robin; image sizes 64x64, 24x40, 40x24, 17x23, 5x3, 1x1 and 12x60; fp64 and
fp32 state.  The kernel renders into the test's own sentinel-filled buffer with guard
regions on both sides.

Per image: a pixel is *stable* if the reference's five samples (centre, +-3e-5 in
normalised image coordinates along x and y) see the same surface and both second
differences of the depth are <= 1e-6.  Every stable pixel is within the bound of
the reference, without exception; every unstable pixel lies within the min and max
of the five samples +- the bound (a hole in the ground cannot hide there); every
pixel is in (0, 1]; the guards are untouched.

Bound: min(1e-4, 8 x yardstick + 1e-6) per case.  The yardstick is the same
reference run in float32 on the same scenes, against its float64 run on stable
pixels (worst over the case's images); 8x is the margin this project gives a
different operation order, 1e-6 covers the float32 output rounding and the
overlap of the kernel's padded triangles; 1e-4 m is the earlier tolerance, kept
as a hard ceiling.

Worst error on stable pixels, kernel / yardstick per bank slot (flat, hills 7 at
size_z 2, hills 11 at size_z 0.5, GPU perlin), and the largest ratio; single run:

  tilt  64x64 fp64  1.6e-6/2.5e-6  2.1e-6/2.9e-6  2.4e-6/2.0e-6  4.7e-6/1.0e-5   1.2
  lift  24x40 fp64  1.8e-6/1.8e-6  2.3e-6/1.6e-6  1.7e-6/1.6e-6  3.0e-6/3.9e-6   1.4
  edge  40x24 fp64  6.1e-6/5.3e-6  7.2e-6/6.1e-6  5.0e-6/4.8e-6  1.3e-5/1.2e-5   1.2
  ball  24x40 fp64  1.7e-6/8.3e-7  2.0e-6/4.7e-6  1.6e-6/2.3e-6  2.3e-6/7.1e-6   2.1
  below 17x23 fp64  4.1e-7/3.8e-7  6.7e-7/4.6e-7  4.4e-7/7.1e-7  1.9e-6/4.2e-6   1.5
  tilt  17x23 fp32  6.5e-7/6.4e-7  7.1e-7/6.8e-7  5.6e-7/9.7e-7  2.3e-6/1.2e-5   1.0
  edge  24x40 fp32  2.2e-6/2.2e-6  1.9e-6/1.9e-6  2.0e-6/1.8e-6  7.7e-6/2.0e-5   1.2
  tilt  12x60 fp64  1.1e-6/5.6e-7  9.2e-7/7.5e-7  1.3e-6/1.9e-6  1.3e-6/2.6e-6   2.0

The kernel holds the adopted bound in every case (4x margin or more); no unstable
pixel leaves its five samples.  The 12x60 case is there for the robot's own
geometry: the cameras are fixed in the base, so every pose shows the same ball and
one wheel at the usual sizes, and only x out to +-5 brings the sticks, the other
wheels' far caps and the rays that pass the tower into view.

Found by these tests and fixed in csrc/bb_render.hip: one stable pixel of the tilt
family (flat slot, env 20, camera 0, pixel (45, 42), ground at 0.221 m) came back
as depth 1, a ray that slipped between two triangles in float; and rel_ts was one
float ulp high at steps % every = 5.

Parity against MuJoCo's OpenGL renderer itself is unpinned (MuJoCo is unavailable;
DESIGN.md §5).
"""
import ctypes as C

import numpy as np
import pytest

import render_ref as RR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENTINEL = -7.0
GUARD = 4096
CEILING = 1e-4


def _env(n, terrain, seed=0, **kw):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device="cuda:0", terrain_config=terrain, disable_cameras=False, auto_reset=False,
                         seed=seed, **kw)


def _render_raw(env, H, W, every=6, force=1):
    """bb_render_depth on the env's handle into a sentinel-filled buffer of the test's own, with a
    guard region on both sides -> (depth [n, 2, H, W], rel_ts [n]) on the host."""
    from ballbot_gym import _native as N

    n = env.num_envs
    size = n * 2 * H * W
    buf = torch.full((GUARD + size + GUARD,), SENTINEL, dtype=torch.float32, device=env.device)
    ts = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=env.device)
    N.check(N.lib().bb_render_depth(env._h, C.c_void_p(buf[GUARD:].data_ptr()), C.c_void_p(ts[GUARD:].data_ptr()),
                                    H, W, every, force, None), "bb_render_depth")
    torch.cuda.synchronize()
    b, t = buf.cpu().numpy(), ts.cpu().numpy()
    for a, m in ((b, size), (t, n)):
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + m:] == SENTINEL).all(), "guard region written"
    return b[GUARD:GUARD + size].reshape(n, 2, H, W), t[GUARD:GUARD + n]


@pytest.fixture(scope="module")
def fields():
    return [(h, z) for h, z in zip(RR.bank() + [RR.perlin_field()], RR.SIZE_Z)]


def _bank_env(fields, precision="fp64"):
    """A camera env over the 4-slot bank, env e pinned to slot e % 4."""
    from ballbot_gym import _native as N
    from ballbot_gym.envs.config import np_random

    env = _env(RR.N_ENVS, {"type": "perlin", "config": {}}, terrain_slots=len(fields), precision=precision)
    assert env.precision == precision
    for slot, (hf, size_z) in enumerate(fields[:3]):
        N.check(N.lib().bb_set_hfield(env._h, slot, hf.ctypes.data_as(C.POINTER(C.c_float)), float(size_z)),
                "bb_set_hfield")
    env.load_terrain(3, int(np_random(0).integers(0, 10000)))  # generated on the GPU
    ids = np.arange(RR.N_ENVS, dtype=np.int32) % len(fields)
    env.assign_terrain(ids)  # acts on later resets
    env.reset()
    assert (env.env_terrain()[0] == ids).all()
    return env


def _check_image(got, ref, bound, where):
    """The per-image assertions; -> the worst error on stable pixels."""
    assert np.isfinite(got).all() and (got > 0).all() and (got <= 1).all(), (where, float(got.min()), float(got.max()))
    st = ref["stable"]
    err = np.abs(got - ref["d"])
    worst = float(err[st].max()) if st.any() else 0.0
    assert worst <= bound, (where, "stable pixel", np.unravel_index(np.argmax(np.where(st, err, 0)), err.shape),
                            worst, bound)
    out = np.maximum(ref["lo"] - got, got - ref["hi"])[~st]
    assert (out <= bound).all(), (where, "unstable pixel outside its five samples", float(out.max()), bound)
    return worst


def _run_case(oracle, fields, family, H, W, precision):
    """One render call of a 32-env camera env at the family's poses -> (depth [n, 2, H, W], the
    reference of every image {(env, cam): ...}, the float32 yardstick per bank slot)."""
    q0 = oracle.reset_state(0.01)[0]
    Q = RR.poses(family, fields, q0)
    env = _bank_env(fields, precision)
    env.set_state(Q, np.zeros((RR.N_ENVS, 15)), None, np.zeros(RR.N_ENVS, np.int32))
    if precision == "fp32":  # the reference gets the state the kernel holds
        Q = env.get_state()[0]
        assert np.array_equal(Q, Q.astype(np.float32).astype(np.float64))
    depth, _ = _render_raw(env, H, W)
    env.close()
    refs, yard = {}, np.zeros(len(fields))
    for e in range(RR.N_ENVS):
        hf, size_z = fields[e % len(fields)]
        for cam in (0, 1):
            scene = oracle.render_scene(Q[e], cam)
            ref = refs[e, cam] = RR.stable_reference(scene, hf, size_z, H, W)
            d32, _ = RR.render(scene, hf, size_z, H, W, dtype=np.float32)
            if ref["stable"].any():
                yard[e % len(fields)] = max(yard[e % len(fields)], np.abs(d32 - ref["d"])[ref["stable"]].max())
    return depth, refs, yard


@pytest.mark.parametrize("family,H,W,precision", RR.CASES, ids=lambda v: str(v))
def test_depth_matches_reference(oracle, fields, family, H, W, precision):
    depth, refs, yard = _run_case(oracle, fields, family, H, W, precision)
    bound = min(CEILING, 8 * yard.max() + 1e-6)
    for (e, cam), ref in refs.items():
        _check_image(depth[e, cam], ref, bound, (family, (H, W), precision, e, cam))


@pytest.mark.parametrize("terrain", ["flat", "hills", "perlin"])
def test_depth_matches_oracle(oracle, terrain):
    """Recorded states (the robot balancing at the field centre), every env and camera at three
    times.  No pixel may differ from the oracle by more than 1e-4 unless the reference calls it
    unstable and the kernel stays within the reference's five samples there; the first envs are
    also held to the reference itself by the stable-pixel rule."""
    import traj
    from ballbot_gym.envs.config import np_random
    from ballbot_gym.terrain import generate_hills_terrain
    from ballbot_gym.terrain.perlin import generate_perlin_terrain

    kw = {}
    if terrain == "flat":
        hf, tcfg = oracle.flat_hfield(), {"type": "flat", "config": {}}
    elif terrain == "hills":
        hf = generate_hills_terrain(293, seed=7).astype(np.float32)
        tcfg = {"type": "hills", "config": {"seed": 7}}
    else:  # GPU bank slot 0 = the first seed of np_random(0); sloped ground in view
        hf = generate_perlin_terrain(293, seed=int(np_random(0).integers(0, 10000))).astype(np.float32)
        tcfg, kw = {"type": "perlin", "config": {}}, {"n_terrains": 1, "shared_stream": True}
    rec = traj.record(n_envs=32, n_steps=40, hfield=hf, seed=21)
    env = _env(32, tcfg, **kw)
    for t in (0, 13, 39):
        q = rec["qpos"][t]
        env.set_state(q, rec["qvel"][t], rec["warm"][t], np.zeros(32, np.int32))
        depth = env.render_depth(force=True).cpu().numpy()
        for e in range(32):
            for cam in (0, 1):
                got = depth[e, cam]
                assert (got > 0).all() and (got <= 1).all()
                bad = np.abs(got - oracle.render_depth(q[e], hf, cam)) > CEILING
                assert bad.mean() <= 0.005, (t, e, cam, int(bad.sum()))  # the earlier rule still holds
                if e < 2 or bad.any():
                    ref = RR.stable_reference(oracle.render_scene(q[e], cam), hf, 2.0, 64, 64)
                    assert not (bad & ref["stable"]).any(), (t, e, cam, int(bad.sum()))
                    _check_image(got, ref, CEILING, (terrain, t, e, cam))
    env.close()


def test_partial_render_touches_only_due_envs(fields):
    """force=0 renders the envs whose step counter is a multiple of the frame interval and leaves
    the other images alone; rel_ts = float(double(steps % every) * 0.002) for every env."""
    env = _bank_env(fields)
    rng = np.random.default_rng(5)
    q, v, w, _ = env.get_state()
    q[:, 7:10] = rng.uniform(-np.pi, np.pi, (RR.N_ENVS, 3))
    steps = np.tile(np.array([0, 1, 5, 6, 7, 12, 13, 4000], np.int32), RR.N_ENVS // 8)
    env.set_state(q, v, w, steps)
    H, W = 17, 23
    full, _ = _render_raw(env, H, W, 6, force=1)
    assert (full > 0).all() and (full <= 1).all()
    for every in (1, 6, 7):
        part, ts = _render_raw(env, H, W, every, force=0)
        due = steps % every == 0
        assert due.any() and (every == 1 or (~due).any())
        assert np.array_equal(part[due], full[due]), every
        assert (part[~due] == SENTINEL).all(), every
        want = (np.float64(steps % every) * 0.002).astype(np.float32)
        assert np.array_equal(ts, want), (every, ts[:8], want[:8])
    env.close()


def test_frame_cadence_and_timestamp():
    env = _env(64, {"type": "flat", "config": {}})
    env.reset()
    acts = torch.zeros(64, 3, device=env.device)
    first = env.depth.clone()
    for k in range(1, 13):
        env.step(acts)
        od = env.obs_dict()
        assert set(od) == {"actions", "angular_vel", "motor_state", "orientation", "relative_image_timestamp",
                           "rgbd_0", "rgbd_1", "vel"}
        assert od["rgbd_0"].shape == (64, 1, 64, 64)
        ts = od["relative_image_timestamp"].cpu().numpy()[:, 0]
        assert np.allclose(ts, (k % 6) * 0.002, atol=1e-7), (k, ts[:3])
        if k % 6:
            assert torch.equal(env.depth, first), k  # images are held between frames
        else:
            first = env.depth.clone()
    env.close()
