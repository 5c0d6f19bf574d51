"""GPU onboard RGB-D cameras (csrc/bb_rgbd.hip, bb_render_rgbd) against tests/rgbd_ref.py, the fp64
reference of the frame's definition, plus the cadence, the env surface, the single
env's logs and the trainer on 4-channel frames.

Cases (rgbd_ref.CASES): render_ref's five pose families over the 4-slot bank (flat, hills seed 7 at
size_z 2, hills seed 11 at size_z 0.5, GPU perlin) pinned round-robin, a different pose in every
env, both cameras; sizes 24x40, 17x23, 12x60, 5x3, 1x1 and 64x64; fp32 state on edge 17x23, tilt
5x3 and edge 1x1 (the reference reads the state back), fp64 elsewhere.  The kernel writes into the
test's own sentinel-filled buffers with 4097-float / 4097-byte guards on both sides, so the image
base is not 16-byte aligned and both cases of the packed row store run.

Per image: every R, G, B value is bit-equal to float32(k) / float32(255) for an integer k.  A pixel
is *stable* if the reference's five samples (centre, +-3e-5 in normalised image coordinates along x
and y) agree in surface id, colour class and hit triangle and both second differences of the depth
are <= 1e-6 (test_rgbd_ref.py asserts the share).  Every stable pixel has the reference's id,
without exception, and each of R, G, B within +-1 count; every unstable pixel shows an id of one of
the five samples and channels within their min / max +- 1.  The +-1 is test_gpu_view's: float32
moves 255 c by about 0.03 at most, so only a value at a rounding boundary of int(255 c + 0.5) can
differ, and by one.  The D plane is held by the depth camera's rule (test_gpu_render.py, restated
here) against render_ref.stable_reference: every stable pixel within min(1e-4, 8 x yardstick +
1e-6), the yardstick being render_ref run in float32 on the same scenes; unstable pixels within
their five samples +- the bound; every pixel in (0, 1].

Worst count difference on stable pixels and how many differ at all; worst D error / bound; and how
many D pixels differ at all from bb_render_depth on the same state (reported, not asserted: the
two units may contract differently), per case (single run):

  tilt  24x40 x16 fp64  0    0 of  30664   D 4.1e-06 / 4.6e-05  vs depth kernel 11277 of  30720, at most 5.1e-07
  lift  24x40 x16 fp64  1    1 of  30540   D 2.1e-06 / 2.1e-05  vs depth kernel 10960 of  30720, at most 1.1e-06
  edge  17x23 x32 fp32  1    3 of  25007   D 3.1e-06 / 7.1e-05  vs depth kernel  8066 of  25024, at most 5.4e-07
  ball  17x23 x32 fp64  1    1 of  24932   D 2.4e-06 / 6.0e-05  vs depth kernel  4273 of  25024, at most 8.3e-07
  below 17x23 x16 fp64  0    0 of  12512   D 1.9e-06 / 6.9e-06  vs depth kernel  1507 of  12512, at most 4.1e-07
  tilt  12x60 x32 fp64  1    3 of  45962   D 1.2e-06 / 2.2e-05  vs depth kernel 13507 of  46080, at most 1.4e-06
  tilt   5x3  x8  fp32  0    0 of    225   D 4.3e-07 / 1.6e-05  vs depth kernel    74 of    240, at most 1.3e-06
  edge   1x1  x8  fp32  0    0 of     16   D 5.8e-07 / 7.3e-06  vs depth kernel     2 of     16, at most 3.0e-08
  tilt  64x64 x8  fp64  0    0 of  65403   D 3.7e-06 / 4.0e-05  vs depth kernel 20675 of  65536, at most 2.0e-06

No stable pixel shows another surface than the reference, and no unstable pixel leaves its five
samples.  A quarter to a third of the D pixels differ in their bits from the depth kernel's: the two
units contract their products differently, by 2.0e-6 at most, and both hold the same bound against
the reference.

The tower is in view of neither camera in any family (test_rgbd_ref.py), so its colour is not
asserted from here.  Parity against MuJoCo's OpenGL image itself is unpinned (MuJoCo is
unavailable).
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import render_ref as RR
import rgbd_ref as GR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD = 4097  # floats / bytes: the image's first element is not 16-byte aligned
SENT_F, SENT_B = -7.0, 0x5A
CEILING = 1e-4


def _env(n, terrain, seed=0, **kw):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device="cuda:0", terrain_config=terrain, auto_reset=False, seed=seed, **kw)


def _bank_env(n, precision="fp64"):
    """An env over the 4-slot bank, env e pinned to slot e % 4."""
    from ballbot_gym import _native as N
    from ballbot_gym.envs.config import np_random

    fields = GR.fields()
    env = _env(n, {"type": "perlin", "config": {}}, terrain_slots=len(fields), precision=precision)
    assert env.precision == precision
    for slot, (hf, size_z) in enumerate(fields[:3]):
        N.check(N.lib().bb_set_hfield(env._h, slot, hf.ctypes.data_as(C.POINTER(C.c_float)), float(size_z)),
                "bb_set_hfield")
    env.load_terrain(3, int(np_random(0).integers(0, 10000)))  # generated on the GPU
    ids = np.arange(n, dtype=np.int32) % len(fields)
    env.assign_terrain(ids)  # acts on later resets
    env.reset()
    assert (env.env_terrain()[0] == ids).all()
    return env


def _render_raw(env, H, W, every=6, force=1, want_ids=True):
    """bb_render_rgbd on the env's handle into sentinel-filled buffers of the test's own with a guard
    region on both sides -> (rgbd [n, 2, 4, H, W], ids int8 [n, 2, H, W], rel_ts [n]) on the host."""
    from ballbot_gym import _native as N

    n = env.num_envs
    nf, nb = n * 2 * 4 * H * W, n * 2 * H * W
    buf = torch.full((GUARD + nf + GUARD,), SENT_F, dtype=torch.float32, device=env.device)
    ids = torch.full((GUARD + nb + GUARD,), SENT_B, dtype=torch.int8, device=env.device)
    ts = torch.full((GUARD + n + GUARD,), SENT_F, dtype=torch.float32, device=env.device)
    assert buf[GUARD:].data_ptr() % 16 != 0
    N.check(N.lib().bb_render_rgbd(env._h, C.c_void_p(buf[GUARD:].data_ptr()), C.c_void_p(ts[GUARD:].data_ptr()),
                                   C.c_void_p(ids[GUARD:].data_ptr()) if want_ids else None, H, W, every, force, None),
            "bb_render_rgbd")
    torch.cuda.synchronize()
    b, i, t = buf.cpu().numpy(), ids.cpu().numpy(), ts.cpu().numpy()
    for a, m, s in ((b, nf, SENT_F), (i, nb, SENT_B), (t, n, SENT_F)):
        assert (a[:GUARD] == s).all() and (a[GUARD + m:] == s).all(), "guard region written"
    if not want_ids:
        assert (i == SENT_B).all()
    return b[GUARD:GUARD + nf].reshape(n, 2, 4, H, W), i[GUARD:GUARD + nb].reshape(n, 2, H, W), t[GUARD:GUARD + n]


def _render_depth_raw(env, H, W):
    from ballbot_gym import _native as N

    out = torch.full((env.num_envs, 2, H, W), SENT_F, dtype=torch.float32, device=env.device)
    N.check(N.lib().bb_render_depth(env._h, C.c_void_p(out.data_ptr()), None, H, W, 6, 1, None), "bb_render_depth")
    torch.cuda.synchronize()
    return out.cpu().numpy()


COUNTS = np.arange(256, dtype=np.float32) / np.float32(255)


def _counts(rgb, where):
    """The integer counts of an R, G, B block; every value bit-equal to float32(k) / float32(255)."""
    k = np.rint(rgb.astype(np.float64) * 255).astype(np.int64)
    assert (k >= 0).all() and (k <= 255).all(), where
    assert np.array_equal(COUNTS[k].view(np.uint32), rgb.view(np.uint32)), (where, "not float32(k) / 255")
    return k.astype(np.int16)


def _check_colour(rgb, ids, ref, where):
    """rgb [3, H, W] planes, ids [H, W] -> (worst count difference on stable pixels, how many differ)."""
    q = _counts(rgb, where).transpose(1, 2, 0)  # [H, W, 3]
    st = ref["stable"]
    assert (ids[st] == ref["ids"][st]).all(), (where, "stable pixel id", np.argwhere(st & (ids != ref["ids"]))[:4])
    diff = np.abs(q - ref["q"].astype(np.int16)).max(-1)
    worst = int(diff[st].max()) if st.any() else 0
    assert worst <= 1, (where, "stable pixel colour", np.argwhere(st & (diff > 1))[:4], worst)
    un = ~st
    assert (ids[None] == ref["ids5"]).any(0)[un].all(), (where, "unstable pixel: id of none of its five samples")
    out = np.maximum(ref["lo"] - q, q - ref["hi"]).max(-1)
    assert (out[un] <= 1).all(), (where, "unstable pixel outside its five samples", int(out[un].max()))
    return worst, int((diff[st] > 0).sum())


def _check_depth(got, ref, bound, where):
    """The depth camera's per-image rule (render_ref.stable_reference) -> worst error on stable pixels."""
    assert np.isfinite(got).all() and (got > 0).all() and (got <= 1).all(), (where, float(got.min()), float(got.max()))
    st = ref["stable"]
    err = np.abs(got - ref["d"])
    worst = float(err[st].max()) if st.any() else 0.0
    assert worst <= bound, (where, "stable D pixel", np.unravel_index(np.argmax(np.where(st, err, 0)), err.shape),
                            worst, bound)
    out = np.maximum(ref["lo"] - got, got - ref["hi"])[~st]
    assert (out <= bound).all(), (where, "unstable D pixel outside its five samples", float(out.max()), bound)
    return worst


@pytest.mark.parametrize("case", GR.CASES, ids=lambda c: "-".join(map(str, c)))
def test_rgbd_matches_reference(oracle, case):
    family, H, W, n, precision = case
    Q = GR.case_poses(oracle, family, n, precision)
    env = _bank_env(n, precision)
    env.set_state(Q, np.zeros((n, 15)), None, np.zeros(n, np.int32))
    assert np.array_equal(env.get_state()[0], Q)  # fp32: the reference has the state the kernel holds
    rgbd, ids, _ = _render_raw(env, H, W)
    only, _, _ = _render_raw(env, H, W, want_ids=False)  # ids_dev may be NULL
    assert np.array_equal(only.view(np.uint32), rgbd.view(np.uint32))
    depth = _render_depth_raw(env, H, W)
    env.close()
    refs = GR.case_references(oracle, family, H, W, n, precision)
    F = GR.fields()
    drefs, yard = {}, 0.0
    for e in range(n):
        hf, size_z = F[e % len(F)]
        for cam in (0, 1):
            scene = oracle.render_scene(Q[e], cam)
            dref = drefs[e, cam] = RR.stable_reference(scene, hf, size_z, H, W)
            d32, _ = RR.render(scene, hf, size_z, H, W, dtype=np.float32)
            if dref["stable"].any():
                yard = max(yard, float(np.abs(d32 - dref["d"])[dref["stable"]].max()))
    bound = min(CEILING, 8 * yard + 1e-6)
    worst = differ = stable = 0
    dworst = 0.0
    for (e, cam), ref in refs.items():
        where = (case, e, cam)
        w, k = _check_colour(rgbd[e, cam, :3], ids[e, cam], ref, where)
        worst, differ, stable = max(worst, w), differ + k, stable + int(ref["stable"].sum())
        dworst = max(dworst, _check_depth(rgbd[e, cam, 3], drefs[e, cam], bound, where))
    same = int((rgbd[:, :, 3].view(np.uint32) != depth.view(np.uint32)).sum())
    apart = float(np.abs(rgbd[:, :, 3] - depth).max())
    print(f"RGBD {family:5s} {H}x{W} x{n} {precision}  {worst} {differ:4d} of {stable:6d}   "
          f"D {dworst:.1e} / {bound:.1e}"
          f"  vs depth kernel {same} of {depth.size:6d}, at most {apart:.1e}")


def test_partial_render_touches_only_due_envs():
    """force=0 renders the envs whose step counter is a multiple of the frame interval and leaves the
    other images and ids alone; rel_ts = float(double(steps % every) * 0.002) for every env."""
    n = 16
    env = _bank_env(n)
    rng = np.random.default_rng(5)
    q, v, w, _ = env.get_state()
    q[:, 7:10] = rng.uniform(-np.pi, np.pi, (n, 3))
    steps = np.tile(np.array([0, 1, 5, 6, 7, 12, 13, 4000], np.int32), n // 8)
    env.set_state(q, v, w, steps)
    H, W = 17, 23
    full, full_ids, _ = _render_raw(env, H, W, 6, force=1)
    assert (full >= 0).all() and (full <= 1).all() and (full_ids >= 0).all() and (full_ids <= 8).all()
    for every in (1, 6, 7):
        part, part_ids, ts = _render_raw(env, H, W, every, force=0)
        due = steps % every == 0
        assert due.any() and (every == 1 or (~due).any())
        assert np.array_equal(part[due].view(np.uint32), full[due].view(np.uint32)), every
        assert (part[~due] == SENT_F).all(), every
        assert np.array_equal(part_ids[due], full_ids[due]) and (part_ids[~due] == SENT_B).all(), every
        want = (np.float64(steps % every) * 0.002).astype(np.float32)
        assert np.array_equal(ts, want), (every, ts[:8], want[:8])
    env.close()


def test_env_surface(oracle):
    from ballbot_gym.envs import BallbotVecEnv

    kw = dict(device="cuda:0", terrain_config={"type": "flat", "config": {}}, disable_cameras=False, seed=3)
    cam = {"height": 16, "width": 16}
    env = BallbotVecEnv(8, env_config={"camera": {**cam, "disable_rgb": False}}, **kw)
    plain = BallbotVecEnv(8, env_config={"camera": {**cam, "disable_rgb": True}}, **kw)
    assert env.cam_channels == 4 and plain.cam_channels == 1
    assert tuple(env.rgbd.shape) == (8, 2, 4, 16, 16) and tuple(env.depth.shape) == (8, 2, 16, 16)
    assert env.depth.data_ptr() == env.rgbd[:, :, 3].data_ptr() and env.depth.stride() == env.rgbd[:, :, 3].stride()
    assert env.observation_space["rgbd_0"].shape == (4, 16, 16)
    assert plain.observation_space["rgbd_0"].shape == (1, 16, 16)
    # env 3 starts tilted past the limit: it fails in the first step and is reset (and rendered) in it
    q, v, w, s = env.get_state()
    q[3] = RR._place(q[3], (0.0, 0.0), 0.0, 0.0, np.array([0.6, 0.0, 0.0]), np.zeros(3))
    for e_ in (env, plain):
        e_.set_state(q, v, w, s)
        e_.render_depth(force=True)
    tilted = env.rgbd[3].clone()
    acts = torch.zeros(8, 3, device=env.device)
    held = env.rgbd.clone()
    for k in range(1, 14):
        _, _, term, _, _ = env.step(acts)
        plain.step(acts)
        od = env.obs_dict()
        assert set(od) == {"actions", "angular_vel", "motor_state", "orientation", "relative_image_timestamp",
                           "rgbd_0", "rgbd_1", "vel"}
        assert tuple(od["rgbd_0"].shape) == (8, 4, 16, 16) and tuple(od["rgbd_1"].shape) == (8, 4, 16, 16)
        host = {key: val[0].cpu().numpy() for key, val in od.items()}
        assert env.observation_space.contains(host), k
        steps = env.get_state()[3]
        assert bool(term[3]) == (k == 1) and steps[3] == k - 1 and (np.delete(steps, 3) == k).all()
        due = torch.as_tensor(steps % 6 == 0, device=env.device)
        assert bool(due[3]) == (k in (1, 7, 13)) and bool(due[0]) == (k % 6 == 0)
        ts = od["relative_image_timestamp"].cpu().numpy()[:, 0]
        assert np.allclose(ts, (steps % 6) * 0.002, atol=1e-7), (k, ts)
        fresh, _, _ = _render_raw(env, 16, 16)
        fresh = torch.as_tensor(fresh).to(env.device)
        assert torch.equal(env.rgbd[~due], held[~due]), k  # images are held between frames
        assert torch.equal(env.rgbd[due], fresh[due]), k   # and renewed when due
        if k == 1:
            assert not torch.equal(env.rgbd[3], tilted)  # the reset env shows its new pose
        held = env.rgbd.clone()
        assert torch.equal(env.depth, env.rgbd[:, :, 3])
        assert np.array_equal(plain.get_state()[0], env.get_state()[0])
    assert env.render_rgbd(force=True) is env.rgbd
    with pytest.raises(RuntimeError):
        plain.render_rgbd()
    # the depth-only env at the same states: its image and the D plane are both held to the depth
    # reference by the depth rule, and lie within its bound of each other on stable pixels
    Q = env.get_state()[0]
    d4, d1 = env.depth.cpu().numpy(), plain.render_depth(force=True).cpu().numpy()
    flat = np.zeros(RR.HF_N * RR.HF_N, np.float32)
    drefs, yard = {}, 0.0
    for e in range(8):
        for c in (0, 1):
            scene = oracle.render_scene(Q[e], c)
            dref = drefs[e, c] = RR.stable_reference(scene, flat, 2.0, 16, 16)
            d32, _ = RR.render(scene, flat, 2.0, 16, 16, dtype=np.float32)
            yard = max(yard, float(np.abs(d32 - dref["d"])[dref["stable"]].max()))
    bound = min(CEILING, 8 * yard + 1e-6)
    for (e, c), dref in drefs.items():
        _check_depth(d4[e, c], dref, bound, ("rgbd env", e, c))
        _check_depth(d1[e, c], dref, bound, ("depth env", e, c))
        assert np.abs(d4[e, c] - d1[e, c])[dref["stable"]].max() <= bound, (e, c)
    env.close()
    plain.close()


def _png_rgb(path):
    """Pixels uint8 [H, W, 3] of an 8-bit RGB PNG with filter type 0 scanlines, by a zlib decode of its IDAT."""
    import struct

    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        (length,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        if kind == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
            assert (depth, colour) == (8, 2)
            size = (h, w)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + length
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(size[0], 1 + 3 * size[1])
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(size[0], size[1], 3)


def test_single_env_and_logs(tmp_path):
    from ballbot_gym.envs.ballbot_env import BBotSimulation

    sim = BBotSimulation(terrain_type="flat", depth_only=False, log_options={"cams": True, "dir": str(tmp_path)},
                         max_ep_steps=7)
    assert sim.depth_only is False and sim.observation_space["rgbd_0"].shape == (4, 64, 64)
    obs, _ = sim.reset(seed=2)
    assert obs["rgbd_0"].shape == (4, 64, 64) and obs["rgbd_0"].dtype == np.float32
    assert isinstance(obs["rgbd_1"], np.ndarray)
    assert sim.observation_space.contains(obs)
    done = False
    for _ in range(7):
        obs, _, done, _, _ = sim.step(np.zeros(3, np.float32))
        assert sim.observation_space.contains(obs)
    assert done
    assert len(sim.rgbd_hist_0) == 1 and sim.rgbd_hist_0[0].shape == (64, 64, 4)  # the frame of step 6
    ep = tmp_path / sim.log_dir / "rgbd_log_episode_0"
    for tag, hist in (("a", sim.rgbd_hist_0), ("b", sim.rgbd_hist_1)):
        assert (ep / "depth" / f"depth_{tag}_0.png").exists()
        frame = hist[0]
        assert np.array_equal(_png_rgb(ep / "rgb" / f"rbgd_{tag}_0.png"), (frame[:, :, :3] * 255).astype(np.uint8))
    assert np.array_equal(sim.rgbd_hist_0[0].transpose(2, 0, 1)[3], obs["rgbd_0"][3])  # held since step 6
    sim.close()
    plain = BBotSimulation(terrain_type="flat", env_config={"camera": {"disable_rgb": True}}, depth_only=False)
    assert plain.depth_only is True and plain.observation_space["rgbd_0"].shape == (1, 64, 64)  # the config wins
    plain.close()


def test_ppo_trains_on_rgbd():
    from ballbot_gym.envs import BallbotVecEnv
    from ballbot_rl.policies.mlp_policy import depth_cnn
    from ballbot_rl.training.ppo import BatchedPPO

    env = BallbotVecEnv(8, device="cuda:0", seed=5, disable_cameras=False,
                        env_config={"camera": {"height": 16, "width": 16, "disable_rgb": False}})
    m = BatchedPPO(env, n_steps=12, batch_size=48, n_epochs=1, learning_rate=1e-3, seed=10)
    ex = m.policy.features_extractor
    convs = [ex.extractors[k][0] for k in ("rgbd_0", "rgbd_1")]
    assert all(c.in_channels == 4 for c in convs) and ex.features_dim == 15 + 1 + 20 + 20
    before = [c.weight.detach().clone() for c in convs]
    m.learn(total_timesteps=8 * 12)
    assert tuple(m.buf.depth.shape) == (12, 8, 2, 4, 16, 16)
    assert float(m.buf.depth.min()) >= 0 and float(m.buf.depth.max()) <= 1.0
    assert len(torch.unique(m.buf.depth[:, :, :, :3])) > 4  # colour reached the buffer
    for c, w0 in zip(convs, before):
        assert torch.isfinite(c.weight).all() and not torch.equal(c.weight, w0)
    for key in ("train/loss", "train/value_loss", "train/policy_gradient_loss"):
        assert np.isfinite(m.logger.values[key]), key
    frozen = depth_cnn(1, 16, 16)
    with pytest.raises(ValueError, match="Channel mismatch: Encoder expects 1 channels"):
        BatchedPPO(env, n_steps=12, batch_size=48, n_epochs=1, seed=10, frozen_encoder=frozen)
    env.close()
