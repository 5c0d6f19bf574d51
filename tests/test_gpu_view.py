"""GPU world-view renderer (csrc/bb_view.hip, bb_render_view) against tests/view_ref.py, the fp64
reference of the image's definition, plus its buffers, its public surface and the
trainer's video recorder.

Cases (view_ref.CASES): the tilt, edge and lift pose families of render_ref, 8 envs pinned
round-robin over a 4-slot bank (flat, hills seed 7 at size_z 2, hills seed 11 at size_z 0.5, GPU
perlin); image sizes 24x32, 17x23, 33x47 (no multiples of the 8x8 tile), 5x3 and 1x1; fp64 and fp32
state (the fp32 reference reads the state back); the default camera and three close-ups of the
drive.  The kernel renders into the test's own sentinel-filled buffers with guard regions on both
sides, at byte offsets that are no multiple of 4, so every packed store's alignment case runs.

Per image: a pixel is *stable* if the reference's five samples (centre, +-3e-5 in normalised image
coordinates along x and y) agree in surface id, colour class and hit triangle and both second
differences of the depth are <= 1e-6 (test_view_ref.py asserts that >= 95 % of every image is).
Every stable pixel has the reference's surface id, without exception, and every channel within
+-1 count; every unstable pixel shows an id of one of the five samples and channels within their
min / max +- 1.  The +-1: float32 moves 255 c by about 0.03 at most (the sphere's normal carries
1e-5 / 0.09), so only a value at a rounding boundary of int(255 c + 0.5) can differ, and by one.

Worst count difference on stable pixels, and how many stable pixels differ at all, per case
(8 images each; single run):

  tilt 24x32 fp64 default   0   0 of  6091      lift 24x32 fp32 close150  1   1 of  6108
  edge 17x23 fp32 default   1   2 of  3123      edge 17x23 fp64 close270  1   1 of  3095
  lift 33x47 fp64 default   1   2 of 12265      tilt  5x3  fp64 default   0   0 of   120
  tilt 33x47 fp32 close30   1   2 of 12329      edge  5x3  fp32 close30   0   0 of   120
  edge 24x32 fp64 close150  1   1 of  6123      tilt  1x1  fp32 default   0   0 of     8
  lift 17x23 fp64 close270  0   0 of  3113      lift  1x1  fp64 close270  0   0 of     8

No stable pixel shows another surface than the reference, and no unstable pixel leaves its five
samples.

The issue's tracking check ("after set_state moves the robot by (1, 2, 0) on flat ground the ids
image is unchanged") cannot hold as written: the field ends at +-5 m, its far edge is in view as the
horizon, and it moves when the robot does.  The test below asks for the rest: every robot pixel
and the whole lower half of the image unchanged, and above it only ground turned to background.

Parity against MuJoCo's OpenGL image itself is unpinned (MuJoCo is unavailable).
"""
import ctypes as C

import numpy as np
import pytest

import render_ref as RR
import view_ref as VR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD_RGB, GUARD_IDS = 4099, 4097  # odd: the image's first byte is not dword aligned
SENT = 0x5A
BACKGROUND = (140, 179, 230)  # int(255 (0.55, 0.70, 0.90) + 0.5)


def _env(n, terrain, seed=0, **kw):
    from ballbot_gym.envs import BallbotVecEnv

    return BallbotVecEnv(n, device="cuda:0", terrain_config=terrain, auto_reset=False, seed=seed, **kw)


@pytest.fixture(scope="module")
def fields():
    return [(h, z) for h, z in zip(RR.bank() + [RR.perlin_field()], RR.SIZE_Z)]


def _bank_env(fields, precision="fp64", n=VR.N_ENVS, **kw):
    """An env over the 4-slot bank, env e pinned to slot e % 4."""
    from ballbot_gym import _native as N
    from ballbot_gym.envs.config import np_random

    env = _env(n, {"type": "perlin", "config": {}}, terrain_slots=len(fields), precision=precision, **kw)
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


def _cfg(H, W, camera):
    from ballbot_gym import _native as N

    return N.ViewCfg(H, W, camera["fovy"], camera["azimuth"], camera["elevation"], camera["distance"],
                     (C.c_float * 3)(*camera["lookat_offset"]))


def _render_raw(env, env_ids, H, W, camera=VR.DEFAULT_CAM, want_ids=True):
    """bb_render_view on the env's handle into sentinel-filled buffers of the test's own with a guard
    region on both sides -> (rgb uint8 [k, H, W, 3], ids int8 [k, H, W]) on the host."""
    from ballbot_gym import _native as N

    k = len(env_ids)
    nrgb, nid = k * H * W * 3, k * H * W
    rgb = torch.full((GUARD_RGB + nrgb + GUARD_RGB,), SENT, dtype=torch.uint8, device=env.device)
    ids = torch.full((GUARD_IDS + nid + GUARD_IDS,), SENT, dtype=torch.int8, device=env.device)
    e = torch.as_tensor(np.asarray(env_ids, np.int32)).to(env.device)
    cfg = _cfg(H, W, camera)
    N.check(N.lib().bb_render_view(env._h, C.c_void_p(e.data_ptr()) if k else None, k, C.byref(cfg),
                                   C.c_void_p(rgb[GUARD_RGB:].data_ptr()),
                                   C.c_void_p(ids[GUARD_IDS:].data_ptr()) if want_ids else None, None),
            "bb_render_view")
    torch.cuda.synchronize()
    r, i = rgb.cpu().numpy(), ids.cpu().numpy()
    for a, g, m in ((r, GUARD_RGB, nrgb), (i, GUARD_IDS, nid)):
        assert (a[:g] == SENT).all() and (a[g + m:] == SENT).all(), "guard region written"
    if not want_ids:
        assert (i == SENT).all()
    return r[GUARD_RGB:GUARD_RGB + nrgb].reshape(k, H, W, 3), i[GUARD_IDS:GUARD_IDS + nid].reshape(k, H, W)


def _check_image(rgb, ids, ref, where):
    """The per-image assertions -> (worst count difference on stable pixels, how many differ)."""
    st = ref["stable"]
    assert (ids[st] == ref["ids"][st]).all(), (where, "stable pixel id", np.argwhere(st & (ids != ref["ids"]))[:4])
    diff = np.abs(rgb.astype(np.int16) - ref["rgb"].astype(np.int16)).max(-1)
    worst = int(diff[st].max()) if st.any() else 0
    assert worst <= 1, (where, "stable pixel colour", np.argwhere(st & (diff > 1))[:4], worst)
    un = ~st
    assert (ids[None] == ref["ids5"]).any(0)[un].all(), (where, "unstable pixel: id of none of its five samples")
    out = np.maximum(ref["lo"] - rgb.astype(np.int16), rgb.astype(np.int16) - ref["hi"]).max(-1)
    assert (out[un] <= 1).all(), (where, "unstable pixel outside its five samples", int(out[un].max()))
    return worst, int((diff[st] > 0).sum())


@pytest.mark.parametrize("case", VR.CASES, ids=lambda c: "-".join(map(str, c)))
def test_view_matches_reference(oracle, fields, case):
    family, H, W, precision, camera = case
    cam = VR.CAMERAS[camera]
    Q = RR.poses(family, fields, oracle.reset_state(0.01)[0], n=VR.N_ENVS)
    env = _bank_env(fields, precision)
    env.set_state(Q, np.zeros((VR.N_ENVS, 15)), None, np.zeros(VR.N_ENVS, np.int32))
    if precision == "fp32":  # the reference gets the state the kernel holds
        Q = env.get_state()[0]
        assert np.array_equal(Q, Q.astype(np.float32).astype(np.float64))
    rgb, ids = _render_raw(env, list(range(VR.N_ENVS)), H, W, cam)
    env.close()
    worst = differ = stable = 0
    for e, ref in enumerate(VR.references(oracle, fields, Q, H, W, cam)):
        assert ref["stable"].mean() >= 0.95 or H * W < 20, (case, e)
        w, n = _check_image(rgb[e], ids[e], ref, (case, e))
        worst, differ, stable = max(worst, w), differ + n, stable + int(ref["stable"].sum())
    print(f"VIEW {'-'.join(map(str, case)):32s} worst {worst} count, {differ} of {stable} stable pixels differ")


def test_buffers_order_duplicates_and_bad_ids(oracle, fields):
    from ballbot_gym import _native as N

    Q = RR.poses("tilt", fields, oracle.reset_state(0.01)[0], n=VR.N_ENVS)
    env = _bank_env(fields)
    env.set_state(Q, np.zeros((VR.N_ENVS, 15)), None, np.zeros(VR.N_ENVS, np.int32))
    H, W = 17, 23
    cam = VR.CAMERAS["close30"]
    every, every_ids = _render_raw(env, list(range(VR.N_ENVS)), H, W, cam)
    assert len({every[e].tobytes() for e in range(VR.N_ENVS)}) == VR.N_ENVS  # every env its own picture
    rgb, ids = _render_raw(env, [5, 0, 5], H, W, cam)
    assert np.array_equal(rgb[0], every[5]) and np.array_equal(rgb[1], every[0]) and np.array_equal(rgb[2], rgb[0])
    assert np.array_equal(ids[0], every_ids[5]) and np.array_equal(ids[1], every_ids[0]) and np.array_equal(ids[2], ids[0])
    rgb, ids = _render_raw(env, [VR.N_ENVS, 3, -1, 2 ** 31 - 1], H, W, cam)  # out of range: background only
    for v in (0, 2, 3):
        assert (rgb[v] == BACKGROUND).all() and (ids[v] == 0).all(), v
    assert np.array_equal(rgb[1], every[3]) and np.array_equal(ids[1], every_ids[3])
    only_rgb, _ = _render_raw(env, [5, 0, 5], H, W, cam, want_ids=False)  # ids_dev may be NULL
    assert np.array_equal(only_rgb[0], every[5])
    rgb, ids = _render_raw(env, [], H, W, cam)  # n_views = 0: a no-op (the guards cover the whole buffer)
    assert rgb.size == 0 and ids.size == 0
    # argument errors: status < 0 and a message, nothing launched
    buf = torch.zeros(64, dtype=torch.uint8, device=env.device)
    e = torch.zeros(1, dtype=torch.int32, device=env.device)
    L, p = N.lib(), C.c_void_p
    for cfg, k, out, msg in ((_cfg(0, 4, cam), 1, p(buf.data_ptr()), "image size"), (_cfg(4, -1, cam), 1, p(buf.data_ptr()), "image size"),
                             (_cfg(2, 2, cam), -1, p(buf.data_ptr()), "n_views"), (_cfg(2, 2, cam), 1, None, "NULL")):
        assert L.bb_render_view(env._h, p(e.data_ptr()), k, C.byref(cfg), out, None, None) < 0
        assert msg in N.last_error(), (msg, N.last_error())
    torch.cuda.synchronize()
    assert (buf == 0).all()
    env.close()


def test_render_view_has_no_side_effects(fields):
    """20 steps with render_view calls interleaved: the state, obs, rewards and the depth-camera
    buffer are bit-equal to 20 steps without them."""
    rng = np.random.default_rng(11)
    acts = torch.as_tensor(rng.uniform(-1, 1, (20, VR.N_ENVS, 3)).astype(np.float32)).to("cuda:0")
    runs = []
    for with_views in (False, True):
        env = _bank_env(fields, disable_cameras=False)
        trace = []
        for t in range(20):
            if with_views:
                env.render_view([t % VR.N_ENVS, 0], 17 + t, 23, azimuth=10.0 * t)
            obs, rew, term, trunc, info = env.step(acts[t])
            if with_views and t % 3 == 0:
                env.render_view(list(range(VR.N_ENVS)), 9, 11)
            trace.append((obs.clone(), rew.clone(), term.clone(), env.depth.clone(), env.rel_ts.clone()))
        runs.append((trace, env.get_state()))
        env.close()
    (ta, sa), (tb, sb) = runs
    for a, b in zip(ta, tb):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)


def test_single_env_render_tracks_the_robot():
    from ballbot_gym.envs.ballbot_env import BBotSimulation

    sim = BBotSimulation(terrain_type="flat", disable_cameras=True)
    sim.reset(seed=3)
    frame = sim.render()
    assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8 and frame.shape == (640, 480, 3)
    env = sim._env
    ids = torch.zeros(1, 640, 480, dtype=torch.int8, device=env.device)
    rgb = env.render_view(ids_out=ids)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (1, 640, 480, 3)
    assert np.array_equal(rgb[0].cpu().numpy(), frame)
    ids = ids[0].cpu().numpy()
    assert ids[320, 240] == VR.TOWER  # the camera looks at the tower, 0.2 m above the base origin
    assert set(np.unique(ids)) >= {VR.NONE, VR.GROUND, VR.BALL, VR.TOWER}
    assert (frame[ids == 0] == BACKGROUND).all()
    # the camera tracks the base: move the robot by (1, 2, 0) on flat ground and the picture of the robot
    # and of the ground around it stays.  The field ends at +-5 m, so its far edge (the horizon, in the
    # image's upper half: 10 to 14 degrees below the horizontal, the camera looks 20 degrees down)
    # moves; nothing else may, and there only ground and background trade places.
    small = torch.zeros(1, 96, 72, dtype=torch.int8, device=env.device)
    env.render_view(None, 96, 72, ids_out=small)
    before = small[0].cpu().numpy().copy()
    q, v, w, s = env.get_state()
    q[:, 0:3] += [1.0, 2.0, 0.0]
    q[:, 10:13] += [1.0, 2.0, 0.0]
    env.set_state(q, v, w, s)
    env.render_view(None, 96, 72, ids_out=small)
    after = small[0].cpu().numpy()
    assert len(np.unique(before)) >= 4 and (before >= 2).sum() > 100
    assert np.array_equal(after >= 2, before >= 2) and np.array_equal(after[before >= 2], before[before >= 2])
    assert np.array_equal(after[48:], before[48:]) and (before[48:] == VR.GROUND).any()
    moved = after != before
    # 2 m nearer to the far edge: it sinks in the image, ground gives way to background
    assert 0 < moved.sum() < 0.1 * moved.size and (before[moved] == VR.GROUND).all() and (after[moved] == VR.NONE).all()
    sim.close()


def test_vec_env_render_mode():
    from ballbot_gym.envs import BallbotVecEnv

    assert BallbotVecEnv.render_mode is None
    with pytest.raises(ValueError):
        BallbotVecEnv(2, device="cuda:0", render_mode="human")
    env = BallbotVecEnv(2, device="cuda:0", render_mode="rgb_array")
    frame = env.render()
    assert frame.dtype == np.uint8 and frame.shape == (640, 480, 3)
    assert np.array_equal(frame, env.render_view([0])[0].cpu().numpy())
    out = torch.zeros(2, 5, 7, 3, dtype=torch.uint8, device=env.device)
    assert env.render_view(torch.tensor([1, 0], device=env.device), 5, 7, out=out) is out
    with pytest.raises(ValueError):
        env.render_view([0], 5, 7, out=out)  # the wrong shape for one view
    env.close()
    env = BallbotVecEnv(2, device="cuda:0")
    with pytest.raises(RuntimeError):
        env.render()
    env.close()


class _ZeroPolicy:
    def predict(self, obs, deterministic=False):
        return torch.zeros(obs.shape[0], 3, device=obs.device)


def test_video_recorder_writes_the_device_stack(tmp_path):
    from ballbot_rl.training.callbacks import VideoRecorder, read_apng

    flat = {"type": "flat", "config": {}}
    eval_env = _env(64, flat, seed=5, stream_seeds=[5 + i for i in range(64)])
    words, seeds = eval_env.terrain_rng()
    video_env = _env(1, flat, seed=77, max_ep_steps=100)
    video_env.auto_reset = True
    rec = VideoRecorder(video_env, tmp_path / "videos", video_length=40, frame_skip=8, size=(48, 64), async_write=True)
    path = rec.record(_ZeroPolicy())
    stack = rec.stack.cpu().numpy()
    rec.close()
    frames = read_apng(path)
    assert path.name == "best_model_episode_1.png"
    assert frames.shape[1:] == (48, 64, 3) and 1 <= frames.shape[0] <= 6
    assert np.array_equal(frames, stack[:frames.shape[0]])
    assert (frames[0] != np.array(BACKGROUND)).any() and (stack[frames.shape[0]:] == 0).all()
    w2, s2 = eval_env.terrain_rng()
    assert np.array_equal(words, w2) and np.array_equal(seeds, s2)  # the eval env's terrain stream is untouched
    eval_env.close()


def test_train_main_records_videos(tmp_path):
    from ballbot_rl.training.callbacks import read_apng
    from ballbot_rl.training.train import main

    cfg = {"algo": {"batch_sz": 2048, "clip_range": 0.015, "ent_coef": 0.001, "learning_rate": -1, "n_epochs": 2,
                    "n_steps": 8, "name": "ppo", "normalize_advantage": False, "target_kl": 0.3, "vf_coef": 2.0,
                    "weight_decay": 0.01},
           "env": {"max_allowed_tilt": 20, "max_ep_steps": 100, "max_wheel_velocity": 10.0},
           "evaluation": {"freq": 8, "n_episodes": 4, "num_envs": 64}, "hidden_sz": 64, "num_envs": 512, "seed": 10,
           "problem": {"reward": {"type": "directional", "config": {"target_direction": [0.0, 1.0]}},
                       "terrain": {"type": "flat", "config": {}}}, "total_timesteps": 512 * 8 * 2,
           "visualization": {"record_videos": True, "video_freq": "every_eval", "video_length": 40,
                             "video_frame_skip": 8, "video_size": [48, 64]}}
    m = main(cfg, 10, out=str(tmp_path / "run"))
    videos = sorted((m.out_path / "videos").glob("*.png"))
    assert [v.name for v in videos] == ["eval_episode_1.png", "eval_episode_2.png"]
    for v in videos:
        f = read_apng(v)
        assert f.shape[1:] == (48, 64, 3) and f.shape[0] >= 1
