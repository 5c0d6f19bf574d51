"""The trainer's video recorder without a GPU (ballbot_rl/training/callbacks.py): the animated
PNG round trip, the frame schedule on a fake env, and train's reading of the reference's
`visualization` section."""
import numpy as np
import pytest
import torch

from fake_env import FakeEnv


def test_apng_round_trip_bit_for_bit(tmp_path):
    from ballbot_rl.training.callbacks import read_apng, write_apng

    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (6, 13, 7, 3), dtype=np.uint8)
    frames[3] = frames[2]  # two identical frames in a row stay two frames
    frames[5, 2:5] = frames[4, 2:5]
    write_apng(tmp_path / "a.png", frames)
    got = read_apng(tmp_path / "a.png")
    assert got.dtype == np.uint8 and got.shape == frames.shape and np.array_equal(got, frames)
    write_apng(tmp_path / "one.png", frames[:1])
    assert np.array_equal(read_apng(tmp_path / "one.png"), frames[:1])
    with pytest.raises(ValueError):
        write_apng(tmp_path / "bad.png", frames[..., :2])


class _VideoFake(FakeEnv):
    """One env; render_view paints the number of steps taken since the reset into the frame."""

    def __init__(self, ep_len):
        super().__init__(1, ep_len=ep_len)
        self.steps = 0
        self.rendered = []

    def reset(self):
        self.steps = 0
        self.t[:] = 0
        return super().reset()

    def step(self, a):
        self.steps += 1
        return super().step(a)

    def render_view(self, env_ids=None, height=640, width=480, *, out=None, **kw):
        assert env_ids is None and out.shape == (1, height, width, 3) and out.dtype == torch.uint8
        out.fill_(self.steps)
        self.rendered.append(self.steps)
        return out


class _Policy:
    def predict(self, obs, deterministic=False):
        assert deterministic
        return torch.zeros(obs.shape[0], 3)


@pytest.mark.parametrize("ep_len,video_length,frame_skip,want", [
    (100, 40, 8, [0, 8, 16, 24, 32, 40]),   # stops at video_length; a frame after its last step
    (20, 40, 8, [0, 8, 16]),                 # stops at done (step 20): the reset state is not filmed
    (16, 40, 8, [0, 8]),                     # done at a frame step: that frame would show the next episode
    (100, 5, 17, [0]),                       # shorter than one frame interval
    (100, 34, 17, [0, 17, 34]),
])
def test_frame_schedule(tmp_path, ep_len, video_length, frame_skip, want):
    from ballbot_rl.training.callbacks import VideoRecorder, read_apng

    env = _VideoFake(ep_len)
    rec = VideoRecorder(env, tmp_path / "videos", video_length=video_length, frame_skip=frame_skip, size=(6, 4),
                        async_write=True)
    path = rec.record(_Policy())
    rec.close()
    assert env.rendered == want
    assert want == VideoRecorder.frame_steps(min(video_length, ep_len - 1), frame_skip)
    assert path == tmp_path / "videos" / "best_model_episode_1.png"
    frames = read_apng(path)
    assert frames.shape == (len(want), 6, 4, 3) and [int(f[0, 0, 0]) for f in frames] == want
    assert np.array_equal(frames, rec.stack[:len(want)].numpy())


def test_recorder_numbers_its_files_and_needs_one_env(tmp_path):
    from ballbot_rl.training.callbacks import VideoRecorder

    with pytest.raises(ValueError):
        VideoRecorder(FakeEnv(2), tmp_path)
    rec = VideoRecorder(_VideoFake(50), tmp_path, video_length=10, frame_skip=4, size=(3, 5), async_write=False,
                        name_prefix="eval")
    assert [rec(_Policy()).name for _ in range(3)] == [f"eval_episode_{k}.png" for k in (1, 2, 3)]
    rec.close()
    assert all(p.exists() for p in rec.paths)


def test_visualization_section_parsing():
    from ballbot_rl.training.callbacks import video_options

    assert video_options({}) is None  # no section: nothing is recorded
    assert video_options({"visualization": {}}) is None
    assert video_options({"visualization": {"record_videos": False, "video_freq": "every_eval"}}) is None
    o = video_options({"visualization": {"record_videos": True}, "env": {"max_ep_steps": 300}})
    assert o == {"video_freq": "on_new_best", "episodes": 1, "async_write": True, "video_length": 300, "frame_skip": 17,
                 "size": (640, 480), "name_prefix": "best_model"}
    o = video_options({"visualization": {"record_videos": True, "video_freq": 5, "video_episodes": 2,
                                         "async_video_recording": False, "video_length": 40, "video_frame_skip": 8,
                                         "video_size": [48, 64]}})
    assert o == {"video_freq": 5, "episodes": 2, "async_write": False, "video_length": 40, "frame_skip": 8,
                 "size": (48, 64), "name_prefix": "eval"}
    for bad in ("sometimes", 0, True):
        with pytest.raises(ValueError):
            video_options({"visualization": {"record_videos": True, "video_freq": bad}})


def test_eval_callback_hooks():
    from ballbot_rl.training.callbacks import EvalCallback, EveryNth

    cb = EvalCallback(None)
    assert cb.callback_on_new_best is None and cb.callback_after_eval is None  # the default: as it was
    seen = []
    nth = EveryNth(seen.append, 3)
    for k in range(7):
        nth(k)
    assert seen == [2, 5]
