"""The per-episode log writer (ballbot_gym/utils/logging.py) on synthetic histories, and
bb_reward_terms' argument errors -- no GPU.

The file formats are the reference's (its ballbot_gym/utils/logging.py:9-117): 1-D float32
term_1.npy / term_2.npy overwritten per call, one "{seed}\\n" line appended to
terrain_seed_history per call on perlin terrains only, and 8-bit grey PNGs
rgbd_log_episode_{k}/depth/depth_{a,b}_{i}.png of (depth * 255).astype(uint8).  The PNGs
are decoded here by hand (IHDR + IDAT), so the check does not depend on an image library."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

from ballbot_gym.utils.logging import save_episode_logs, write_png


def _decode_png(path):
    """-> uint8 [H, W] (grey) or [H, W, 3] (RGB) of an 8-bit, non-interlaced PNG whose scanlines use filter 0."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (ln,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + ln]
        (crc,) = struct.unpack(">I", data[pos + 8 + ln:pos + 12 + ln])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        pos += 12 + ln
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, ctype, comp, flt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, flt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 1 if ctype == 0 else 3
    raw = zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT"))
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + w * ch)
    assert not rows[:, 0].any()  # filter type 0 on every scanline
    px = rows[:, 1:]
    return px.reshape(h, w) if ch == 1 else px.reshape(h, w, 3)


def _frames(rng, k, shape=(1, 6, 5)):
    return [rng.uniform(0.0, 1.0, shape).astype(np.float32) for _ in range(k)]


def test_term_files_are_1d_float32_and_overwritten(tmp_path):
    d = str(tmp_path)
    t1 = [np.float32(0.25), np.float32(-1.5), np.float32(3e-7)]
    t2 = [np.float32(-1e-4), np.float32(0.0), np.float32(-2.5e-5)]
    save_episode_logs(d, [], [], t1, t2, None, "flat", True, {"reward_terms": True, "cams": False}, 0, False)
    for name, want in (("term_1.npy", t1), ("term_2.npy", t2)):
        a = np.load(tmp_path / name)
        assert a.dtype == np.float32 and a.shape == (3,)
        assert a.tobytes() == np.asarray(want, np.float32).tobytes()
    # the next episode's call carries the longer history (never cleared) and overwrites the files
    t1b, t2b = t1 + [np.float32(7.0)], t2 + [np.float32(-8.0)]
    save_episode_logs(d, [], [], np.asarray(t1b), np.asarray(t2b), None, "flat", True, {"reward_terms": True}, 1, False)
    assert np.load(tmp_path / "term_1.npy").tolist() == [float(x) for x in t1b]
    assert np.load(tmp_path / "term_2.npy").tolist() == [float(x) for x in t2b]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["term_1.npy", "term_2.npy"]


def test_reward_terms_off_or_empty_writes_no_term_files(tmp_path):
    save_episode_logs(str(tmp_path), [], [], [1.0], [2.0], None, "flat", True, {"reward_terms": False}, 0, False)
    save_episode_logs(str(tmp_path), [], [], [], [], None, "flat", True, {"reward_terms": True}, 0, False)
    assert list(tmp_path.iterdir()) == []


def test_seed_history_grows_by_one_line_per_call_on_perlin_only(tmp_path):
    d = str(tmp_path)
    opts = {"reward_terms": False, "cams": False}
    for k, seed in enumerate((4711, 3, 9999)):
        save_episode_logs(d, [], [], [], [], seed, "perlin", True, opts, k, False)
        assert (tmp_path / "terrain_seed_history").read_text() == "".join(f"{s}\n" for s in (4711, 3, 9999)[:k + 1])
    save_episode_logs(d, [], [], [], [], 17, "flat", True, opts, 3, False)     # not perlin
    save_episode_logs(d, [], [], [], [], None, "perlin", True, opts, 4, False)  # no seed
    assert (tmp_path / "terrain_seed_history").read_text() == "4711\n3\n9999\n"


def test_depth_pngs_names_count_and_pixels(tmp_path):
    rng = np.random.default_rng(5)
    h0, h1 = _frames(rng, 3), _frames(rng, 3)
    h0[0][0, 0, :3] = (0.0, 1.0, 0.999)  # the ends of the range and a value that truncates to 254
    save_episode_logs(str(tmp_path), h0, h1, [], [], None, "flat", True, {"cams": True}, 7, False)
    ep = tmp_path / "rgbd_log_episode_7"
    assert sorted(p.name for p in ep.iterdir()) == ["depth", "rgb"]
    assert list((ep / "rgb").iterdir()) == []  # created as the reference does, empty in depth-only mode
    assert sorted(p.name for p in (ep / "depth").iterdir()) == sorted(
        f"depth_{c}_{i}.png" for c in "ab" for i in range(3))
    for c, hist in (("a", h0), ("b", h1)):
        for i, f in enumerate(hist):
            got = _decode_png(ep / "depth" / f"depth_{c}_{i}.png")
            want = (f[0] * 255).astype("uint8")
            assert got.shape == (6, 5) and got.dtype == np.uint8
            assert np.array_equal(got, want), (c, i)
    assert _decode_png(ep / "depth" / "depth_a_0.png")[0, :3].tolist() == [0, 255, 254]


def test_depth_frames_in_the_reference_layouts(tmp_path):
    """[H, W, 1] (the reference's depth-only frames) and [H, W] decode to the same pixels."""
    rng = np.random.default_rng(6)
    f = rng.uniform(0, 1, (4, 7)).astype(np.float32)
    save_episode_logs(str(tmp_path), [f[:, :, None]], [f], [], [], None, "flat", True, {"cams": True}, 0, False)
    want = (f * 255).astype("uint8")
    for c in "ab":
        assert np.array_equal(_decode_png(tmp_path / "rgbd_log_episode_0" / "depth" / f"depth_{c}_0.png"), want)


def test_cams_off_or_no_frames_writes_no_episode_directory(tmp_path):
    rng = np.random.default_rng(7)
    save_episode_logs(str(tmp_path), _frames(rng, 2), _frames(rng, 2), [], [], None, "flat", True, {"cams": False}, 0,
                      False)
    save_episode_logs(str(tmp_path), [], [], [], [], None, "flat", True, {"cams": True}, 0, False)
    assert list(tmp_path.iterdir()) == []


def test_eval_env_writes_nothing(tmp_path):
    rng = np.random.default_rng(8)
    save_episode_logs(str(tmp_path), _frames(rng, 2), _frames(rng, 2), [1.0, 2.0], [3.0, 4.0], 12, "perlin", True,
                      {"cams": True, "reward_terms": True}, 0, True)
    assert list(tmp_path.iterdir()) == []


def test_write_png_round_trips_and_rejects_other_pixels(tmp_path):
    rng = np.random.default_rng(9)
    grey = rng.integers(0, 256, (3, 9), dtype=np.uint8)
    rgb = rng.integers(0, 256, (5, 2, 3), dtype=np.uint8)
    write_png(str(tmp_path / "g.png"), grey)
    write_png(str(tmp_path / "c.png"), rgb)
    assert np.array_equal(_decode_png(tmp_path / "g.png"), grey)
    assert np.array_equal(_decode_png(tmp_path / "c.png"), rgb)
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "x.png"), grey.astype(np.float32))


def test_png_decodes_with_pil_too(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    px = np.random.default_rng(10).integers(0, 256, (8, 8), dtype=np.uint8)
    write_png(str(tmp_path / "g.png"), px)
    with Image.open(tmp_path / "g.png") as im:
        assert im.mode == "L" and np.array_equal(np.asarray(im), px)


def test_reward_terms_argument_errors_without_gpu():
    """bb_reward_terms rejects bad arguments before any HIP call (the header's error contract):
    status < 0 and its own bb_last_error text for NULL pointers, k < 1 and a NULL handle."""
    from ballbot_gym import _native

    _native.build()  # no-op when up to date
    L = _native.lib()
    for args, msg in (((None, None, None, 1, None, 1, None, None), "bb_reward_terms: NULL argument"),
                      ((None, 16, 16, 1, 16, 1, None, None), "bb_reward_terms: NULL argument"),
                      ((None, 16, 16, 0, 16, 1, 16, None), "bb_reward_terms: k_steps must be >= 1"),
                      ((None, 16, 16, 1, 16, -1, 16, None), "bb_reward_terms: terms_rows must be >= 0"),
                      ((None, 16, 16, 1, 16, 1, 16, None), "bb_reward_terms: NULL handle")):
        assert L.bb_reward_terms(*args) < 0
        assert msg in _native.last_error(), (msg, _native.last_error())
    assert "bb_reward_terms" in _native.EXPORTS and _native.ABI_VERSION >= 20
    names = [f for f, _ in _native.RolloutArgs._fields_]
    assert names[-2:] == ["buf_terminal_obs", "buf_flags"]
    assert C.sizeof(_native.RolloutArgs) == _native.RolloutArgs.buf_flags.offset + C.sizeof(C.c_void_p)
