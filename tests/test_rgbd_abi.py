"""The RGB-D cameras' C-ABI without a GPU: the built gfx950 library exports bb_render_rgbd, its unit
bb_rgbd.hip is one of the HIP sources, the ABI version stays 21 (the addition is purely additive:
callers detect it by symbol), argument errors come back < 0 with their message before anything is
launched, and the observation space has the (4, H, W) camera boxes."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def native():
    from ballbot_gym import _native

    _native.build()  # no-op when up to date; hipcc cross-compiles for gfx950 without a GPU
    return _native


def test_exports_and_version(native):
    lib = C.CDLL(str(native.LIB_PATH))
    assert hasattr(lib, "bb_render_rgbd")
    assert "bb_render_rgbd" in native.EXPORTS
    assert "bb_rgbd.hip" in native.HIP_SOURCES
    assert native.lib().bb_abi_version() == 21 == native.ABI_VERSION


def test_argument_errors_carry_their_message(native):
    L = native.lib()
    # the argument checks come before the handle is read: any non-NULL addresses do
    handle, image = C.create_string_buffer(4096), C.create_string_buffer(64)
    h, img = C.cast(handle, C.c_void_p), C.cast(image, C.c_void_p)
    assert L.bb_render_rgbd(None, img, None, None, 8, 8, 6, 1, None) < 0
    assert "bb_render_rgbd: NULL argument" in native.last_error()
    assert L.bb_render_rgbd(h, None, None, None, 8, 8, 6, 1, None) < 0
    assert "bb_render_rgbd: NULL argument" in native.last_error()
    for H, W in ((0, 8), (8, 0), (-1, 8), (8, 1025)):
        assert L.bb_render_rgbd(h, img, None, None, H, W, 6, 1, None) < 0
        assert f"bb_render_rgbd: image size {H}x{W} out of range" in native.last_error()
    for every in (0, -3):
        assert L.bb_render_rgbd(h, img, None, None, 8, 8, every, 1, None) < 0
        assert f"frame interval must be >= 1 step (got {every})" in native.last_error()
    assert image.raw == b"\0" * 64


def test_observation_space_has_four_channels():
    from ballbot_gym import spaces

    sp = spaces.observation_space({"h": 8, "w": 8}, 4, False)
    assert sp["rgbd_0"].shape == (4, 8, 8) and sp["rgbd_1"].shape == (4, 8, 8)
    assert sp.contains(sp.sample())
