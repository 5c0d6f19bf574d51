"""The world-view renderer's C-ABI (ABI 21) without a GPU: the built gfx950 library exports
bb_render_view and bb_default_view, reports ABI 21, fills the default view (640 x 480, fovy 45,
azimuth 90, elevation -20, distance 2.5, look-at offset (0, 0, 0.2)), the ctypes mirror of
bb_view_cfg has the C compiler's layout, and a NULL handle is an error with a message."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def native():
    from ballbot_gym import _native

    _native.build()  # no-op when up to date; hipcc cross-compiles for gfx950 without a GPU
    return _native


def test_exports_and_version(native):
    lib = C.CDLL(str(native.LIB_PATH))
    assert hasattr(lib, "bb_render_view") and hasattr(lib, "bb_default_view")
    assert native.lib().bb_abi_version() == 21 == native.ABI_VERSION
    assert "bb_view.hip" in native.HIP_SOURCES


def test_default_view(native):
    c = native.ViewCfg()
    native.lib().bb_default_view(C.byref(c))
    assert (c.height, c.width) == (640, 480)
    assert (c.fovy_deg, c.azimuth_deg, c.elevation_deg, c.distance) == (45.0, 90.0, -20.0, 2.5)
    assert tuple(c.lookat_offset) == (0.0, 0.0, pytest.approx(0.2, rel=1e-7))


def test_null_arguments_are_errors(native):
    L = native.lib()
    c = native.ViewCfg()
    L.bb_default_view(C.byref(c))
    assert L.bb_render_view(None, None, 1, C.byref(c), None, None, None) < 0
    assert "bb_render_view: NULL argument" in native.last_error()


def test_view_cfg_layout(tmp_path, native):
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ballbot_mi355x.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(bb_view_cfg));']
    for field, _ in native.ViewCfg._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof(bb_view_cfg, {field}));')
    lines += ["return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                       text=True).stdout.strip().split("\n"))
    assert int(got["size"]) == C.sizeof(native.ViewCfg)
    for field, _ in native.ViewCfg._fields_:
        assert int(got[field]) == getattr(native.ViewCfg, field).offset, field
