"""The ball-terrain pass's cell window on the host (CPU only).

tests/hostcheck/prism_window_check.cpp is a stand-alone program over the product's prism_window
(csrc/bb_physics.h), the window t16::collide_team walks, against brute force over the whole sub-grid
under the ball's AABB, in float and double: no prism that passes collide_ground's z cull and coarse
test lies outside the window (zero misses is the condition), the window is a subset of the AABB's, it
is the AABB's where no bound applies, and the contact list over it is the list over the AABB's
sub-grid bit for bit.  Its header lists the fields and the seeded cases.  The same function runs on
the GPU in tests/test_gpu_collide_window.py and tests/test_gpu_prism_window_step.py.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
SRC = ROOT / "tests" / "hostcheck" / "prism_window_check.cpp"
EXE = ROOT / "tests" / "_build" / "prism_window_check"


def test_prism_window_holds_every_passing_prism_on_host():
    EXE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", "-o", str(EXE), str(SRC)],
                   check=True, capture_output=True)
    r = subprocess.run([str(EXE)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
