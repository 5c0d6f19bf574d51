"""The forward's twin forms and once-per-launch model terms on the host (CPU only).

tests/hostcheck/prephase_check.cpp is a stand-alone program over the product's templates
(csrc/bb_physics.h): the half-selected quaternion step, kinematics and bias chain, and every field of
ModelOnce, against the serial forms, bit for bit in float and double, on seeded states with the edge
cases its header lists.  The same templates run on the GPU in tests/test_gpu_prephase.py.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
SRC = ROOT / "tests" / "hostcheck" / "prephase_check.cpp"
EXE = ROOT / "tests" / "_build" / "prephase_check"


def test_twin_and_once_forms_equal_serial_on_host():
    EXE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", "-o", str(EXE), str(SRC)],
                   check=True, capture_output=True)
    r = subprocess.run([str(EXE)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
