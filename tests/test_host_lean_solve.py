"""The lean forms of the FUSE kernels' factorisation and sweeps, on the host (CPU only).

tests/hostcheck/lean_solve_check.cpp is a stand-alone program that emulates the sixteen lanes of a team: chol_rows
with the floors formed ahead of the columns and the lane's own inverse pivot (csrc/bb_team16.h: kLeanFloor, kLeanMax,
kLeanDiag), chol_solve_rows with the own-pivot forward and backward sweeps, the transpose's
stores from one lane base (kLeanLtr, ltr_lane_slot against ltr_slot),
each against the text it replaces, bit for bit in float and double (its header lists the inputs).  Built twice: as
the other host checks are, and with the address and undefined-behaviour sanitizers on the host code.  The same code
runs on the GPU in tests/test_gpu_lean_solve.py.
"""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
SRC = ROOT / "tests" / "hostcheck" / "lean_solve_check.cpp"
BUILD = ROOT / "tests" / "_build"


@pytest.mark.parametrize("name,flags", [
    ("lean_solve_check", ["-O2"]),
    ("lean_solve_check_san", ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                              "-fno-sanitize-recover=all"]),
])
def test_lean_forms_equal_parent_forms_on_host(name, flags):
    BUILD.mkdir(parents=True, exist_ok=True)
    exe = BUILD / name
    subprocess.run(["hipcc", *flags, "-ffp-contract=off", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", "-o", str(exe),
                    str(SRC)],
                   check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
