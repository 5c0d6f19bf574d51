"""Where the fast kernels' solve finds its operands, on the host (CPU only).

tests/hostcheck/hrow_check.cpp is a stand-alone program over the product's layout functions (csrc/bb_solve.h:
hsq_row_off, grec_off, ws_at, the constants beside them) and the addressing of csrc/bb_team16.h's mass_rows_team,
ground_setup and ground_get: the dense mass matrix stored by rows against the packed triangle through hidx, the
one-record ball-terrain contact against ground_contact's outputs and the two-region form, and the three team sums
behind the sweeps in the interleaved order against the serial one through the fallback branch, bit for bit in float
and double (its header lists the inputs).  The same code runs on the GPU in tests/test_gpu_hrow.py.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
SRC = ROOT / "tests" / "hostcheck" / "hrow_check.cpp"
EXE = ROOT / "tests" / "_build" / "hrow_check"


def test_rows_records_and_sums_equal_parent_forms_on_host():
    EXE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", "-o", str(EXE), str(SRC)],
                   check=True, capture_output=True)
    r = subprocess.run([str(EXE)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
