"""The forward's batched-read forms on the host (CPU only).

tests/hostcheck/pre_batch_check.cpp is a stand-alone program over the product's templates (csrc/bb_step.h:
rk_sums_batch; csrc/bb_solve.h: mass_entry_off, tri_unpack_count; the addressing of csrc/bb_team16.h:
mass_dense_team<true>) against copies of the text they replace, bit for bit in float and double, on seeded
values over many binades with the edge cases its header lists.  The same templates run on the GPU in
tests/test_gpu_pre_batch.py.
"""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openballbot-rl_amd" / "csrc"
SRC = ROOT / "tests" / "hostcheck" / "pre_batch_check.cpp"
EXE = ROOT / "tests" / "_build" / "pre_batch_check"


def test_batched_forms_equal_parent_text_on_host():
    EXE.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", f"-I{CSRC}", "-o", str(EXE), str(SRC)],
                   check=True, capture_output=True)
    r = subprocess.run([str(EXE)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
