"""csrc/commit_next.h on the host: the control block the append launch's finalize block writes (a whole DevCtrl) and
the scalars the launch's other workgroups derive (a CommitRegs filled from the same block) come from the same
functions - tests/commit_next_harness.cpp runs both on 200 000 random rounds (committed, faulted, cut by the iteration
cap, stopped by the node / border capacity) and compares every field the workgroups read.  No GPU: the header is built
with the host compiler alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")      # (kernels.h names HIP's host types)


def test_finalize_block_and_derived_scalars_agree(tmp_path):
    out = tmp_path / "commit_next_harness"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROCM, "include"),
                           "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "commit_next_harness.cpp"), "-o", str(out)])
    text = subprocess.check_output([str(out)], text=True)
    assert text.startswith("ok "), text
