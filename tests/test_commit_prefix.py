"""csrc/commit_next.h on the host: the node-id prefix the append launch derives from k_commit's workgroup lines
(commit_line_prefix: accepted samples before every 64-sample group; a line counts when it carries the commit's launch
number) - tests/commit_prefix_harness.cpp holds it against a plain running sum for 1, 2, 64, 65, 256, 257 and 1024
lines with current, stale and mixed stamps and counts of 0 and 64.  No GPU: the header is built with the host compiler
alone, once as it is and once with the address and undefined-behaviour sanitizers, as a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "space_filling_forest_star_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")      # (kernels.h names HIP's host types)


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_prefix_of_the_workgroup_lines(tmp_path, flags):
    out = tmp_path / "commit_prefix_harness"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I" + CSRC, "-I" + os.path.join(ROCM, "include"),
                           "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "commit_prefix_harness.cpp"), "-o", str(out)])
    text = subprocess.check_output([str(out)], text=True)
    assert text.startswith("ok "), text
