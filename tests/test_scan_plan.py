"""The pass geometry of the range scans (zra_amd/csrc/zra_scan_plan.h: search, multi-pattern search, grep, extract) on the CPU. The
header is host-only C++, so the arithmetic that decides which pass tests a start position that straddles a pass seam is compiled
into a small program (tools/model/scan_plan_check.cpp) and walked over every small shape: the owned intervals of a call's passes
partition [lo, hi - trim) in order, no pass reaches further into the carry area than it holds, every byte an owned start needs is
decoded in its pass, and the pass count is the frames' ceiling. The GPU tests reach the same code only through whole calls."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_ownership_is_a_partition(tmp_path):
    exe = str(tmp_path / "scan_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "zra_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "model", "scan_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:]
    m = re.search(r"cases (\d+) bad (\d+)", r.stdout)
    # U 1..30 x 6 frame sizes x 5 pattern lengths x 3 pass sizes x every range, trim 0 and, where the range holds a pattern, M - 1
    assert m and (int(m.group(1)), int(m.group(2))) == (785070, 0), r.stdout[-1500:]

