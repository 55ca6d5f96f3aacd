"""The pass arithmetic of the calls on whole frames (zra_amd/csrc/zra_pass_plan.h: verify, sign, index, compare, diff, signature diff)
on the CPU. The header is host-only C++, so the frame-range rule, the passes of a frame range, the content bytes of a range, the
diff's tail behind the common content and the two-half window are compiled into a small program (tools/model/pass_plan_check.cpp)
and walked over every small shape: the passes tile the range in order, a pass has between one frame and a pass's worth, the bytes add
up, the tail's runs tile [C, U), and the range rule is the brute-force one. The GPU tests reach the same code only through whole calls."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_passes_tile_their_range(tmp_path):
    exe = str(tmp_path / "pass_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "zra_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "model", "pass_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:]
    m = re.search(r"cases (\d+) bad (\d+)", r.stdout)
    # U 0..40 x 6 frame sizes x 5 pass sizes x (every (first, count), ~0 included + every C <= U + the window of every slot count)
    assert m and (int(m.group(1)), int(m.group(2))) == (254366, 0), r.stdout[-1500:]
