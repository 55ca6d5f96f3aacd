"""The scratch arithmetic of the encode driver (zra_amd/csrc/zra_enc_plan.h) on the CPU. The header is host-only C++, so the parameter
rows and the per-frame strides are compiled into a small program (tools/model/enc_plan_check.cpp) and walked over every level -128..22
and ten frame sizes, with and without a short last frame: the sequence store of a frame holds blockSize / minMatch sequences for both
parameter sets (it was blockSize / 4 whatever minMatch: the optimal parsers of levels 12-22 write up to blockSize / 3), it stays a
multiple of 8, and every stride of a call with minMatch >= 4 is what it was. The dense-word inputs of encoder_cases.py then hold the
oracle's own sequence counts against the stride of their call: more than a quarter of the block, and no more than the stride."""
import os
import re
import subprocess

import pytest

import encoder_cases as E
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("enc_plan") / "enc_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "zra_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tools", "model", "enc_plan_check.cpp")])
    return exe


def test_strides_hold_what_a_block_can_produce(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:]
    m = re.search(r"cases (\d+) bad (\d+)", r.stdout)
    # 151 levels x 10 frame sizes x (no tail + up to three tails, each behind three full frames and alone)
    assert m and (int(m.group(1)), int(m.group(2))) == (9664, 0), r.stdout[-1500:]


def test_the_driver_takes_its_strides_from_the_plan():
    """zra_encode.hip computes no stride of its own: both paths (the batch path and the persistent pipeline) read the one EncPlan"""
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_encode.hip")).read()
    assert '#include "zra_enc_plan.h"' in src and "enc_plan(full, tail, frameSize, maxBlocksPerFrame)" in src
    assert not re.search(r"seqStride\s*=\s*\(", src) and not re.search(r"entWorkStride\s*=\s*\(", src) and "/ 4 + 16" not in src


def test_dense_word_inputs_fit_the_sequence_store(checker):
    cases = bad = dense = 0
    for name, d, level, fs, ck, must in E.directed_cases():
        if "dense" not in must:
            continue
        r = subprocess.run([checker, "stride", str(level), str(fs), str(len(d))], capture_output=True, text=True, timeout=60)
        m = re.match(r"seqStride (\d+) minMatch (\d+) (\d+) blockSize (\d+) (\d+)", r.stdout)
        assert r.returncode == 0 and m, r.stdout
        stride, block = int(m.group(1)), int(m.group(4))
        over = []
        for f in range(0, len(d), fs):
            n = len(O.sequences(d[f:f + fs], level)) - 1          # (the oracle appends the block's last literals as one more entry)
            cases += 1
            bad += n > stride
            over.append(n > block // 4 + 16)
            print(name, "frame", f // fs, "sequences", n, "stride", stride, "a quarter of the block + 16:", block // 4 + 16)
        # the input does what it is for: a frame with more sequences than the old stride, next to a neighbour (or as the call's last frame)
        assert any(over), name
        assert over[-1] if name.endswith("-last") else len(over) >= 3, name
        dense += 1
    print("cases %d bad %d" % (cases, bad))
    assert dense >= 5 and cases >= 15 and bad == 0
