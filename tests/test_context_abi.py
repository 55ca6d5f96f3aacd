"""CPU tests of the context grep's boundary (include/zra_hip.h: ZraHipGrepArchiveContext, ZraHipArchiveGrepContext): declared, exported
and bound, every rule-1 refusal before anything touches a device with the outputs zeroed, no CPU result without a GPU, the zra_grepc_*
kernels compiled without scratch, the end of a pass and its pending records under the host sanitizers
(tools/model/context_pass_check.cpp), and the model the GPU tests use as their yardstick (tests/context_model.py) agrees with the system's
`grep -F -b -A -B` (and `-v`) on generated lines and with answers pinned by hand."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import context_model as CM
import grep_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["ZraHipGrepArchiveContext", "ZraHipArchiveGrepContext"]
MAXU64 = (1 << 64) - 1
PAIRS = [(0, 0), (1, 0), (0, 1), (2, 3), (64, 64)]                            # (after, before)


def test_context_calls_are_declared_exported_and_bound(zra):
    txt = open(os.path.join(ROOT, "include", "zra_hip.h")).read()
    declared = set(re.findall(r"ZRA_EXPORT[^;(]*?\b(Zra\w+)\s*\(", txt))
    L = zra.load()
    for s in CALLS:
        assert s in declared, s
        assert s in zra.HIP_ABI_SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r"#define\s+ZRA_HIP_GREP_MAX_CONTEXT\s+64u", txt) and re.search(r"#define\s+ZRA_HIP_CONTEXT_SELECTED\s+\(1ull << 63\)", txt)
    assert zra.GREP_MAX_CONTEXT == 64 and zra.CONTEXT_SELECTED == 1 << 63
    assert callable(zra.Engine.grep_context) and callable(zra.Archive.grep_context)


def _sizes(*v):
    return (ctypes.c_uint32 * len(v))(*v)


def test_context_refuses_rule_1_without_an_engine(zra):
    """{ZStdError, 42} from both entry points; the three counts are zeroed and the record array is left alone. nSelected or nGroups
    NULL is accepted (the refusal is the engine's, not theirs)."""
    L = zra.load()
    P = ctypes.c_void_p
    pats = ctypes.create_string_buffer(b"\x07" * 5000)
    nl = ctypes.create_string_buffer(b"ab\ncd")
    # (patterns, sizes, count, syntax, delimiter, mode, before, after)
    cases = [(pats, _sizes(3), 1, 0, 10, 0, 65, 0), (pats, _sizes(3), 1, 0, 10, 0, 0, 65), (pats, _sizes(3), 1, 0, 10, 1, 1 << 31, 2),    # the context
             (pats, _sizes(3), 1, 0, 10, 2, 1, 1), (pats, _sizes(3), 1, 0, 10, 3, 1, 1), (pats, _sizes(3), 1, 0, 10, 0x80000000, 0, 0),   # mode bits
             (nl, _sizes(5), 1, 0, 10, 0, 1, 1), (nl, _sizes(2, 3), 2, 0, 10, 1, 1, 1), (pats, _sizes(3), 1, 0, 7, 0, 0, 0),              # a pattern holds the delimiter
             (pats, _sizes(3), 1, 4, 10, 0, 1, 1), (pats, _sizes(3, 0), 2, 0, 10, 0, 1, 1), (pats, _sizes(3), 0, 0, 10, 0, 1, 1),        # the grep's own
             (None, _sizes(3), 1, 0, 10, 0, 1, 1), (pats, None, 1, 0, 10, 0, 1, 1),
             (pats, _sizes(3), 1, 0, 10, 0, 2, 3), (pats, _sizes(3), 1, 0, 10, 1, 64, 64)]                                                # accepted arguments: no engine
    for hp, hs, k, syntax, delim, mode, before, after in cases:
        for arc in ((None, 0), (P(64), 100)):
            for extra in ((True, True), (False, True), (True, False), (False, False)):
                arr = (ctypes.c_uint64 * 8)()
                ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
                n, ns, ng = ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234), ctypes.c_uint64(0x1234)
                tail = (arr, 4, ctypes.byref(n), ctypes.byref(ns) if extra[0] else None, ctypes.byref(ng) if extra[1] else None)
                tag = (k, syntax, delim, mode, before, after, arc, extra)
                assert L.ZraHipGrepArchiveContext(None, *arc, hp, hs, k, syntax, delim, mode, before, after, 0, MAXU64, 0, *tail).tup() == (1, 42), tag
                assert (n.value, ns.value, ng.value) == (0, 0 if extra[0] else 0x1234, 0 if extra[1] else 0x1234) and bytes(arr) == b"\xEE" * 64, tag
                n.value = ns.value = ng.value = 0x1234
                assert L.ZraHipArchiveGrepContext(None, hp, hs, k, syntax, delim, mode, before, after, 0, MAXU64, 0, *tail).tup() == (1, 42), tag
                assert (n.value, ns.value, ng.value) == (0, 0 if extra[0] else 0x1234, 0 if extra[1] else 0x1234) and bytes(arr) == b"\xEE" * 64, tag
            assert L.ZraHipGrepArchiveContext(None, *arc, hp, hs, k, syntax, delim, mode, before, after, 0, MAXU64, 0, None, 0, None, None, None).tup() == (1, 42)


def test_context_fails_loudly_without_gpu(zra):
    L = zra.load()
    if L.ZraHipDeviceCount() > 0:
        return                                                                 # a GPU is present: tests/test_gpu_grep_context.py
    with pytest.raises(zra.ZraError):
        zra.Engine(0).grep_context(64, 100, [b"abc", b"d"], before=1, after=1)   # no engine without a GPU: never a CPU result


def test_context_kernels_use_no_scratch():
    res = json.load(open(os.path.join(ROOT, "zra_amd", "build", "kernel_resources.json")))
    src = open(os.path.join(ROOT, "zra_amd", "csrc", "zra_grep_context.hip")).read()
    kernels = [k for k in res if k.startswith("zra_grepc_")]
    assert sorted(kernels) == sorted(set(re.findall(r"__global__.*?\b(zra_grepc_\w+)\s*\(", src))) and len(kernels) == 5, kernels
    for k in kernels:
        assert res[k]["source"] == "zra_grep_context.hip", (k, res[k])
        assert res[k]["scratch_bytes"] == 0 and res[k]["vgpr_spill"] == 0 and res[k]["sgpr_spill"] == 0, (k, res[k])
        assert res[k]["lds_bytes"] <= 65536, (k, res[k])
    assert all(res[k]["lds_bytes"] <= 32768 for k in kernels if "scan" not in k)


def test_pending_check_program_under_the_host_sanitizers(tmp_path):
    """(pending), zra_context.h's pass_end() and the slots the fill writes, pass by pass on streams of selection bits"""
    checker = os.path.join(ROOT, "tools", "model", "context_pass_check.cpp")
    csrc = os.path.join(ROOT, "zra_amd", "csrc")
    exe = str(tmp_path / "context_pass_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc, checker, "-o", exe], check=True,
                   capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    m = re.fullmatch(r"context_pass_check: (\d+) cases ok", r.stdout.strip().split("\n")[-1])
    assert m and int(m.group(1)) >= 200000, r.stdout[-500:]
    # stand-alone; the kernels of both sets include the header whose pass end it runs
    assert re.findall(r'#include\s+"([^"]+)"', open(checker).read()) == ["zra_context.h"]
    for name in ("zra_grep_context.hip", "zra_grep_regex_context.hip"):
        assert '#include "zra_context_tile.h"' in open(os.path.join(csrc, name)).read(), name


def _system_grep(tmp_path, data, pats, invert, after, before):
    """([(offset, selected)], groups) as GNU grep prints them: `offset:` in front of a selected line, `offset-` in front of a context
    line, `--` between groups"""
    f = tmp_path / "lines.txt"
    f.write_bytes(data)
    args = ["grep", "-F", "-b", "-a", "-A", str(after), "-B", str(before)] + (["-v"] if invert else [])
    for p in pats:
        args += ["-e", p.decode()]
    r = subprocess.run(args + [str(f)], capture_output=True, env=dict(os.environ, LC_ALL="C"), timeout=60)
    assert r.returncode in (0, 1), r.stderr
    out, groups = [], 0
    for line in r.stdout.split(b"\n")[:-1] if r.stdout else []:
        if line == b"--":
            groups += 1
            continue
        m = re.match(rb"(\d+)([:-])", line)
        assert m, line
        out.append((int(m.group(1)), m.group(2) == b":"))
    return out, groups + (1 if out else 0)


@pytest.mark.skipif(shutil.which("grep") is None, reason="no system grep")
def test_model_agrees_with_the_system_grep(tmp_path):
    rng = np.random.RandomState(52)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"eps", b"zeta", b"x"]
    seen_groups = 0
    for case in range(12):
        density = [2, 8, 40, 200][case % 4]
        lines = []
        for _ in range(int(rng.randint(1, 400))):
            k = int(rng.randint(1, 5))                                         # (no empty line: grep -F with a pattern list treats none specially, but keep it plain)
            w = [words[int(rng.randint(0, len(words)))] for _ in range(k)]
            if rng.randint(0, density) == 0:
                w.insert(int(rng.randint(0, k + 1)), b"NEEDLE" if rng.randint(0, 2) else b"pin")
            lines.append(b" ".join(w))
        data = b"\n".join(lines) + (b"\n" if case % 2 else b"")
        pats = [b"NEEDLE", b"pin"]
        for after, before in PAIRS:
            for invert in (False, True):
                listed, nsel, groups, recs, _ = CM.context(data, pats, 10, invert, before, after)
                want, wgroups = _system_grep(tmp_path, data, pats, invert, after, before)
                assert [(o, s) for o, _, s in listed] == want, (case, after, before, invert)
                assert groups == wgroups and nsel == sum(1 for _, s in want if s), (case, after, before, invert, groups, wgroups)
                seen_groups += groups > 1
    assert seen_groups > 10


def test_context_answers_pinned_by_hand():
    d = b"a\nb\nX\nc\nd\ne\nX\nf\ng"
    R = GM.records(d)
    assert R == [(2 * i, 1) for i in range(9)]
    T = lambda ks, sel: [(2 * k, 1, k in sel) for k in ks]
    assert CM.context(d, [b"X"], before=0, after=0)[:3] == (T([2, 6], {2, 6}), 2, 2)
    assert CM.context(d, [b"X"], before=1, after=0)[:3] == (T([1, 2, 5, 6], {2, 6}), 2, 2)
    assert CM.context(d, [b"X"], before=1, after=2)[:3] == (T([1, 2, 3, 4, 5, 6, 7, 8], {2, 6}), 2, 1)   # a gap of 3 == after + before: one group
    assert CM.context(d, [b"X"], before=1, after=1)[:3] == (T([1, 2, 3, 5, 6, 7], {2, 6}), 2, 2)         # 3 > 2: two
    assert CM.context(d, [b"X"], before=64, after=64)[:3] == (T(range(9), {2, 6}), 2, 1)
    assert CM.context(d, [b"X"], invert=True, before=0, after=0)[:3] == (T([0, 1, 3, 4, 5, 7, 8], {0, 1, 3, 4, 5, 7, 8}), 7, 3)
    assert CM.context(d, [b"X"], before=5, after=5, lo=3, hi=9)[:3] == ([(3, 0, False), (4, 1, True), (6, 1, False), (8, 1, False)], 1, 1)   # clipped at both ends
    assert CM.context(d, [b"q"], before=3, after=3)[:3] == ([], 0, 0)
