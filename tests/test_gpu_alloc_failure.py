"""GPU tests of the memory_allocation contract of the device calls ("memory_allocation"): when a piece of engine scratch
cannot be reserved the call answers {ZStdError, 64}, writes none of the caller's outputs, leaves its own counters zero and the other
calls' alone, and the engine goes on working: the next call that fits gives the answer of its CPU model.

DevBuf::reserve (zra_amd/csrc/zra_engine.hip) frees before it asks, so a failed reservation leaves its buffer empty; the bring-up knob
ZRA_ALLOC_LIMIT_MIB makes every reservation whose padded size (n + n / 8 + 256) exceeds the limit fail, and is read once per process.
So every group of cases runs in a fresh child process (tests/alloc_failure_cases.py GROUP), which prints one JSON line per case and
stops at the first one that does not hold; the sizes of each group and where they come from stand there, in front of the group. A
case that does not fail where it was built to fail is a failure of the test ("sizes no longer straddle the limit").

A child that dies of a signal, is aborted, runs into its time limit, fails a device synchronise (exit 3) or reports an illegal memory
access has met a fault on the device:
the tests of this module that follow it do not start another process on that device."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "alloc_failure_cases.py")
KNOBS = ("ZRA_ALLOC_LIMIT_MIB", "ZRA_DEC_SMALL_MAX", "ZRA_SCRATCH_CAP_GIB", "ZRA_DEC_FMB", "ZRA_DEC_FMB_MIN")
_FAULT = None                                                                  # why the rest of the module is skipped


def _child(group, env, n_cases, timeout=240):
    """runs one group; returns its cases {name: line}. Asserts exit 0, every case ok, the closing line, and the number of cases."""
    global _FAULT
    if _FAULT:
        pytest.skip(_FAULT)
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    t = time.time()
    try:
        r = subprocess.run([sys.executable, CHILD, group], env=e, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as x:
        _FAULT = "the child of group %s ran into its time limit" % group
        pytest.fail("%s; its output: %s" % (_FAULT, (x.stdout or "")[-1500:]))
    wall = time.time() - t
    # (exit 3: the child's synchronise failed, a HIP error of whatever kind)
    if r.returncode < 0 or r.returncode in (3, 124, 134, 137, 139) or "illegal memory access" in r.stderr:
        _FAULT = "the child of group %s met a fault (exit %d)" % (group, r.returncode)
    lines = [json.loads(x) for x in r.stdout.split("\n") if x.startswith("{")]
    print("group %s %s: %.1f s, %d cases: %s" % (group, env, wall, len(lines), [(c["case"], c["s"]) for c in lines]))
    bad = [c for c in lines if not c["ok"]]
    assert not bad and r.returncode == 0, (r.returncode, bad, r.stdout[-1500:], r.stderr[-1500:])
    assert lines and lines[-1]["case"] == "end of " + group and len(lines) == n_cases + 1, lines
    return {c["case"]: c for c in lines}


def test_decode_takes_the_rounds_when_the_block_pass_cannot_reserve():
    """ZraHipDecompressBuffer of 64 and of 96 frames of 256 KiB under an 11 MiB limit: the block-parallel pass of Engine::decode_launch
    fails its reservation (at decSeqs_ behind a decLits_ that has already moved; at decLits_), the rounds' scratch is sized again and
    the rounds decode: Success, the content, 0xEE behind the capacity, a rounds word of 2. Then 256 frames, whose rounds' scratch does
    not fit either: the contract. The premise (the same calls take the block pass when nothing limits them) is the next test."""
    _child("decode", {"ZRA_DEC_SMALL_MAX": "0", "ZRA_ALLOC_LIMIT_MIB": "11"}, 3)


def test_decode_premise_the_same_calls_take_the_block_pass_without_a_limit():
    """Without the limit the calls of the test above take the block pass alone: a rounds word of 1 for 64, 96 and 256 frames. Without
    this the rounds word of 2 there would prove nothing."""
    _child("decode", {"ZRA_DEC_SMALL_MAX": "0"}, 3)


def test_random_access_handle_read_and_update_refuse_a_staging_window_that_does_not_fit():
    """ZraHipDecompressRABatch, ZraHipArchiveRead (a handle without a cache), ZraHipUpdateArchive and ZraHipArchiveUpdate with 200
    touched frames of 64 KiB under an 11 MiB limit: stage_ cannot be had. The contract; the handle's counters stay; a failing update
    through a handle leaves it bound to the old archive, and reads of resident and other frames give the old bytes. Then fewer
    touched frames, against the content and against the oracle's decode of the updated archive. And a read through a handle with a
    cache whose piece list (300,000 queries of three slices) cannot be had: refused in front of the lookup that copies the hits."""
    _child("ra", {"ZRA_ALLOC_LIMIT_MIB": "11"}, 5)


def test_the_searches_and_the_greps_refuse_a_window_that_does_not_fit():
    """search, search_multi, grep, grep(where=...), grep_regex and grep_context over 12 MiB in one window (staging_bytes = 0) under an
    11 MiB limit: the contract. Then a range of 4.5 MiB in two passes of a 4 MiB window, against the models of the per-call tests."""
    _child("scan_a", {"ZRA_ALLOC_LIMIT_MIB": "11"}, 6)


def test_the_extracts_the_cut_the_tally_and_a_handle_grep_refuse_a_window_that_does_not_fit():
    """extract, extract_regex, cut, the composite tally (ZraHipTallyFields: five words zero, workspace and keys untouched) and
    ZraHipArchiveGrep through a handle with 30 resident frames, as in the test above. The handle's counters stay through the failing
    call, its fitting call stages the resident frames, and a read of resident and other frames afterwards gives the content."""
    _child("scan_b", {"ZRA_ALLOC_LIMIT_MIB": "11"}, 5)


def test_tally_text_refuses_a_hash_table_that_does_not_fit():
    """ZraHipTallyRecords of 330,000 two-byte records under an 11 MiB limit: 2^19 slots cannot be had. The same text with
    max_distinct = its 600 distinct keys fits in 1,024 slots and equals tally_model."""
    _child("tally_text", {"ZRA_ALLOC_LIMIT_MIB": "11"}, 1)


def test_compare_diff_sign_and_signature_diff_refuse_a_window_that_does_not_fit():
    """The frame-pass driver's reservation (FramePasses::open) through compare, diff, sign and diff_signature over 768 frames of 16 KiB
    with staging_bytes = 0 under an 11 MiB limit: the contract. Then a 4 MiB window, in two to six passes, against compare_model,
    diff_model and sign_model; the signature diff also against the byte diff at the signature's grain."""
    _child("frames_a", {"ZRA_ALLOC_LIMIT_MIB": "11"}, 4)


def test_index_locate_read_and_verify_refuse_a_window_that_does_not_fit():
    """index_records, locate_records, read_records (400 record numbers: up to 768 boundary frames) and verify in content mode, as in the
    test above, against records_model, and for verify against a sound archive's counters and the oracle's status of one frame with a
    flipped checksum byte."""
    _child("frames_b", {"ZRA_ALLOC_LIMIT_MIB": "11"}, 4)


def test_compress_refuses_scratch_that_does_not_fit_and_leaves_nothing_in_flight():
    """ZraHipCompressBuffer of 64 MiB at level 3 (the persistent path) and level 9 (the batch path: two scratch contexts and a side
    stream) under a 24 MiB limit: the contract. The input is overwritten and freed at once; three frames on the same engine then equal
    the oracle's archive. (The encoder's retry with half the budget needs GiB of scratch to succeed after a failure: not driven here.)"""
    _child("compress", {"ZRA_ALLOC_LIMIT_MIB": "24"}, 2)
