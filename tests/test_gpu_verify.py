"""GPU tests of ZraHipVerifyArchive (include/zra_hip.h): every faulty frame of a device-resident archive, in frame order, without an
output buffer. Yardsticks: for the content stage the status ZraHipDecompressRABatch gives under ZRA_HIP_OPT_RA_WHOLE_FRAMES for a
one-byte query inside each frame (existing code); for the structure stage the pure-Python model of the header comment's table
(tests/verify_model.py, cross-checked on the CPU in tests/test_verify_abi.py). Archives are written on the device and damaged on the
host before upload."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import corpus as C
import verify_model as M
from test_gpu_update import _compress, _data, _dev, _update

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
MAXU64 = (1 << 64) - 1
DAMAGED = [0, 63, 64, 65, 255, 256, 299]


def _verify(eng, arc, d_arc=None, **kw):
    """((zra, zstd), n_faults, [(frame, code, stage)]) of one verification"""
    import zra_amd
    d = _dev(arc) if d_arc is None else d_arc
    try:
        n, faults = eng.verify(d.data_ptr(), len(arc), **kw)
        return (0, 0), n, faults
    except zra_amd.ZraError as e:
        return (e.zra, e.zstd), 0, []


def _frame_status(eng, zra, arc, frames=None, d_arc=None):
    """{frame: zstd code} of the frames whose whole-frame one-byte query fails (the yardstick); frames whose first byte the
    reference's bound does not let a query reach are left out"""
    import torch
    L = zra.load()
    d = _dev(arc) if d_arc is None else d_arc
    d_out = torch.empty(64, dtype=torch.uint8, device="cuda:0")
    hs, t, F, fs, U = M.fields(arc)
    bad = {}
    before = L.ZraHipGetOptions()
    L.ZraHipSetOptions(8)                                                      # ZRA_HIP_OPT_RA_WHOLE_FRAMES
    try:
        for f in (range(F) if frames is None else frames):
            if f * fs + 1 >= U:
                continue
            try:
                eng.decompress_ra_batch(d.data_ptr(), len(arc), d_out.data_ptr(), [f * fs], [1], [0])
            except zra.ZraError as x:
                assert x.zra == 1, (f, x)
                bad[f] = x.zstd
    finally:
        L.ZraHipSetOptions(before)
    return bad


def _flip_mid(arc, frames):
    hs = M.fields(arc)[0]
    e = M.entries(arc)
    a = bytearray(arc)
    for k in frames:
        a[hs + (e[k] + e[k + 1]) // 2] ^= 0x10
    return bytes(a)


@pytest.fixture(scope="module")
def damaged300(zra, gpu_engine):
    """300 frames of 1,024 bytes (the last one short, more than 2 bytes), checksums on, seven of them with one byte flipped in the
    middle of their compressed span; the yardstick statuses of all 300, computed once"""
    fs = 1024
    data = _data(np.random.RandomState(300), 299 * fs + 700)
    arc = _flip_mid(_compress(gpu_engine, zra, data, 3, fs, True), DAMAGED)
    d_arc = _dev(arc)
    want = _frame_status(gpu_engine, zra, arc, d_arc=d_arc)
    return dict(arc=arc, d_arc=d_arc, want=want)


# ---- 1
@pytest.mark.parametrize("level", [1, 3, 9])
@pytest.mark.parametrize("ck", [True, False])
@pytest.mark.parametrize("fs,nfr", [(1024, 70), (65536, 9), (262144, 4)])
def test_clean_archives_have_no_faults(zra, gpu_engine, fs, nfr, ck, level):
    n = nfr * fs + fs // 3 + 1
    data = _data(np.random.RandomState(fs + level), n)
    arc = _compress(gpu_engine, zra, data, level, fs, ck)
    assert M.structure_faults(arc) == {}
    if fs == 262144:
        hs, e = M.fields(arc)[0], M.entries(arc)
        assert len(M.block_headers(arc[hs + e[0]:hs + e[1]])) >= 2               # the block walk takes more than one step
    d = _dev(arc)
    st, nf, faults = _verify(gpu_engine, arc, d, content=False)
    s = gpu_engine.verify_stats()
    assert (st, nf, faults) == ((0, 0), 0, []), (st, nf, faults)
    assert gpu_engine.kernel_stats()["dec_launches"] == 0
    assert s == dict(frames=nfr + 1, checked=nfr + 1, structure_faults=0, content_faults=0, decoded=0, content_bytes=0, passes=0), s
    st, nf, faults = _verify(gpu_engine, arc, d, content=True)
    s = gpu_engine.verify_stats()
    assert (st, nf, faults) == ((0, 0), 0, []), (st, nf, faults)
    assert gpu_engine.kernel_stats()["dec_launches"] >= 1
    assert s == dict(frames=nfr + 1, checked=nfr + 1, structure_faults=0, content_faults=0, decoded=nfr + 1, content_bytes=n, passes=1), s


# ---- 2
def test_every_bad_frame_is_reported_in_order_and_nothing_else(zra, gpu_engine, damaged300):
    want = damaged300["want"]
    assert sorted(want) == DAMAGED and all(c != 0 for c in want.values()), want
    st, nf, faults = _verify(gpu_engine, damaged300["arc"], damaged300["d_arc"], content=True)
    assert st == (0, 0) and nf == 7
    assert [f for f, _, _ in faults] == DAMAGED
    assert all(stage == M.CONTENT for _, _, stage in faults), faults
    assert {f: c for f, c, _ in faults} == want
    s = gpu_engine.verify_stats()
    assert (s["frames"], s["checked"], s["structure_faults"], s["content_faults"], s["decoded"]) == (300, 300, 0, 7, 300), s
    # the flips are inside block contents: the structure stage alone has nothing to say
    assert _verify(gpu_engine, damaged300["arc"], damaged300["d_arc"], content=False) == ((0, 0), 0, [])


# ---- 3
def test_passes(zra, gpu_engine, damaged300):
    arc, d = damaged300["arc"], damaged300["d_arc"]
    ref = _verify(gpu_engine, arc, d)
    assert ref[1] == 7 and gpu_engine.verify_stats()["passes"] == 1
    assert _verify(gpu_engine, arc, d, staging_bytes=16 * 1024) == ref
    s = gpu_engine.verify_stats()
    assert s["passes"] == 19 and s["decoded"] == 300, s                         # ceil(300 / 16)
    assert _verify(gpu_engine, arc, d, staging_bytes=1) == ref                  # one slot
    assert gpu_engine.verify_stats()["passes"] == 300
    # scratch handed back in between: the same answer
    gpu_engine.release_scratch()
    assert _verify(gpu_engine, arc, d, staging_bytes=5 * 1024) == ref


# ---- 4
def test_capacity_and_ranges(zra, gpu_engine, damaged300):
    L = zra.load()
    arc, d = damaged300["arc"], damaged300["d_arc"]
    want = damaged300["want"]

    def raw(cap, first=0, count=MAXU64, mode=2):
        arr = (zra.ZraHipFrameFault * (cap + 2))()                            # two entries more than the call may write
        ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
        n = ctypes.c_size_t(0x1234)
        gpu_engine._order()
        st = L.ZraHipVerifyArchive(gpu_engine.h, d.data_ptr(), len(arc), mode, first, count, 0, arr if cap else None, cap, ctypes.byref(n)).tup()
        return st, n.value, bytes(arr)

    def listed(mem, k):
        return [(x.frame, x.code, x.stage) for x in (zra.ZraHipFrameFault * k).from_buffer_copy(mem[:16 * k])]

    full = [(f, want[f], M.CONTENT) for f in DAMAGED]
    st, n, mem = raw(3)
    assert st == (0, 0) and n == 7 and listed(mem, 3) == full[:3] and mem[48:] == b"\xEE" * 32   # all counted, three listed
    st, n, mem = raw(9)
    assert st == (0, 0) and n == 7 and listed(mem, 7) == full and mem[7 * 16:] == b"\xEE" * 64   # the sentinel stays behind the faults
    st, n, mem = raw(0)
    assert st == (0, 0) and n == 7 and mem == b"\xEE" * 32                     # NULL array with capacity 0
    # ranges
    assert _verify(gpu_engine, arc, d, first_frame=64, frame_count=192)[1:] == (3, [(f, want[f], M.CONTENT) for f in (64, 65, 255)])
    s = gpu_engine.verify_stats()
    assert (s["frames"], s["checked"], s["decoded"], s["content_faults"]) == (300, 192, 192, 3), s
    assert _verify(gpu_engine, arc, d, first_frame=65, frame_count=1)[1:] == (1, [(65, want[65], M.CONTENT)])
    assert _verify(gpu_engine, arc, d, first_frame=299)[1:] == (1, [(299, want[299], M.CONTENT)])
    for first, count in ((10, 0), (300, 0), (300, MAXU64)):
        st, n, mem = raw(4, first, count)
        assert (st, n) == ((0, 0), 0) and mem == b"\xEE" * 96, (first, count)
    assert gpu_engine.verify_stats() == dict(zip(zra.VERIFY_STATS, (300, 0, 0, 0, 0, 0, 0)))
    for first, count in ((200, 101), (301, 0), (301, MAXU64), (0, 301), (MAXU64, 1), (5, MAXU64 - 1)):
        st, n, mem = raw(4, first, count)
        assert (st, n) == ((5, 0), 0) and mem == b"\xEE" * 96, (first, count)
        assert set(gpu_engine.verify_stats().values()) == {0}
    # refusals behind a real engine
    n = ctypes.c_size_t(0x1234)
    arr = (zra.ZraHipFrameFault * 2)()
    for args in ((None, len(arc), 2, 0, MAXU64, 0, arr, 2, ctypes.byref(n)), (d.data_ptr(), len(arc), 2, 0, MAXU64, 0, None, 2, ctypes.byref(n)),
                 (d.data_ptr(), len(arc), 0, 0, MAXU64, 0, arr, 2, ctypes.byref(n)), (d.data_ptr(), len(arc), 4, 0, MAXU64, 0, arr, 2, ctypes.byref(n)),
                 (d.data_ptr(), len(arc), 2, 0, MAXU64, 0, arr, 2, None)):
        assert L.ZraHipVerifyArchive(gpu_engine.h, *args).tup() == (1, 42), args
    assert n.value == 0


# ---- 5
def _structure_cases(eng, zra, fs, nfr):
    """(name, archive, expected {frame: code} or None for 'the model's') of the structure classes on one clean archive per setting"""
    data = _data(np.random.RandomState(fs), (nfr - 1) * fs + fs // 2)
    arc = _compress(eng, zra, data, 3, fs, True)
    plain = _compress(eng, zra, data, 3, fs, False)
    hs, t, F, _, U = M.fields(arc)
    e = M.entries(arc)
    assert F == nfr and M.structure_faults(arc) == {} and M.structure_faults(plain) == {}
    magic = bytearray(arc); magic[hs + e[2]] ^= 0x40
    ep = M.entries(plain)
    last = M.block_headers(plain[hs + ep[1]:hs + ep[2]])[-1]
    nolast = bytearray(plain); nolast[hs + ep[1] + last] &= 0xFE
    return [
        ("magic", bytes(magic), {2: 10}),
        ("entry moved", M.set_entry(arc, 2, e[2] + 1), None),
        ("last entry short", M.set_entry(arc, F, e[F] - 1), {F - 1: 72}),
        ("last entry beyond the body", M.set_entry(arc, F, e[F] + 1000), {F - 1: 72}),
        ("truncated", arc[:-5], {F - 1: 72}),
        ("inverted span", M.set_entry(arc, 1, e[2] + 7), None),
        ("content size right", M.with_fcs(arc, 1, fs), {}),
        ("content size larger", M.with_fcs(arc, 1, fs + 1), {1: 70}),
        ("content size smaller", M.with_fcs(arc, F - 1, U - (F - 1) * fs - 1), {F - 1: 20}),
        ("last block bit cleared", bytes(nolast), {1: 72}),
    ]


CLASSES = ["magic", "entry moved", "last entry short", "last entry beyond the body", "truncated", "inverted span", "content size right",
           "content size larger", "content size smaller", "last block bit cleared"]
_cases = {}


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("fs,nfr", [(65536, 8), (262144, 3)])
def test_structure_classes(zra, gpu_engine, fs, nfr, name):
    """Codes and frame sets against the model, in both modes, and the property that a frame the structure stage flags also fails its
    whole-frame random-access query. ("last block bit cleared" is the class that needs whole-frame jobs to run without a limit: a job
    limited to the expected size stops before the frame end that the cleared bit takes away.)"""
    if (fs, nfr) not in _cases:
        _cases[(fs, nfr)] = {c[0]: c[1:] for c in _structure_cases(gpu_engine, zra, fs, nfr)}
    a, expect = _cases[(fs, nfr)][name]
    model = M.structure_faults(a)
    if expect is not None:
        assert model == expect, (name, model)
    else:
        assert len(model) >= 2, (name, model)
    d = _dev(a)
    st, n, faults = _verify(gpu_engine, a, d, content=False)
    assert st == (0, 0) and n == len(model), (name, st, faults)
    assert faults == [(f, model[f], M.STRUCTURE) for f in sorted(model)], (name, faults, model)
    s = gpu_engine.verify_stats()
    assert (s["checked"], s["structure_faults"], s["content_faults"], s["decoded"], s["passes"]) == (nfr, len(model), 0, 0, 0), (name, s)
    # content mode: the same frames, found by the structure stage, and they are not decoded
    st, n, faults2 = _verify(gpu_engine, a, d, content=True)
    assert st == (0, 0) and faults2 == faults, (name, faults2)
    s = gpu_engine.verify_stats()
    assert (s["structure_faults"], s["content_faults"], s["decoded"]) == (len(model), 0, nfr - len(model)), (name, s)
    # structure never cries wolf: a flagged frame does not decode
    bad = _frame_status(gpu_engine, zra, a, frames=sorted(model), d_arc=d)
    print(name, "flagged", model, "whole-frame queries that fail", bad)
    assert set(bad) == set(model), (name, bad, model)


def test_structure_never_cries_wolf_on_mutated_archives(zra, gpu_engine):
    def compress(data, level, fs, ck):
        return (0, 0), _compress(gpu_engine, zra, data, level, fs, ck)

    ran = flagged = 0
    for case, a in C.mutated_archives(77, 24, compress):
        d = _dev(a)
        st, n, faults = _verify(gpu_engine, a, d, content=False)
        if st != (0, 0):
            assert n == 0 and faults == []
            continue                                                           # (a header the call refuses: test_header)
        ran += 1
        model = M.structure_faults(a)
        assert faults == [(f, model[f], M.STRUCTURE) for f in sorted(model)], (case, faults, model)
        hs, t, F, fs, U = M.fields(a)
        reachable = [f for f in model if f * fs + 1 < U]
        bad = _frame_status(gpu_engine, zra, a, frames=reachable, d_arc=d)
        assert set(bad) == set(reachable), (case, bad, model)
        flagged += len(reachable)
        # and the content stage reports exactly the frames that do not decode, whichever stage finds them
        st, n, both = _verify(gpu_engine, a, d, content=True)
        every = _frame_status(gpu_engine, zra, a, d_arc=d)
        assert st == (0, 0) and {f for f, _, _ in both if f * fs + 1 < U} == set(every), (case, both, every)
        assert {f: c for f, c, s in both if s == M.CONTENT and f * fs + 1 < U} == {f: c for f, c in every.items() if f not in model}, (case, both, every)
    assert ran >= 8, ran


# ---- 6
def test_header(zra, gpu_engine):
    import oracle_lib as O
    L = zra.load()
    fs = 4096
    arc = _compress(gpu_engine, zra, _data(np.random.RandomState(6), 20 * fs + 9), 3, fs, True)
    assert M.crc_ok(arc)

    def raw(a, d):
        arr = (zra.ZraHipFrameFault * 4)()
        ctypes.memset(arr, 0xEE, ctypes.sizeof(arr))
        n = ctypes.c_size_t(0x1234)
        gpu_engine._order()
        st = L.ZraHipVerifyArchive(gpu_engine.h, d.data_ptr(), len(a), 2, 0, MAXU64, 0, arr, 4, ctypes.byref(n)).tup()
        return st, n.value, bytes(arr)

    # one flipped bit in the seek table, the stored CRC-32 left alone (a low bit: ZraHipArchiveOpen has no objection)
    bad = bytearray(arc); bad[38 + 5 * 7] ^= 1; bad = bytes(bad)
    d = _dev(bad)
    h = ctypes.c_void_p()
    assert L.ZraHipArchiveOpen(gpu_engine.h, d.data_ptr(), len(bad), 0, ctypes.byref(h)).tup() == (0, 0)
    L.ZraHipArchiveClose(h)
    assert raw(bad, d) == ((3, 0), 0, b"\xEE" * 64)
    assert set(gpu_engine.verify_stats().values()) == {0}
    fixed = M.fix_crc(bad)                                                      # with the CRC redone the call runs, and finds frames 6 and 7
    st, n, mem = raw(fixed, _dev(fixed))
    assert st == (0, 0) and n == 2 and set(M.structure_faults(fixed)) == {6, 7}
    # a flipped bit in the stored CRC itself
    b2 = bytearray(arc); b2[14] ^= 0x80
    assert raw(bytes(b2), _dev(b2)) == ((3, 0), 0, b"\xEE" * 64)
    # damaged header fields: the status of opening a handle where that fails, HeaderInvalid or a run by the CRC otherwise
    n_open = n_crc = 0
    for case, a, _, _, _ in C.mutated_headers(321, 40, O.zra_compress):
        d = _dev(a)
        so = L.ZraHipArchiveOpen(gpu_engine.h, d.data_ptr(), len(a), 0, ctypes.byref(h)).tup()
        st, n, mem = raw(a, d)
        if so != (0, 0):
            assert st == so and n == 0 and mem == b"\xEE" * 64, (case, st, so)
            n_open += 1
        else:
            L.ZraHipArchiveClose(h)
            if M.crc_ok(a):
                assert st == (0, 0), (case, st)
            else:
                assert st == (3, 0) and n == 0 and mem == b"\xEE" * 64, (case, st)
                n_crc += 1
    assert n_open > 0 and n_crc > 0
    for size in (0, 10, 38, 42):
        assert raw(arc[:size], _dev(arc))[:2] == ((5, 0), 0), size


# ---- 7
def test_damage_carried_over_by_an_update_is_found(zra, gpu_engine):
    fs = 4096
    data = _data(np.random.RandomState(7), 20 * fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    bad = _flip_mid(arc, [7])
    want = _frame_status(gpu_engine, zra, bad)
    assert set(want) == {7}
    st, out, size = _update(gpu_engine, zra, bad, [(2 * fs + 5, b"\x02" * 10)])
    assert st == (0, 0)
    new = out[:size]
    assert M.crc_ok(new)
    assert _verify(gpu_engine, new) == ((0, 0), 1, [(7, want[7], M.CONTENT)])
    assert _verify(gpu_engine, new, content=False) == ((0, 0), 0, [])
    # the same write into the sound archive leaves nothing to find
    st, out, size = _update(gpu_engine, zra, arc, [(2 * fs + 5, b"\x02" * 10)])
    assert st == (0, 0) and _verify(gpu_engine, out[:size]) == ((0, 0), 0, [])


# ---- 8
def test_cli_mode_t(zra, gpu_engine, damaged300, tmp_path):
    fs = 1024
    clean = _compress(gpu_engine, zra, _data(np.random.RandomState(8), 40 * fs + 5), 3, fs, True)
    p_clean, p_bad, p_junk = tmp_path / "clean.zra", tmp_path / "bad.zra", tmp_path / "junk.zra"
    p_clean.write_bytes(clean); p_bad.write_bytes(damaged300["arc"]); p_junk.write_bytes(b"\x01" * 100)
    r = subprocess.run([TOOL, "t", str(p_clean)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "41 frames" in r.stdout and "0 faulty" in r.stdout
    r = subprocess.run([TOOL, "t", str(p_bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, (r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    assert [int(ln.split()[1].rstrip(":")) for ln in lines] == DAMAGED
    for ln, f in zip(lines, DAMAGED):
        assert "zstd error %d " % damaged300["want"][f] in ln and "content" in ln
    assert "7 faulty" in r.stdout
    r = subprocess.run([TOOL, "t", str(p_junk)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.stdout, r.stderr)
