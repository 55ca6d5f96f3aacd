"""GPU test of the record index through an archive handle (include/zra_hip.h: ZraHipArchiveIndexRecords, ZraHipArchiveLocateRecords,
ZraHipArchiveReadRecords): a whole-frame sweep takes its resident frames out of the handle's arena and decodes the others, the read's
byte fetch is a read of the handle, and every answer is the plain call's on the same bytes. The yardsticks are tests/records_model.py
and the plain engine calls; for a frame that does not decode, _frame_status of tests/test_gpu_verify.py.
Shape A is tests/test_gpu_archive_scan.py's: 40 frames at frame sizes 1,024 and 1,000, the last one of 300 bytes, 12 of them resident in
slots whose order is not frame order; the content is newline-delimited lines with one record of 2,500 bytes across the missing frames
9 to 11, an empty record, a delimiter as the last byte of resident frame 5 and as the first byte of missing frame 3, and no trailing
delimiter. Shape B: 12 frames of 20,000 bytes (three tiles, the last one short), 5 resident. Every device buffer is followed by
sentinel bytes. The expected staged and decoded counts are computed from the model and the warm set."""
import ctypes

import numpy as np
import pytest

import records_model as RM
import test_gpu_grep as G
from test_gpu_archive_scan import MAXU64, NF, WARM, _flen, _open_warm, _resident_ok
from test_gpu_records import (ALL, EXTRA, INDEX_ZERO, LOCATE_ZERO, NL, OOB, READ_ZERO, SENT, SENTW, TOO_SMALL, _idxbuf, _index_raw, _locate_raw, _placed,
                              _read_raw, _words)
from test_gpu_update import _compress, _dev
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
LONG = 2500


def _content(seed, fs):
    U = (NF - 1) * fs + 300
    a = bytearray(G._lines(np.random.RandomState(seed), U))
    s = 9 * fs + 101                                                           # the long record: [s, s + LONG), frames 9, 10, 11
    a[s:s + LONG] = bytes(a[s:s + LONG]).replace(b"\n", b"c")
    a[s - 1] = a[s + LONG] = NL
    a[500] = a[501] = NL                                                       # an empty record
    a[6 * fs - 1] = NL                                                         # the last byte of resident frame 5
    a[3 * fs] = NL                                                             # the first byte of missing frame 3
    data = bytes(a)
    assert len(data) == U and data[-1] != NL
    return data


class Model:
    """the records of a content and, for a list of requests, the frames each sweep needs"""

    def __init__(self, data, fs, delim=NL):
        self.data, self.fs, self.U, self.delim = data, fs, len(data), delim
        self.t = RM.delimiters(data, delim)
        self.D, self.R = RM.counts(data, delim)
        self.F = -(-self.U // fs)
        self.words = RM.index_words(data, fs, delim)
        self.recs = RM.locate(data, delim, range(self.R))

    def boundary_frames(self, numbers):
        need = set()
        for r in numbers:
            if r > 0:
                need.add(self.t[r - 1] // self.fs)
            if r < self.D:
                need.add(self.t[r] // self.fs)
        return sorted(need)

    def boundaries(self, numbers):
        return sum((r != 0) + (r != self.D) for r in numbers)

    def fetch_frames(self, numbers):
        touched = set()
        for r in numbers:
            s, n = self.recs[r]
            n += r < self.D
            touched.update(range(s // self.fs, (s + n - 1) // self.fs + 1))
        return sorted(touched)

    def inside(self, frame, both=True):
        """records whose two boundaries (both) or whose end (not both) lie in `frame`"""
        lo, hi = frame * self.fs, (frame + 1) * self.fs
        return [k for k in range(1, self.D) if lo <= self.t[k] < hi and (not both or lo <= self.t[k - 1] < hi)]


def _slots(staging, fs):
    return 65536 if staging == 0 else max(1, staging // fs)


def _sweep(frames, resident, fs, U, staging):
    """(staged, decoded, decoded bytes, passes) of a whole-frame sweep over `frames`"""
    miss = [f for f in frames if f not in resident]
    return len(frames) - len(miss), len(miss), sum(_flen(f, fs, U) for f in miss), -(-len(frames) // _slots(staging, fs))


def _h_index_raw(zra, h, delim, first=0, count=ALL, staging=0, cap=None, buf=None, d_index=None):
    import torch
    if buf is None:
        buf = _idxbuf(cap)
    torch.cuda.synchronize()
    info = zra.ZraHipRecordIndex(1, 2, 3, 4, 5, 6)
    h.engine._order()
    st = zra.load().ZraHipArchiveIndexRecords(h.h, delim, first, count, staging, (buf.data_ptr() if cap else None) if d_index is None else d_index, cap,
                                              ctypes.byref(info)).tup()
    return dict(st=st, info=(info.contentSize, info.frameSize, info.delimiter, info.frames, info.delimiters, info.records), words=_words(buf), buf=buf)


def _h_locate_raw(zra, h, info, buf, index_words, numbers, staging=0):
    import torch
    n = len(numbers)
    nums = (ctypes.c_uint64 * max(n, 1))(*numbers)
    out = (ctypes.c_uint64 * (2 * n + 2))()
    ctypes.memset(out, 0xEE, ctypes.sizeof(out))
    torch.cuda.synchronize()
    ci = zra.ZraHipRecordIndex(*info)
    h.engine._order()
    st = zra.load().ZraHipArchiveLocateRecords(h.h, ctypes.byref(ci), buf.data_ptr(), index_words, nums, n, staging, out).tup()
    raw = bytes(out)
    return dict(st=st, ranges=[(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)], untouched=raw == b"\xEE" * len(raw), tail_ok=raw[16 * n:] == b"\xEE" * 16)


def _h_read_raw(zra, h, info, buf, index_words, numbers, dcap, staging=0, d_data=None, ranges=True):
    import torch
    n = len(numbers)
    nums = (ctypes.c_uint64 * max(n, 1))(*numbers)
    out = (ctypes.c_uint64 * (2 * n + 2))()
    ctypes.memset(out, 0xEE, ctypes.sizeof(out))
    dbuf = torch.full((dcap + 64,), SENT, dtype=torch.uint8, device="cuda:0") if d_data is None else None
    torch.cuda.synchronize()
    ci = zra.ZraHipRecordIndex(*info)
    size = ctypes.c_uint64(0x1234)
    h.engine._order()
    st = zra.load().ZraHipArchiveReadRecords(h.h, ctypes.byref(ci), buf.data_ptr(), index_words, nums, n, staging, out if ranges else None,
                                             (dbuf.data_ptr() if dcap else None) if d_data is None else d_data, dcap, ctypes.byref(size)).tup()
    torch.cuda.synchronize()
    raw = bytes(out)
    data = dbuf.cpu().numpy().tobytes() if dbuf is not None else b""
    return dict(st=st, size=size.value, ranges=[(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)], untouched=raw == b"\xEE" * len(raw),
                data=data[:dcap], sentinel_ok=data[dcap:] == bytes([SENT]) * 64 if dbuf is not None else True,
                all_sentinel=data == bytes([SENT]) * (dcap + 64) if dbuf is not None else True)


def _plain_index(eng, zra, A, F, cap=None):
    """the whole archive indexed by the plain call into a buffer of `cap` words; (RecordIndex, buffer)"""
    r = _index_raw(eng, zra, A, NL, cap=F if cap is None else cap)
    assert r["st"] == (0, 0), r["st"]
    return zra.RecordIndex(*r["info"]), r["buf"]


@pytest.fixture(scope="module", params=[1024, 1000])
def shape(request, zra, gpu_engine):
    """the archive, its model, its plain index (computed once, left unchanged) and a handle that only index and locate calls use: its
    resident set stays the warm set"""
    fs = request.param
    data = _content(91, fs)
    m = Model(data, fs)
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    A = (d, len(arc))
    idx, buf = _plain_index(gpu_engine, zra, A, NF)
    assert _words(buf)[:NF] == m.words and (idx.delimiters, idx.records) == (m.D, m.R) and m.R == m.D + 1
    h = _open_warm(zra, gpu_engine, d, len(arc), fs, len(data))
    _resident_ok(h)
    yield dict(fs=fs, U=len(data), data=data, m=m, arc=arc, d=d, A=A, idx=idx, buf=buf, h=h)
    h.close()


def _requests(m, fs):
    """Record 0, record D, the long record, records inside one resident frame, across a resident and a missing frame, and, for windows of
    one and of three needed frames, across a pass seam; shuffled, with duplicates."""
    long_ = next(k for k, (s, n) in enumerate(m.recs) if n == LONG)
    in6 = m.inside(6)[:3]                                                      # both boundaries in resident frame 6
    assert len(in6) == 3
    res_miss = next(k for k in m.inside(9, both=False) if m.t[k - 1] // fs == 8)      # starts in resident 8, ends in missing 9
    miss_res = next(k for k in m.inside(14, both=False) if m.t[k - 1] // fs == 13)    # starts in missing 13, ends in resident 14
    asc = sorted({0, m.D, long_, res_miss, miss_res, *in6, *m.inside(12)[:2], *m.inside(27)[:2], *m.inside(30)[:2]})
    return long_, asc


# ---- 1
def test_index_through_the_handle(zra, gpu_engine, shape):
    fs, U, m, A, h = (shape[k] for k in ("fs", "U", "m", "A", "h"))
    before = _resident_ok(h)
    tot = h.record_stats()
    for first, count, mixed in ((0, ALL, True), (2, 7, True), (5, 4, False), (9, 5, False), (17, 0, False)):
        frames = list(range(first, NF if count == ALL else first + count))
        for staging in (0, fs, 3 * fs):
            tag = (fs, first, count, staging)
            staged, decoded, _, passes = _sweep(frames, WARM, fs, U, staging)
            if mixed:
                assert staged and decoded, tag
            plain = _index_raw(gpu_engine, zra, A, NL, first=first, count=count, staging=staging, cap=NF)
            ps = gpu_engine.index_records_stats()
            got = _h_index_raw(zra, h, NL, first=first, count=count, staging=staging, cap=NF)
            assert got["st"] == plain["st"] == (0, 0), (tag, got["st"], plain["st"])
            assert got["words"] == plain["words"] and got["info"] == plain["info"], tag
            assert got["words"] == [m.words[f] if f in frames else SENTW for f in range(NF)] + [SENTW] * EXTRA, tag
            if count == ALL:
                assert got["info"] == (U, fs, NL, NF, m.D, m.R), tag
            assert gpu_engine.index_records_stats() == ps and ps["indexed"] == len(frames), (tag, ps)
            tot = dict(calls=tot["calls"] + 1, staged=staged, decoded=decoded, passes=passes if frames else 0,
                       staged_total=tot["staged_total"] + staged, decoded_total=tot["decoded_total"] + decoded)
            assert h.record_stats() == tot, (tag, h.record_stats(), tot)
            if frames and not decoded:
                assert gpu_engine.kernel_stats()["dec_launches"] == 0 and h.record_stage_ms() > 0, tag
            if not frames:
                assert h.record_stage_ms() == 0, tag
            assert h.stats() == before, tag
    assert _sweep(list(range(5, 9)), WARM, fs, U, 0)[:2] == (4, 0) and _sweep(list(range(9, 14)), WARM, fs, U, 0)[:2] == (0, 5)


# ---- 2
def test_locate_through_the_handle(zra, gpu_engine, shape):
    fs, U, m, A, h, idx, buf = (shape[k] for k in ("fs", "U", "m", "A", "h", "idx", "buf"))
    long_, asc = _requests(m, fs)
    rng = np.random.RandomState(5)
    shuffled = [asc[i] for i in rng.permutation(len(asc))] + [asc[3], asc[3], 0, m.D]
    before = _resident_ok(h)
    for numbers in (asc, asc[::-1], shuffled, [long_], [0], [m.D]):
        need = m.boundary_frames(numbers)
        for staging in (0, fs, 3 * fs):
            tag = (fs, len(numbers), staging)
            staged, decoded, dec_bytes, passes = _sweep(need, WARM, fs, U, staging)
            if len(numbers) > 1:
                assert staged and decoded, tag
                # a request whose two boundary frames lie in different passes of this window (frames 8 | 9 and 13 | 14 are neighbours in `need`)
                assert staging == 0 or any(need.index(m.t[k] // fs) // _slots(staging, fs) != need.index(m.t[k - 1] // fs) // _slots(staging, fs)
                                           for k in numbers if 0 < k < m.D and m.t[k] // fs != m.t[k - 1] // fs), tag
            want = RM.locate(m.data, NL, numbers)
            plain = _locate_raw(gpu_engine, zra, A, idx, buf, NF, numbers, staging)
            ps = gpu_engine.locate_records_stats()
            tot = h.record_stats()
            got = _h_locate_raw(zra, h, idx, buf, NF, numbers, staging)
            assert got["st"] == plain["st"] == (0, 0), (tag, got["st"])
            assert got["ranges"] == plain["ranges"] == want and got["tail_ok"], tag
            hs = gpu_engine.locate_records_stats()
            assert ps == dict(frames=NF, records=len(numbers), boundaries=m.boundaries(numbers), decoded=len(need),
                              content_bytes=sum(_flen(f, fs, U) for f in need), passes=passes), (tag, ps)
            assert hs == dict(ps, decoded=decoded, content_bytes=dec_bytes), (tag, hs)
            assert gpu_engine.locate_records_ms() > 0, tag
            assert h.record_stats() == dict(calls=tot["calls"] + 1, staged=staged, decoded=decoded, passes=passes,
                                            staged_total=tot["staged_total"] + staged, decoded_total=tot["decoded_total"] + decoded), tag
            if not decoded:
                assert gpu_engine.kernel_stats()["dec_launches"] == 0, tag
            assert h.stats() == before, tag
    assert m.boundary_frames([long_]) == [9, 11] and m.boundary_frames([0]) == [0] and m.boundary_frames([m.D]) == [39]


# ---- 3
def test_read_through_the_handle(zra, gpu_engine, shape):
    fs, U, m, A, d, idx, buf = (shape[k] for k in ("fs", "U", "m", "A", "d", "idx", "buf"))
    long_, _ = _requests(m, fs)
    res_miss = next(k for k in m.inside(9, both=False) if m.t[k - 1] // fs == 8)
    numbers = [m.D, long_, m.inside(6)[0], 0, res_miss, long_]
    want = RM.packed(m.data, NL, numbers)
    need, touched = m.boundary_frames(numbers), m.fetch_frames(numbers)
    assert touched == [0, 6, 8, 9, 10, 11, 39] and need == [0, 6, 8, 9, 11, 39]    # frame 10 is interior: only the fetch needs it
    for staging in (0, fs):
        h = _open_warm(zra, gpu_engine, d, A[1], fs, U)
        cache = _resident_ok(h)
        plain = _read_raw(gpu_engine, zra, A, idx, buf, NF, numbers, len(want) + 5, staging)
        assert plain["st"] == (0, 0) and plain["data"][:len(want)] == want
        # the sizing call: the locate sweep only, no cache counter moves
        q = _h_read_raw(zra, h, idx, buf, NF, numbers, 0, staging)
        assert q["st"] == TOO_SMALL and q["size"] == len(want) and q["untouched"], q["st"]
        assert h.stats() == cache and gpu_engine.read_records_stats() == READ_ZERO and h.record_stats()["calls"] == 0
        # the first call: one read, hits + misses = the frames the located ranges touch
        staged, decoded, _, passes = _sweep(need, WARM, fs, U, staging)
        assert (staged, decoded) == (4, 2)
        got = _h_read_raw(zra, h, idx, buf, NF, numbers, len(want) + 5, staging)
        assert got["st"] == (0, 0) and got["size"] == plain["size"] == len(want), (staging, got["st"])
        assert got["data"] == plain["data"] and got["data"][len(want):] == bytes([SENT]) * 5 and got["sentinel_ok"], staging
        assert got["ranges"] == plain["ranges"] == RM.locate(m.data, NL, numbers)
        s = h.stats()
        miss = [f for f in touched if f not in WARM]
        assert (s["reads"], s["hits"], s["misses"]) == (cache["reads"] + 1, cache["hits"] + len(touched) - len(miss), cache["misses"] + len(miss)), s
        assert s["resident"] == 12 and s["evictions"] == len(miss), s
        assert h.record_stats() == dict(calls=1, staged=staged, decoded=decoded, passes=passes, staged_total=staged, decoded_total=decoded)
        rs = gpu_engine.read_records_stats()
        assert rs == dict(frames=NF, records=len(numbers), packed_bytes=len(want), locate_decoded=decoded, read_decoded=len(miss), locate_passes=passes), rs
        # the second identical call: every touched frame is resident, neither sweep launches the decoder
        got = _h_read_raw(zra, h, idx, buf, NF, numbers, len(want) + 5, staging, ranges=False)
        assert got["st"] == (0, 0) and got["data"] == plain["data"] and got["untouched"], staging
        s2 = h.stats()
        assert (s2["reads"], s2["hits"], s2["misses"], s2["evictions"]) == (s["reads"] + 1, s["hits"] + len(touched), s["misses"], s["evictions"]), s2
        assert gpu_engine.kernel_stats()["dec_launches"] == 0
        r2 = h.record_stats()
        assert (r2["calls"], r2["staged"], r2["decoded"]) == (2, len(need), 0), r2
        rs = gpu_engine.read_records_stats()
        assert (rs["locate_decoded"], rs["read_decoded"]) == (0, 0), rs
        h.close()


def test_read_with_three_slots_and_a_read_that_ends_at_the_content(zra, gpu_engine, shape):
    fs, U, m, A, d, idx, buf = (shape[k] for k in ("fs", "U", "m", "A", "d", "idx", "buf"))
    numbers = [m.inside(f)[0] for f in range(1, 39, 2)] + [_requests(m, fs)[0]]
    touched = m.fetch_frames(numbers)
    assert len(touched) >= 20
    want = RM.packed(m.data, NL, numbers)
    h = _open_warm(zra, gpu_engine, d, A[1], fs, U, warm=(21, 3, 11), slots=3)
    _resident_ok(h, 3)
    for staging in (0, 2 * fs):
        got = _h_read_raw(zra, h, idx, buf, NF, numbers, len(want), staging)
        assert got["st"] == (0, 0) and got["data"] == want and got["sentinel_ok"] and got["ranges"] == RM.locate(m.data, NL, numbers), staging
        s = h.stats()
        assert s["slots"] == 3 and s["resident"] <= 3, s
    assert s["reads"] == 3 + 2 and s["hits"] + s["misses"] == 3 + 2 * len(touched), s
    h.close()
    # a record whose delimiter is content byte U - 1: the fetch's last query ends AT the content's end
    plain = b"ab\ncd\nefg\n" * 300
    x = _compress(gpu_engine, zra, plain, 3, 1000, True)
    B = (_dev(x), len(x))
    i2, b2 = _plain_index(gpu_engine, zra, B, 3)
    R = i2.records
    nums = [R - 1, 0, R - 1]
    want = RM.packed(plain, NL, nums)
    for slots in (2, 0):
        with zra.Archive(gpu_engine, B[0].data_ptr(), B[1], slots * 1000) as h2:
            for _ in range(2):
                got = _h_read_raw(zra, h2, i2, b2, 3, nums, len(want))
                assert got["st"] == (0, 0) and got["data"] == want and want.endswith(b"efg\n") and got["sentinel_ok"], (slots, got["st"])
            assert h2.stats()["reads"] == 2


# ---- 4
def test_after_an_update_the_touched_frames_are_indexed_from_the_cache(zra, gpu_engine, shape):
    import torch
    fs, U, data, arc = shape["fs"], shape["U"], shape["data"], shape["arc"]
    d = _dev(arc)
    idx, buf = _plain_index(gpu_engine, zra, (d, len(arc)), NF, cap=NF + 1)    # the old index, with room for the appended frame's word
    h = _open_warm(zra, gpu_engine, d, len(arc), fs, U)
    _resident_ok(h)
    writes = [(6 * fs + 100, b"\n\nNEW-IN-RESIDENT-SIX\n\n"), (10 * fs + 50, b"NEW\nIN\nMISSING\nTEN\n"), (20 * fs + 7, b"\n\n\nNEW-IN-RESIDENT-TWENTY\n\n\n")]
    app = bytes(G._lines(np.random.RandomState(17), fs))
    new = bytearray(data)
    for off, b in writes:
        new[off:off + len(b)] = b
    new = bytes(new) + app
    m2 = Model(new, fs)
    assert m2.F == NF + 1 and all(m2.words[f] != shape["m"].words[f] for f in (6, 10, 20, 39))
    blob = _dev(b"".join(b for _, b in writes))
    d_app = _dev(app)
    cap = len(arc) + zra.GetOutputBufferSize(len(new), fs) + 64
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    offs, sizes = [o for o, _ in writes], [len(b) for _, b in writes]
    new_size = h.update(d_out.data_ptr(), cap, writes=(offs, sizes, [0, sizes[0], sizes[0] + sizes[1]]), d_data=blob.data_ptr(), d_append=d_app.data_ptr(),
                        append_size=len(app))
    cache = _resident_ok(h)
    # the words of the touched frame range [6, 40], through the handle, into the old buffer
    frames = list(range(6, NF + 1))
    staged, decoded, _, _ = _sweep(frames, WARM, fs, len(new), 0)
    assert 6 in WARM and 20 in WARM and 39 in WARM and 10 not in WARM and (staged, decoded) == (9, 26)
    got = _h_index_raw(zra, h, NL, first=6, staging=3 * fs, cap=NF + 1, buf=buf)
    assert got["st"] == (0, 0), got["st"]
    assert got["words"] == m2.words + [SENTW] * EXTRA
    assert got["info"] == (len(new), fs, NL, NF + 1, m2.D, m2.R)
    r = h.record_stats()
    assert (r["staged"], r["decoded"], r["passes"]) == (staged, decoded, -(-len(frames) // 3)), r
    assert h.stats() == cache
    # the records in those frames are the new bytes
    idx2 = zra.RecordIndex(*got["info"])
    rec_at = lambda pos: next(k for k in range(1, m2.D) if m2.t[k - 1] < pos <= m2.t[k])
    numbers = [rec_at(6 * fs + 103), rec_at(6 * fs + 103) + 2, rec_at(10 * fs + 51), rec_at(10 * fs + 60), rec_at(20 * fs + 12), m2.D, m2.inside(40)[0]]
    B = (d_out, new_size)
    plain = _locate_raw(gpu_engine, zra, B, idx2, buf, NF + 1, numbers)
    q = _h_locate_raw(zra, h, idx2, buf, NF + 1, numbers)
    assert q["st"] == (0, 0) and q["ranges"] == plain["ranges"] == RM.locate(new, NL, numbers)
    r = h.record_stats()
    need = m2.boundary_frames(numbers)
    assert {6, 10, 20} <= set(need) and (r["staged"], r["decoded"]) == _sweep(need, WARM, fs, len(new), 0)[:2] and r["staged"] >= 2, (r, need)
    want = RM.packed(new, NL, numbers)
    q = _h_read_raw(zra, h, idx2, buf, NF + 1, numbers, len(want))
    assert q["st"] == (0, 0) and q["data"] == want and q["sentinel_ok"]
    assert b"NEW-IN-RESIDENT-SIX\n" in want and b"MISSING\n" in want and b"NEW-IN-RESIDENT-TWENTY\n" in want
    h.close()


# ---- 5
def test_a_stale_word_of_a_resident_frame_is_found(zra, gpu_engine, shape):
    import torch
    fs, m, idx, buf, h = (shape[k] for k in ("fs", "m", "idx", "buf", "h"))
    k = m.inside(6)[1]
    assert 6 in WARM
    before, rec = _resident_ok(h), h.record_stats()
    for wrong in (m.words[6] + 1, m.words[6] ^ RM.BIT63):
        w = list(m.words)
        w[6] = wrong
        stale = torch.cat([torch.from_numpy(np.array(w, dtype="<u8").view(np.uint8).copy()), torch.full((8 * EXTRA,), SENT, dtype=torch.uint8)]).to("cuda:0")
        for staging in (0, fs):
            q = _h_locate_raw(zra, h, idx, stale, NF, [0, k], staging)
            assert q["st"] == (1, 20) and q["untouched"], (wrong, staging, q["st"])
            assert gpu_engine.locate_records_stats() == LOCATE_ZERO
            q = _h_read_raw(zra, h, idx, stale, NF, [k], 4096, staging)
            assert q["st"] == (1, 20) and q["untouched"] and q["all_sentinel"] and q["size"] == 0, (wrong, staging, q["st"])
            assert h.record_stats() == rec and h.stats() == before
    assert _h_locate_raw(zra, h, idx, buf, NF, [0, k])["ranges"] == RM.locate(m.data, NL, [0, k])   # the right word serves the same request


# ---- 6
def test_a_damaged_missing_frame_ends_locate_and_read_and_changes_nothing(zra, gpu_engine, shape):
    fs, U, m, arc, idx, buf = (shape[k] for k in ("fs", "U", "m", "arc", "idx", "buf"))
    e_hs = _flip_mid(arc, [12])
    from verify_model import entries, fields
    two = bytearray(e_hs)
    two[fields(arc)[0] + entries(arc)[30]] ^= 0xFF                             # frame 30: its first byte, another kind of damage
    two = bytes(two)
    for bad, damaged in ((e_hs, [12]), (two, [12, 30])):
        db = _dev(bad)
        want = _frame_status(gpu_engine, zra, bad, frames=[11, 12, 13, 29, 30, 31], d_arc=db)
        assert sorted(want) == damaged and all(want.values()), want
        assert len(damaged) == 1 or want[12] != want[30], want                # else the lower frame could not be told from the higher
        h = _open_warm(zra, gpu_engine, db, len(bad), fs, U)                   # the same warmed set: frames 12 and 30 are not resident
        cache, rec = _resident_ok(h), h.record_stats()
        numbers = [m.inside(30)[0], m.inside(6)[0], m.inside(12)[0], 0]
        assert m.boundary_frames(numbers) == [0, 6, 12, 30]
        for staging in (0, fs, 3 * fs):                                        # one pass; every frame its own; 12 and 30 in different passes
            q = _h_locate_raw(zra, h, idx, buf, NF, numbers, staging)
            assert q["st"] == (1, want[12]) and q["untouched"], (damaged, staging, q["st"], want)
            assert gpu_engine.locate_records_stats() == LOCATE_ZERO
            q = _h_read_raw(zra, h, idx, buf, NF, numbers, 8192, staging)
            assert q["st"] == (1, want[12]) and q["untouched"] and q["all_sentinel"] and q["size"] == 0, (damaged, staging, q["st"])
            assert gpu_engine.read_records_stats() == READ_ZERO
            assert h.stats() == cache and h.record_stats() == rec, (damaged, staging)
        ok = [m.inside(6)[0], m.inside(13)[0], 0]                              # beside the damage every call succeeds
        assert _h_locate_raw(zra, h, idx, buf, NF, ok)["ranges"] == RM.locate(m.data, NL, ok)
        assert h.stats() == cache
        h.close()


# ---- 7
def test_a_handle_without_slots_is_the_plain_call(zra, gpu_engine, shape):
    fs, U, m, A, d, idx, buf = (shape[k] for k in ("fs", "U", "m", "A", "d", "idx", "buf"))
    _, asc = _requests(m, fs)
    want = RM.packed(m.data, NL, asc)

    def launches():
        k = gpu_engine.kernel_stats()
        return k["mf_launches"], k["ent_launches"], k["dec_launches"]

    with zra.Archive(gpu_engine, d.data_ptr(), A[1], 0) as h0:
        for staging in (0, 3 * fs):
            plain = _index_raw(gpu_engine, zra, A, NL, first=2, count=9, staging=staging, cap=NF)
            ps, pl = gpu_engine.index_records_stats(), launches()
            got = _h_index_raw(zra, h0, NL, first=2, count=9, staging=staging, cap=NF)
            assert (got["st"], got["words"], got["info"]) == (plain["st"], plain["words"], plain["info"]) and got["st"] == (0, 0), staging
            assert gpu_engine.index_records_stats() == ps and launches() == pl, staging
            r = h0.record_stats()
            assert (r["staged"], r["decoded"], r["passes"], r["staged_total"]) == (0, 9, ps["passes"], 0), r
            plain = _locate_raw(gpu_engine, zra, A, idx, buf, NF, asc, staging)
            ps, pl = gpu_engine.locate_records_stats(), launches()
            got = _h_locate_raw(zra, h0, idx, buf, NF, asc, staging)
            assert got["st"] == (0, 0) and got["ranges"] == plain["ranges"] and gpu_engine.locate_records_stats() == ps and launches() == pl, staging
            r = h0.record_stats()
            assert (r["staged"], r["decoded"], r["passes"]) == (0, ps["decoded"], ps["passes"]), r
            plain = _read_raw(gpu_engine, zra, A, idx, buf, NF, asc, len(want), staging)
            ps, pl = gpu_engine.read_records_stats(), launches()
            got = _h_read_raw(zra, h0, idx, buf, NF, asc, len(want), staging)
            assert got["st"] == (0, 0) and got["data"] == plain["data"] == want and got["ranges"] == plain["ranges"], staging
            assert gpu_engine.read_records_stats() == ps and launches() == pl, (staging, gpu_engine.read_records_stats(), ps)
            assert h0.record_stage_ms() == 0
        s = h0.stats()
        assert (s["slots"], s["resident"], s["reads"], s["hits"]) == (0, 0, 2, 0) and s["misses"] == 2 * len(m.fetch_frames(asc)), s
        assert h0.record_stats()["staged_total"] == 0


# ---- 8
def test_refusals_leave_every_counter_alone(zra, gpu_engine, shape):
    fs, U, m, d, idx, buf, h = (shape[k] for k in ("fs", "U", "m", "d", "idx", "buf", "h"))
    cache, rec = _resident_ok(h), h.record_stats()

    def unchanged(tag):
        assert h.stats() == cache and h.record_stats() == rec, tag

    for other, want in ((idx._replace(content_size=U - 1), (1, 40)), (idx._replace(frame_size=2 * fs, frames=-(-U // (2 * fs))), (1, 40)),
                        (idx._replace(frames=NF + 1), (1, 42)), (idx._replace(delimiter=256), (1, 42))):
        q = _h_locate_raw(zra, h, other, buf, NF + 1, [0])
        assert q["st"] == want and q["untouched"], (other, q["st"])
        q = _h_read_raw(zra, h, other, buf, NF + 1, [0], 4096)
        assert q["st"] == want and q["untouched"] and q["all_sentinel"] and q["size"] == 0, (other, q["st"])
        unchanged(other)
    for numbers in ([m.R], [0, m.R + 7], [ALL]):
        q = _h_locate_raw(zra, h, idx, buf, NF, numbers)
        assert q["st"] == OOB and q["untouched"], (numbers, q["st"])
        q = _h_read_raw(zra, h, idx, buf, NF, numbers, 4096)
        assert q["st"] == OOB and q["untouched"] and q["all_sentinel"] and q["size"] == 0, (numbers, q["st"])
        assert gpu_engine.locate_records_stats() == LOCATE_ZERO and gpu_engine.read_records_stats() == READ_ZERO
        unchanged(numbers)
    # the index inside the archive; the packed data inside the archive and inside the index
    q = _h_index_raw(zra, h, NL, cap=NF, buf=buf, d_index=d.data_ptr() + 8)
    assert q["st"] == (1, 42) and q["info"] == (0,) * 6 and q["words"][:NF] == m.words and gpu_engine.index_records_stats() == INDEX_ZERO, q["st"]
    unchanged("index")
    for d_data in (d.data_ptr() + 100, buf.data_ptr() + 8):
        q = _h_read_raw(zra, h, idx, buf, NF, [0, 1], 64, d_data=d_data)
        assert q["st"] == (1, 42) and q["size"] == 0 and q["untouched"], q["st"]
        unchanged(d_data)
    for first, count in ((NF + 1, 0), (NF, 1), (0, NF + 1)):
        q = _h_index_raw(zra, h, NL, first=first, count=count, cap=NF)
        assert q["st"] == OOB and q["info"] == (0,) * 6 and q["words"] == [SENTW] * (NF + EXTRA), (first, count, q["st"])
        unchanged((first, count))
    q = _h_index_raw(zra, h, NL, cap=NF - 1)                                   # the sizing call
    assert q["st"] == TOO_SMALL and q["info"] == (U, fs, NL, NF, 0, 0) and q["words"] == [SENTW] * (NF - 1 + EXTRA), q
    unchanged("sizing")
    assert _words(buf)[:NF] == m.words


# ---- shape B
@pytest.fixture(scope="module")
def shape_b(zra, gpu_engine):
    """12 frames of 20,000 bytes: tiles at 8,192 and 16,384, the third tile of 3,616 bytes; 5 frames resident. Delimiters on both sides
    of every tile edge and frame edge of resident frame 4 and of missing frame 5, and a few more in every tile of every frame."""
    fs, F = 20000, 12
    U = (F - 1) * fs + 7123
    at = set()
    for f in range(F):
        for x in (0, 100, 5000, 8191, 8192, 8300, 12000, 16383, 16384, 16500, 19000, 19999):
            if f * fs + x < U - 1:
                at.add(f * fs + x)
    data = _placed(3, U, NL, sorted(at))
    arc = _compress(gpu_engine, zra, data, 3, fs, True)
    d = _dev(arc)
    warm = (9, 4, 0, 7, 2)
    h = _open_warm(zra, gpu_engine, d, len(arc), fs, U, warm=warm, slots=5)
    _resident_ok(h, 5)
    idx, buf = _plain_index(gpu_engine, zra, (d, len(arc)), F)
    yield dict(fs=fs, F=F, U=U, data=data, m=Model(data, fs), A=(d, len(arc)), idx=idx, buf=buf, h=h, warm=warm)
    h.close()


def test_three_tiles_per_frame(zra, gpu_engine, shape_b):
    fs, F, U, m, A, idx, buf, h, warm = (shape_b[k] for k in ("fs", "F", "U", "m", "A", "idx", "buf", "h", "warm"))
    cache = _resident_ok(h, 5)
    for staging in (0, 2 * fs):
        plain = _index_raw(gpu_engine, zra, A, NL, staging=staging, cap=F)
        got = _h_index_raw(zra, h, NL, staging=staging, cap=F)
        assert got["st"] == (0, 0) and got["words"] == plain["words"] == m.words + [SENTW] * EXTRA and got["info"] == plain["info"], staging
        r = h.record_stats()
        assert (r["staged"], r["decoded"], r["passes"]) == (5, 7, 6 if staging else 1), r
    # a request for every delimiter of resident frame 4 and of missing frame 5: boundaries in each of the three tiles of both
    numbers = [k for k in range(1, m.D) if m.t[k] // fs in (4, 5)]
    tiles = {(m.t[k] // fs, m.t[k] % fs // 8192) for k in numbers}
    assert tiles == {(f, t) for f in (4, 5) for t in (0, 1, 2)}
    numbers = numbers[::-1] + [0, m.D]
    need = m.boundary_frames(numbers)
    assert need == [0, 3, 4, 5, 11]
    for staging in (0, fs):
        plain = _locate_raw(gpu_engine, zra, A, idx, buf, F, numbers, staging)
        got = _h_locate_raw(zra, h, idx, buf, F, numbers, staging)
        assert got["st"] == (0, 0) and got["ranges"] == plain["ranges"] == RM.locate(m.data, NL, numbers), staging
        r = h.record_stats()
        assert (r["staged"], r["decoded"]) == _sweep(need, warm, fs, U, staging)[:2] == (2, 3), r
        hs = gpu_engine.locate_records_stats()
        assert (hs["decoded"], hs["content_bytes"]) == (3, 2 * fs + _flen(11, fs, U)), hs
    assert h.stats() == cache
    want = RM.packed(m.data, NL, numbers)
    got = _h_read_raw(zra, h, idx, buf, F, numbers, len(want), fs)
    assert got["st"] == (0, 0) and got["data"] == want and got["sentinel_ok"]
    s = h.stats()
    touched = m.fetch_frames(numbers)
    assert s["reads"] == cache["reads"] + 1 and s["hits"] + s["misses"] == cache["hits"] + cache["misses"] + len(touched) and s["resident"] == 5, s
