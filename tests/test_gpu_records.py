"""GPU tests of the record index (include/zra_hip.h: ZraHipIndexRecords, ZraHipLocateRecords, ZraHipReadRecords). The yardstick is
tests/records_model.py over the plaintext the test generated itself (cross-checked against the grep's and the extract's models in
tests/test_records_abi.py); for a frame that does not decode, the status ZraHipDecompressRABatch gives under
ZRA_HIP_OPT_RA_WHOLE_FRAMES for a query inside it. The shapes are the smallest at which each seam exists: a frame size that is no
power of two (1,000), one of three tiles with a short last one (20,000), delimiters on both sides of every frame and tile edge. Every
device buffer is followed by a sentinel that no call may touch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import corpus as C
import records_model as RM
from test_gpu_update import _compress, _data, _dev, _update
from test_gpu_verify import _flip_mid, _frame_status

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "zra_amd", "tools", "zratool_amd")
SENT = 0xA5
SENTW = int.from_bytes(bytes([SENT]) * 8, "little")
EXTRA = 4                                                                      # sentinel words behind an index buffer
TOO_SMALL = (6, 0)
OOB = (5, 0)
ALL = 0xFFFFFFFFFFFFFFFF
NL = 0x0A
INDEX_ZERO = dict.fromkeys(("frames", "indexed", "content_bytes", "delimiters", "passes"), 0)
LOCATE_ZERO = dict.fromkeys(("frames", "records", "boundaries", "decoded", "content_bytes", "passes"), 0)
READ_ZERO = dict.fromkeys(("frames", "records", "packed_bytes", "locate_decoded", "read_decoded", "locate_passes"), 0)


def _filler(seed, n, delim):
    """compressible bytes without the delimiter"""
    a = np.frombuffer(_data(np.random.RandomState(seed), n), dtype=np.uint8).copy()
    a[a == delim] = 0x40
    return a


def _placed(seed, n, delim, at):
    a = _filler(seed, n, delim)
    a[list(at)] = delim
    return a.tobytes()


def _frames_of(n, fs):
    return -(-n // fs)


def _idxbuf(words):
    import torch
    return torch.full((8 * (words + EXTRA),), SENT, dtype=torch.uint8, device="cuda:0")


def _words(buf):
    return [int(x) for x in np.frombuffer(buf.cpu().numpy().tobytes(), dtype="<u8")]


def _index_raw(eng, zra, A, delim, first=0, count=ALL, staging=0, cap=None, buf=None, d_index=None, frames=None):
    """One ZraHipIndexRecords into a buffer of `cap` words (None: `frames`) with EXTRA sentinel words behind it."""
    import torch
    if cap is None:
        cap = frames
    if buf is None:
        buf = _idxbuf(cap)
    torch.cuda.synchronize()
    info = zra.ZraHipRecordIndex(1, 2, 3, 4, 5, 6)
    eng._order()
    st = zra.load().ZraHipIndexRecords(eng.h, A[0].data_ptr() if A[0] is not None else None, A[1], delim, first, count, staging,
                                       (buf.data_ptr() if cap else None) if d_index is None else d_index, cap, ctypes.byref(info)).tup()
    return dict(st=st, info=(info.contentSize, info.frameSize, info.delimiter, info.frames, info.delimiters, info.records), words=_words(buf), buf=buf, cap=cap)


def _locate_raw(eng, zra, A, info, buf, index_words, numbers, staging=0):
    """One ZraHipLocateRecords; the host array is pre-filled with 0xEE. dict: st, ranges, raw."""
    import torch
    n = len(numbers)
    nums = (ctypes.c_uint64 * max(n, 1))(*numbers)
    out = (ctypes.c_uint64 * (2 * n + 2))()
    ctypes.memset(out, 0xEE, ctypes.sizeof(out))
    torch.cuda.synchronize()
    ci = zra.ZraHipRecordIndex(*info)
    eng._order()
    st = zra.load().ZraHipLocateRecords(eng.h, A[0].data_ptr(), A[1], ctypes.byref(ci), buf.data_ptr() if buf is not None else None, index_words, nums, n, staging,
                                        out).tup()
    raw = bytes(out)
    return dict(st=st, ranges=[(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)], untouched=raw == b"\xEE" * len(raw), tail_ok=raw[16 * n:] == b"\xEE" * 16)


def _read_raw(eng, zra, A, info, buf, index_words, numbers, dcap, staging=0, d_data=None, ranges=True):
    import torch
    n = len(numbers)
    nums = (ctypes.c_uint64 * max(n, 1))(*numbers)
    out = (ctypes.c_uint64 * (2 * n + 2))()
    ctypes.memset(out, 0xEE, ctypes.sizeof(out))
    dbuf = torch.full((dcap + 64,), SENT, dtype=torch.uint8, device="cuda:0") if d_data is None else None
    torch.cuda.synchronize()
    ci = zra.ZraHipRecordIndex(*info)
    size = ctypes.c_uint64(0x1234)
    eng._order()
    st = zra.load().ZraHipReadRecords(eng.h, A[0].data_ptr(), A[1], ctypes.byref(ci), buf.data_ptr(), index_words, nums, n, staging, out if ranges else None,
                                      (dbuf.data_ptr() if dcap else None) if d_data is None else d_data, dcap, ctypes.byref(size)).tup()
    raw = bytes(out)
    data = dbuf.cpu().numpy().tobytes() if dbuf is not None else b""
    return dict(st=st, size=size.value, ranges=[(int(out[2 * i]), int(out[2 * i + 1])) for i in range(n)], untouched=raw == b"\xEE" * len(raw),
                data=data[:dcap], sentinel_ok=data[dcap:] == bytes([SENT]) * 64 if dbuf is not None else True,
                all_sentinel=data == bytes([SENT]) * (dcap + 64) if dbuf is not None else True)


def _indexed(eng, zra, A, plain, fs, delim, staging=0):
    """index of the whole archive, checked word for word and total for total against the model; returns (RecordIndex, buffer)"""
    want = RM.index_words(plain, fs, delim)
    D, R = RM.counts(plain, delim)
    F = _frames_of(len(plain), fs)
    r = _index_raw(eng, zra, A, delim, staging=staging, frames=F)
    assert r["st"] == (0, 0), (fs, staging, r["st"])
    assert r["info"] == (len(plain), fs, delim, F, D, R), (r["info"], D, R)
    assert r["words"][:F] == want, (fs, staging, [i for i in range(F) if r["words"][i] != want[i]][:8])
    assert r["words"][F:] == [SENTW] * EXTRA
    slots = 65536 if staging == 0 else max(1, staging // fs)
    assert eng.index_records_stats() == dict(frames=F, indexed=F, content_bytes=len(plain), delimiters=D, passes=-(-F // slots)), eng.index_records_stats()
    return zra.RecordIndex(*r["info"]), r["buf"]


def _arc(eng, zra, plain, fs):
    x = _compress(eng, zra, plain, 3, fs, True)
    return x, (_dev(x), len(x))


def _located(eng, zra, A, idx, buf, plain, delim, numbers, staging=0):
    want = RM.locate(plain, delim, numbers)
    r = _locate_raw(eng, zra, A, idx, buf, idx.frames, numbers, staging)
    assert r["st"] == (0, 0), (staging, r["st"])
    bad = [i for i in range(len(numbers)) if r["ranges"][i] != want[i]]
    assert not bad, (staging, [(numbers[i], r["ranges"][i], want[i]) for i in bad[:6]], len(bad))
    assert r["tail_ok"]
    return r


def _read(eng, zra, A, idx, buf, plain, delim, numbers, staging=0):
    want = RM.packed(plain, delim, numbers)
    r = _read_raw(eng, zra, A, idx, buf, idx.frames, numbers, len(want) + 5, staging)
    assert r["st"] == (0, 0), (staging, r["st"])
    assert r["size"] == len(want)
    assert r["data"][:len(want)] == want, (staging, next(i for i in range(len(want)) if r["data"][i] != want[i]))
    assert r["data"][len(want):] == bytes([SENT]) * 5 and r["sentinel_ok"]
    assert r["ranges"] == RM.locate(plain, delim, numbers)
    return r


def _whole(eng, zra, plain, fs, delim):
    """everything the issue lists for one content: the index at three window sizes, the locate in three orders and at three window
    sizes, the edges of the numbering, the read"""
    x, A = _arc(eng, zra, plain, fs)
    for staging in (fs, 2 * fs, 0):
        idx, buf = _indexed(eng, zra, A, plain, fs, delim, staging)
    D, R = RM.counts(plain, delim)
    assert (idx.delimiters, idx.records) == (D, R)
    asc = list(range(R))
    for staging in (0, fs, 2 * fs):
        _located(eng, zra, A, idx, buf, plain, delim, asc, staging)
    desc = asc[::-1] + asc[:3] + asc[-3:]
    _located(eng, zra, A, idx, buf, plain, delim, desc, fs)
    if R:
        _located(eng, zra, A, idx, buf, plain, delim, [0])
        _located(eng, zra, A, idx, buf, plain, delim, [R - 1])
    for numbers in ([R], [0, R] if R else [5], [ALL]):
        r = _locate_raw(eng, zra, A, idx, buf, idx.frames, numbers)
        assert r["st"] == OOB and r["untouched"], (numbers, r["st"])
        assert eng.locate_records_stats() == LOCATE_ZERO
    _read(eng, zra, A, idx, buf, plain, delim, asc)
    _read(eng, zra, A, idx, buf, plain, delim, desc, fs)
    if R:
        _read(eng, zra, A, idx, buf, plain, delim, [R - 1])
    assert _words(buf)[idx.frames:] == [SENTW] * EXTRA
    return x, A, idx, buf


# hand-placed delimiters at frame size 1,000: the last byte of frame 0 and the first of frame 1, two in a row, a record that spans
# frames 3, 4 and 5 without a delimiter, delimiters on both sides of it
AT1000 = (0, 17, 999, 1000, 1500, 1501, 2999, 6200, 6201, 7100)
# at frame size 20,000 (tiles at 8,192 and 16,384; the third tile holds 3,616 bytes): the last and the first byte of a tile, the last
# byte of a frame and the first of the next, the last byte of a short last tile
AT20000 = (8191, 8192, 16383, 16384, 19999, 20000, 28191, 28192, 36383, 39999, 40001, 45000)


# ---- 1
@pytest.mark.parametrize("tail", ["open", "closed"])
def test_frame_size_1000(zra, gpu_engine, tail):
    """U is no multiple of the frame size; the content ends in a delimiter (closed) or not (open)"""
    U = 7300
    at = AT1000 + ((U - 1,) if tail == "closed" else ())
    plain = _placed(1, U, NL, at)
    _, _, idx, _ = _whole(gpu_engine, zra, plain, 1000, NL)
    assert idx.delimiters == len(at) and idx.records == len(at) + (tail == "open")


# ---- 2
@pytest.mark.parametrize("tail", ["open", "closed"])
def test_frame_size_20000_tile_edges(zra, gpu_engine, tail):
    U = 47123
    at = AT20000 + ((U - 1,) if tail == "closed" else ())
    plain = _placed(2, U, NL, at)
    _, _, idx, _ = _whole(gpu_engine, zra, plain, 20000, NL)
    assert idx.delimiters == len(at)


# ---- 3
def test_one_frame_and_no_content(zra, gpu_engine):
    """U = fs: one frame. U = 0: no frame, R = 0, every number is out of bounds, the index is Success with 0 words"""
    plain = _placed(3, 1000, NL, (0, 500, 999))
    _whole(gpu_engine, zra, plain, 1000, NL)
    x, A = _arc(gpu_engine, zra, b"", 1000)
    r = _index_raw(gpu_engine, zra, A, NL, frames=0)
    assert r["st"] == (0, 0) and r["info"] == (0, 1000, NL, 0, 0, 0) and r["words"] == [SENTW] * EXTRA, r
    idx = zra.RecordIndex(*r["info"])
    for numbers in ([0], [1, 0], [ALL]):
        q = _locate_raw(gpu_engine, zra, A, idx, r["buf"], 0, numbers)
        assert q["st"] == OOB and q["untouched"]
        q = _read_raw(gpu_engine, zra, A, idx, r["buf"], 0, numbers, 16)
        assert q["st"] == OOB and q["untouched"] and q["all_sentinel"] and q["size"] == 0
    q = _read_raw(gpu_engine, zra, A, idx, r["buf"], 0, [], 16)
    assert q["st"] == (0, 0) and q["size"] == 0 and q["all_sentinel"]


# ---- 4
def test_nothing_but_delimiters(zra, gpu_engine):
    """delimiter 0x00 in zeros: 8,192 delimiters per tile, every record empty, the content ends in a delimiter"""
    plain = bytes(20000 + 500)
    _, _, idx, _ = _whole(gpu_engine, zra, plain, 20000, 0)
    assert idx.delimiters == idx.records == len(plain)


# ---- 5
@pytest.mark.parametrize("delim", [NL, 0x00])
def test_loglike(zra, gpu_engine, delim):
    plain = C.gen_loglike(30000)[:29876]
    _whole(gpu_engine, zra, plain, 1000, delim)


@pytest.fixture(scope="module")
def twelve(zra, gpu_engine):
    """12 frames of 1,000 bytes of log lines, indexed once"""
    plain = C.gen_loglike(12000)[:12000]
    x, A = _arc(gpu_engine, zra, plain, 1000)
    idx, buf = _indexed(gpu_engine, zra, A, plain, 1000, NL)
    return dict(plain=plain, arc=x, A=A, idx=idx, buf=buf)


# ---- 6
def test_index_sizing_and_sub_range(zra, gpu_engine, twelve):
    plain, A = twelve["plain"], twelve["A"]
    want = RM.index_words(plain, 1000, NL)
    for cap in (0, 11):
        r = _index_raw(gpu_engine, zra, A, NL, cap=cap)
        assert r["st"] == TOO_SMALL and r["info"] == (12000, 1000, NL, 12, 0, 0), r["info"]
        assert r["words"] == [SENTW] * (cap + EXTRA)
        assert gpu_engine.index_records_stats() == INDEX_ZERO
    # a sub-range writes its words only
    r = _index_raw(gpu_engine, zra, A, NL, first=4, count=3, frames=12, staging=2000)
    assert r["st"] == (0, 0)
    assert r["words"] == [SENTW] * 4 + want[4:7] + [SENTW] * (5 + EXTRA)
    assert gpu_engine.index_records_stats() == dict(frames=12, indexed=3, content_bytes=3000, delimiters=sum(w & (RM.BIT63 - 1) for w in want[4:7]), passes=2)
    # the rest of the frames into the same buffer: the totals are those of the whole content
    r = _index_raw(gpu_engine, zra, A, NL, first=0, count=4, buf=r["buf"], cap=12)
    assert r["st"] == (0, 0)
    r = _index_raw(gpu_engine, zra, A, NL, first=7, buf=r["buf"], cap=12)
    assert r["st"] == (0, 0) and r["words"] == want + [SENTW] * EXTRA
    assert r["info"] == (12000, 1000, NL, 12) + RM.counts(plain, NL)
    # the empty range is Success; a range outside the frames is not
    r2 = _index_raw(gpu_engine, zra, A, NL, first=12, count=0, buf=r["buf"], cap=12)
    assert r2["st"] == (0, 0) and r2["words"] == want + [SENTW] * EXTRA
    for first, count in ((13, 0), (12, 1), (0, 13)):
        r2 = _index_raw(gpu_engine, zra, A, NL, first=first, count=count, buf=r["buf"], cap=12)
        assert r2["st"] == OOB and r2["info"] == (0,) * 6 and r2["words"] == want + [SENTW] * EXTRA
    # the index inside the archive
    r2 = _index_raw(gpu_engine, zra, A, NL, d_index=A[0].data_ptr() + 8, cap=12, buf=r["buf"])
    assert r2["st"] == (1, 42) and r2["info"] == (0,) * 6


# ---- 7
def test_cost_follows_the_records(zra, gpu_engine, twelve):
    """records that all lie in one frame of the 12 decode exactly that frame"""
    plain, A, idx, buf = (twelve[k] for k in ("plain", "A", "idx", "buf"))
    recs = RM.locate(plain, NL, range(idx.records))
    inside = [k for k, (s, n) in enumerate(recs) if s > 7000 and s + n < 7999]
    assert len(inside) >= 3
    _located(gpu_engine, zra, A, idx, buf, plain, NL, inside + inside[::-1])
    s = gpu_engine.locate_records_stats()
    assert s == dict(frames=12, records=2 * len(inside), boundaries=4 * len(inside), decoded=1, content_bytes=1000, passes=1), s
    _read(gpu_engine, zra, A, idx, buf, plain, NL, inside)
    s = gpu_engine.read_records_stats()
    assert s["locate_decoded"] == 1 and s["read_decoded"] >= 1 and s["records"] == len(inside) and s["locate_passes"] == 1, s
    assert gpu_engine.locate_records_stats()["decoded"] == 1                   # the read leaves the locate's counters alone
    # several passes: a window of one and of two needed frames
    spread = [0, idx.records - 1, inside[0]]
    for staging, passes in ((1000, 3), (2000, 2)):
        _located(gpu_engine, zra, A, idx, buf, plain, NL, spread, staging)
        s = gpu_engine.locate_records_stats()
        assert s["decoded"] == 3 and s["passes"] == passes, s


# ---- 8
def test_stale_index_and_refresh(zra, gpu_engine, twelve):
    plain, x, A, idx = (twelve[k] for k in ("plain", "arc", "A", "idx"))
    r = _index_raw(gpu_engine, zra, A, NL, frames=12, cap=16)                  # a buffer with room for the frames an append adds
    buf = r["buf"]
    recs = RM.locate(plain, NL, range(idx.records))
    k = next(k for k, (s, n) in enumerate(recs) if 5000 < s + n < 5900)        # its delimiter lies in frame 5
    t = recs[k][0] + recs[k][1]
    st, out, size = _update(gpu_engine, zra, x, [(t, b"x")])
    assert st == (0, 0)
    y = out[:size]
    B = (_dev(y), len(y))
    new = plain[:t] + b"x" + plain[t + 1:]
    q = _locate_raw(gpu_engine, zra, B, idx, buf, 16, [k])
    assert q["st"] == (1, 20) and q["untouched"], q["st"]
    assert gpu_engine.locate_records_stats() == LOCATE_ZERO
    q = _read_raw(gpu_engine, zra, B, idx, buf, 16, [k], 4096)
    assert q["st"] == (1, 20) and q["untouched"] and q["all_sentinel"] and q["size"] == 0
    far = [j for j, (s, n) in enumerate(recs) if s + n < 3000]                 # frames 0..2 are as they were: their records are served
    assert _locate_raw(gpu_engine, zra, B, idx, buf, 16, far)["ranges"] == [recs[j] for j in far]
    r = _index_raw(gpu_engine, zra, B, NL, first=5, count=1, buf=buf, cap=16)
    assert r["st"] == (0, 0) and r["words"][:12] == RM.index_words(new, 1000, NL) and r["words"][12:] == [SENTW] * (4 + EXTRA)
    assert r["info"] == (12000, 1000, NL, 12) + RM.counts(new, NL)
    idx2 = zra.RecordIndex(*r["info"])
    _located(gpu_engine, zra, B, idx2, buf, new, NL, list(range(idx2.records)))
    _read(gpu_engine, zra, B, idx2, buf, new, NL, list(range(idx2.records)))
    # an append: the old words keep their places, the grown last frame is indexed again and the new frames follow
    tail = C.gen_loglike(3000)[200:2900]
    st, out, size = _update(gpu_engine, zra, y, [(11990, b"\n")], append=tail)
    assert st == (0, 0)
    z = out[:size]
    Z = (_dev(z), len(z))
    grown = new[:11990] + b"\n" + new[11991:] + tail
    q = _locate_raw(gpu_engine, zra, Z, idx2, buf, 16, [0])
    assert q["st"] == (1, 40) and q["untouched"]                               # another content size than the index describes
    before = _words(buf)[:11]
    r = _index_raw(gpu_engine, zra, Z, NL, first=11, buf=buf, cap=16)
    assert r["st"] == (0, 0) and r["words"][:11] == before
    assert r["words"][:15] == RM.index_words(grown, 1000, NL) and r["words"][15:] == [SENTW] * (1 + EXTRA)
    assert r["info"] == (len(grown), 1000, NL, 15) + RM.counts(grown, NL)
    idx3 = zra.RecordIndex(*r["info"])
    _located(gpu_engine, zra, Z, idx3, buf, grown, NL, list(range(idx3.records)), 2000)
    _read(gpu_engine, zra, Z, idx3, buf, grown, NL, list(range(idx3.records))[::-1])


# ---- 9
def test_read_capacity_and_overlap(zra, gpu_engine, twelve):
    plain, A, idx, buf = (twelve[k] for k in ("plain", "A", "idx", "buf"))
    numbers = [idx.records - 1, 3, 3, 0]
    want = RM.packed(plain, NL, numbers)
    q = _read_raw(gpu_engine, zra, A, idx, buf, 12, numbers, 0)                 # the sizing call
    assert q["st"] == TOO_SMALL and q["size"] == len(want) and q["untouched"]
    assert gpu_engine.read_records_stats() == READ_ZERO
    q = _read_raw(gpu_engine, zra, A, idx, buf, 12, numbers, len(want) - 1)
    assert q["st"] == TOO_SMALL and q["size"] == len(want) and q["untouched"] and q["all_sentinel"]
    q = _read_raw(gpu_engine, zra, A, idx, buf, 12, numbers, len(want))
    assert q["st"] == (0, 0) and q["data"] == want and q["sentinel_ok"]
    q = _read_raw(gpu_engine, zra, A, idx, buf, 12, numbers, len(want), ranges=False)   # hRanges is optional
    assert q["st"] == (0, 0) and q["data"] == want and q["untouched"]
    for d_data in (A[0].data_ptr() + 100, buf.data_ptr() + 8):
        q = _read_raw(gpu_engine, zra, A, idx, buf, 12, numbers, 64, d_data=d_data)
        assert q["st"] == (1, 42) and q["size"] == 0 and q["untouched"]
    assert _words(buf)[:12] == RM.index_words(plain, 1000, NL)


# ---- 10
def test_open_last_record_and_read_that_ends_at_the_content(zra, gpu_engine):
    """an open last record gets its delimiter byte; the last record of content that ends in a delimiter is a read that ends at U"""
    for plain in (b"ab\ncd\nefg", b"ab\ncd\nefg\n"):
        plain = plain * 300
        x, A = _arc(gpu_engine, zra, plain, 1000)
        idx, buf = _indexed(gpu_engine, zra, A, plain, 1000, NL)
        R = idx.records
        r = _read(gpu_engine, zra, A, idx, buf, plain, NL, [R - 1, R - 1, 0, R - 1])
        assert r["data"][:r["size"]].endswith(b"efg\n")


# ---- 11
def test_damage(zra, gpu_engine, twelve):
    plain, x, idx, buf = (twelve[k] for k in ("plain", "arc", "idx", "buf"))
    bad = _flip_mid(x, [5])
    B = (_dev(bad), len(bad))
    code = _frame_status(gpu_engine, zra, bad, d_arc=B[0])
    assert list(code) == [5]
    r = _index_raw(gpu_engine, zra, B, NL, frames=12)
    assert r["st"] == (1, code[5]) and r["info"] == (0,) * 6 and r["words"][12:] == [SENTW] * EXTRA
    assert gpu_engine.index_records_stats() == INDEX_ZERO
    r = _index_raw(gpu_engine, zra, B, NL, first=6, frames=12)                   # a range without the frame
    assert r["st"] == (0, 0)
    recs = RM.locate(plain, NL, range(idx.records))
    hit = next(k for k, (s, n) in enumerate(recs) if 5000 < s and s + n < 5999)
    miss = [k for k, (s, n) in enumerate(recs) if s + n < 4999 or s > 6000]
    q = _locate_raw(gpu_engine, zra, B, idx, buf, 12, [miss[0], hit])
    assert q["st"] == (1, code[5]) and q["untouched"]
    q = _read_raw(gpu_engine, zra, B, idx, buf, 12, [hit], 4096)
    assert q["st"] == (1, code[5]) and q["untouched"] and q["size"] == 0
    q = _locate_raw(gpu_engine, zra, B, idx, buf, 12, miss)
    assert q["st"] == (0, 0) and q["ranges"] == [recs[k] for k in miss]


# ---- 12
def test_info_mismatch(zra, gpu_engine, twelve):
    plain, A, idx, buf = (twelve[k] for k in ("plain", "A", "idx", "buf"))
    for other, want in ((idx._replace(content_size=11999), (1, 40)), (idx._replace(content_size=11001, frames=12), (1, 40)),
                        (idx._replace(frames=13), (1, 42)), (idx._replace(frames=11), (1, 42)), (idx._replace(frame_size=0), (1, 42)),
                        (idx._replace(delimiter=256), (1, 42)), (idx._replace(frame_size=2000, frames=6), (1, 40))):
        q = _locate_raw(gpu_engine, zra, A, other, buf, 12, [0])
        assert q["st"] == want and q["untouched"], (other, q["st"])
        q = _read_raw(gpu_engine, zra, A, other, buf, 12, [0], 4096)
        assert q["st"] == want and q["untouched"] and q["all_sentinel"], (other, q["st"])
    q = _locate_raw(gpu_engine, zra, A, idx, buf, 11, [0])                      # fewer words than frames
    assert q["st"] == (1, 42) and q["untouched"]
    # the totals in *info are not trusted: R comes from the words
    q = _locate_raw(gpu_engine, zra, A, idx._replace(records=1, delimiters=0), buf, 12, [idx.records - 1])
    assert q["st"] == (0, 0) and q["ranges"] == RM.locate(plain, NL, [idx.records - 1])
    q = _locate_raw(gpu_engine, zra, A, idx._replace(records=idx.records + 9), buf, 12, [idx.records])
    assert q["st"] == OOB and q["untouched"]


# ---- 13
def test_tool_modes(zra, gpu_engine, twelve, tmp_path):
    """zratool_amd ix prints frames, delimiters and records; rr prints the text of records by their number"""
    plain = twelve["plain"]
    path = tmp_path / "log.zra"
    path.write_bytes(twelve["arc"])
    run = lambda *a: subprocess.run([TOOL] + [str(x) for x in a], capture_output=True, timeout=120)
    D, R = RM.counts(plain, NL)
    r = run("ix", path)
    assert r.returncode == 0 and r.stdout == b"12 frames, %d delimiters, %d records\n" % (D, R), (r.returncode, r.stdout, r.stderr)
    D2, R2 = RM.counts(plain, 0x20)
    r = run("ix", path, "-d", "20")
    assert r.returncode == 0 and r.stdout == b"12 frames, %d delimiters, %d records\n" % (D2, R2), (r.returncode, r.stdout, r.stderr)
    r = run("rr", path, 3, 4)
    assert r.returncode == 0 and r.stdout == RM.packed(plain, NL, [3, 4, 5, 6]), (r.returncode, r.stdout[:80], r.stderr)
    r = run("rr", path, R - 2, 100)                                            # clipped to the records there are
    assert r.returncode == 0 and r.stdout == RM.packed(plain, NL, [R - 2, R - 1])
    r = run("rr", path, "-d", "20", 0, 2)
    assert r.returncode == 0 and r.stdout == RM.packed(plain, 0x20, [0, 1])
    r = run("rr", path, R, 1)
    assert r.returncode == 1 and r.stdout == b""
    r = run("rr", path, 3)
    assert r.returncode == 2 and r.stdout == b""
