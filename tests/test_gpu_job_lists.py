"""GPU tests of the planning kernels of the device-archive calls (zra_amd/csrc/zra_joblist.h) where one launch sees more than 1,024
items: a rank crosses a wave edge and a chunk edge, and a running base is carried from chunk to chunk. Every call that builds a job
list runs on one shape, 2,100 frames of 16 bytes with a short last one (chunks of 1,024 + 1,024 + 52), with a flagged set that holds
single frames on both sides of a wave edge and of both chunk edges and a dense block across the first chunk edge; in one pass and with
a staging window of 1,500 slots, whose pass edge lies inside the second chunk and inside the dense block. The additive scans run on
1,100 frames of 8,192 bytes: more than 1,024 tiles in one launch, which is two items per lane of the search's scan and more than one
wave of the table scan of compare and diff (scan_in_place). That one walks 2,048 items at a time, so its chunk edges lie at items
2,048 and 4,096: the job-list shape under DECODE_ALL crosses the first (2,101 items), 4,200 frames of 16 bytes cross both. The yardsticks are the ones of the calls' own test modules: the
pure-Python models of the plaintexts the test generated itself, the whole-frame one-byte query for a frame that does not decode, and
the plain call for the call through a handle. (The update has no staging argument: it runs in one pass.)"""
import numpy as np
import pytest

import compare_model as CM
import diff_model as DM
import grep_model as GM
import msearch_model as MM
import records_model as RM
import search_model as SM
import verify_model as VM
from test_gpu_archive_records import _h_locate_raw, _h_read_raw
from test_gpu_compare import _break_magic, _cmp, _want
from test_gpu_diff import _diff
from test_gpu_records import NL, SENT, _index_raw, _located, _read
from test_gpu_sign import _sigdiff, _signed
from test_gpu_update import _compress, _data, _decompress, _dev, _patched, _update
from test_gpu_verify import _flip_mid, _frame_status, _verify

pytestmark = pytest.mark.gpu

FS = 16
NFR = 2100
U = (NFR - 1) * FS + 9                                                         # the last frame is short
FLAGGED = sorted({0, 63, 64, 1023, 1024, 1025, 2047, 2048, 2099} | set(range(900, 1101)))
STAGINGS = (0, 1500 * FS)
NEEDLE = bytes([200, 201, 202])
# the needle inside frame 0, across the chunk edge 1023 | 1024, across the frames 1099 | 1100 (the warm handle's last resident frame and
# its first missing one), across the pass edge 1499 | 1500, and at the content's end
NEEDLE_AT = (8, 1023 * FS + 15, 1099 * FS + 14, 1499 * FS + 15, U - 3)
WARM = 1100                                                                    # the handle's resident frames: 0 .. 1099
SLOTS = 1200


def _slots(staging, per_slot=FS):
    return None if staging == 0 else staging // per_slot


@pytest.fixture(scope="module")
def lists(zra, gpu_engine):
    """Content a: compressible bytes without the delimiter, one delimiter at byte 5 of every flagged frame and of no other, and the
    needles. Content b: a with byte 2 of every flagged frame changed. Their archives, on the host and on the device."""
    x = np.frombuffer(_data(np.random.RandomState(2100), U), dtype=np.uint8).copy()
    x[x == NL] = 0x40
    for f in FLAGGED:
        x[f * FS + 5] = NL
    for p in NEEDLE_AT:
        x[p:p + 3] = np.frombuffer(NEEDLE, dtype=np.uint8)
    a = x.tobytes()
    for f in FLAGGED:
        x[f * FS + 2] ^= 0x80
    b = x.tobytes()
    assert len(a) == U and RM.delimiters(a, NL) == [f * FS + 5 for f in FLAGGED] and SM.matches(a, NEEDLE) == sorted(NEEDLE_AT)
    assert {f for f in range(NFR) if a[f * FS:(f + 1) * FS] != b[f * FS:(f + 1) * FS]} == set(FLAGGED)
    xa, xb = _compress(gpu_engine, zra, a, 3, FS, True), _compress(gpu_engine, zra, b, 3, FS, True)
    assert VM.fields(xa)[2:] == (NFR, FS, U)
    return dict(a=a, b=b, xa=xa, xb=xb, A=(_dev(xa), len(xa)), B=(_dev(xb), len(xb)))


@pytest.fixture(scope="module")
def warm(zra, gpu_engine, lists):
    """a handle on archive a with 1,200 slots whose frames 0 .. 1,099 are resident; only scans and locate calls use it: it stays so"""
    import torch
    h = zra.Archive(gpu_engine, lists["A"][0].data_ptr(), lists["A"][1], SLOTS * FS)
    out = torch.empty(WARM, dtype=torch.uint8, device="cuda:0")
    h.read(out.data_ptr(), [f * FS for f in range(WARM)], [1] * WARM, list(range(WARM)))
    s = h.stats()
    assert (s["slots"], s["resident"], s["evictions"]) == (SLOTS, WARM, 0), s
    yield h
    h.close()


# ---- the job lists
@pytest.mark.parametrize("staging", STAGINGS)
def test_verify(zra, gpu_engine, lists, staging):
    """A byte flipped inside the compressed span of every flagged frame but 64 and 1,024: content faults. The magic of frames 64 and
    1,024 broken: structure faults, and no job, so the rank of every sound frame behind them shifts."""
    content_bad = [f for f in FLAGGED if f not in (64, 1024)]
    bad = _break_magic(_flip_mid(lists["xa"], content_bad), [64, 1024])
    d = _dev(bad)
    structure = VM.structure_faults(bad)
    assert sorted(structure) == [64, 1024], structure
    near = sorted({g for f in FLAGGED for g in (f - 1, f, f + 1) if 0 <= g < NFR})
    status = _frame_status(gpu_engine, zra, bad, frames=near, d_arc=d)
    assert sorted(status) == FLAGGED, sorted(set(status) ^ set(FLAGGED))
    want = [(f, structure[f], VM.STRUCTURE) if f in structure else (f, status[f], VM.CONTENT) for f in FLAGGED]
    st, n, faults = _verify(gpu_engine, bad, d, staging_bytes=staging)
    assert st == (0, 0) and n == len(FLAGGED), (st, n)
    assert faults == want, [(x, y) for x, y in zip(faults, want) if x != y][:6]
    s = gpu_engine.verify_stats()
    assert (s["frames"], s["checked"], s["structure_faults"], s["content_faults"], s["decoded"], s["passes"]) == \
        (NFR, NFR, 2, len(FLAGGED) - 2, NFR - 2, 1 if staging == 0 else 2), s


@pytest.mark.parametrize("staging", STAGINGS)
def test_compare_and_diff(zra, gpu_engine, lists, staging):
    a, b, A, B = (lists[k] for k in ("a", "b", "A", "B"))
    want = _want(a, b)
    assert want[1] == len(FLAGGED) and want[3][0] == (2, 1)
    for decode_all in (False, True):
        decoded = None if decode_all else set(FLAGGED)
        got = _cmp(gpu_engine, zra, A, B, staging_bytes=staging, decode_all=decode_all)
        assert got == want, (decode_all, got[:3], [(x, y) for x, y in zip(got[3], want[3]) if x != y][:6])
        s = gpu_engine.compare_stats()
        assert s == CM.stats(a, b, FS, decoded=decoded, slots=_slots(staging, 2 * FS)), (decode_all, s)
        if not decode_all:
            assert (s["decoded"], s["equal_compressed"]) == (len(FLAGGED), NFR - len(FLAGGED)), s
        for grain in (1, 64):
            _diff(gpu_engine, zra, A, B, a, b, FS, grain, staging=staging, mode=1 if decode_all else 0)
            s = gpu_engine.diff_stats()
            assert s == DM.stats(a, b, FS, grain, decoded=decoded, slots=_slots(staging, 2 * FS)), (decode_all, grain, s)
            assert s["decoded"] == (NFR if decode_all else len(FLAGGED)), s


@pytest.mark.parametrize("staging", STAGINGS)
def test_sign_and_signature_diff(zra, gpu_engine, lists, staging):
    """Grain 64: one grain per frame. The patch is the one the diff of the two archives gives at that grain (diff_model.patch)."""
    a, b, A, B, xa = (lists[k] for k in ("a", "b", "A", "B", "xa"))
    sig, buf, _ = _signed(gpu_engine, zra, A, xa, a, FS, 64, staging=staging)
    s = gpu_engine.sign_stats()
    assert (s["frames"], s["signed"], s["grain_words"], s["content_bytes"], s["passes"]) == (NFR, NFR, NFR, U, 1 if staging == 0 else 2), s
    for decode_all in (False, True):
        (writes, _, _, _), _ = _sigdiff(gpu_engine, zra, sig, buf, B, a, b, FS, staging=staging, mode=1 if decode_all else 0)
        assert sorted({p // FS for o, n in writes for p in range(o, o + n, FS)}) == FLAGGED
        s = gpu_engine.diff_signature_stats()
        sl = _slots(staging)
        assert s == DM.stats(a, b, FS, 64, decoded=None if decode_all else set(FLAGGED), slots=sl, tail_slots=sl), (decode_all, s)
        assert s["decoded"] == (NFR if decode_all else len(FLAGGED)), s


def _record_index(eng, zra, lists):
    r = _index_raw(eng, zra, lists["A"], NL, frames=NFR)
    assert r["st"] == (0, 0) and r["words"][:NFR] == RM.index_words(lists["a"], FS, NL)
    return zra.RecordIndex(*r["info"]), r["buf"]


@pytest.mark.parametrize("staging", STAGINGS)
def test_locate_and_read_records(zra, gpu_engine, lists, warm, staging):
    """The delimiters lie in exactly the flagged frames, so those are the frames every record's boundaries need. All records, in shuffled
    order: the plain call, then the same through the warm handle, whose split sees copies (the flagged frames below 1,100) and jobs.
    The list that zra_rec_split_kernel walks holds only the needed frames, 207 entries: one chunk. The chunk edges of that function
    (split_by_residency, which zra_scan_split_kernel is too) are crossed in test_search_and_grep_through_the_handle."""
    a, A = lists["a"], lists["A"]
    idx, buf = _record_index(gpu_engine, zra, lists)
    assert (idx.delimiters, idx.records) == (len(FLAGGED), len(FLAGGED) + 1)
    numbers = [int(k) for k in np.random.RandomState(7).permutation(idx.records)]
    plain = _located(gpu_engine, zra, A, idx, buf, a, NL, numbers, staging)
    s = gpu_engine.locate_records_stats()
    assert (s["frames"], s["records"], s["decoded"], s["content_bytes"], s["passes"]) == \
        (NFR, len(numbers), len(FLAGGED), sum(min(FS, U - f * FS) for f in FLAGGED), 1), s
    _read(gpu_engine, zra, A, idx, buf, a, NL, numbers, staging)
    assert gpu_engine.read_records_stats()["locate_decoded"] == len(FLAGGED)
    # through the handle
    before, tot = warm.stats(), warm.record_stats()
    got = _h_locate_raw(zra, warm, idx, buf, NFR, numbers, staging)
    assert got["st"] == (0, 0) and got["ranges"] == plain["ranges"] == RM.locate(a, NL, numbers) and got["tail_ok"]
    staged = len([f for f in FLAGGED if f < WARM])
    r = warm.record_stats()
    assert (r["calls"], r["staged"], r["decoded"], r["passes"]) == (tot["calls"] + 1, staged, len(FLAGGED) - staged, 1), r
    assert staged == 203 and gpu_engine.locate_records_stats()["decoded"] == len(FLAGGED) - staged
    assert warm.stats() == before
    # the read through a handle of its own: its byte fetch is a read of the handle
    import torch
    h = zra.Archive(gpu_engine, A[0].data_ptr(), A[1], SLOTS * FS)
    try:
        out = torch.empty(WARM, dtype=torch.uint8, device="cuda:0")
        h.read(out.data_ptr(), [f * FS for f in range(WARM)], [1] * WARM, list(range(WARM)))
        want = RM.packed(a, NL, numbers)
        got = _h_read_raw(zra, h, idx, buf, NFR, numbers, len(want) + 5, staging)
        assert got["st"] == (0, 0) and got["size"] == len(want) and got["ranges"] == plain["ranges"]
        assert got["data"][:len(want)] == want and got["data"][len(want):] == bytes([SENT]) * 5 and got["sentinel_ok"]
        r = h.record_stats()
        assert (r["staged"], r["decoded"]) == (staged, len(FLAGGED) - staged), r
    finally:
        h.close()


def test_search_and_grep_through_the_handle(zra, gpu_engine, lists, warm):
    """The whole range in one pass of 2,100 frames: the split ranks 1,100 copies and 1,000 jobs across both chunk edges."""
    a, A = lists["a"], lists["A"]
    P, size = A[0].data_ptr(), A[1]
    before = warm.stats()
    want = SM.matches(a, NEEDLE)
    plain = gpu_engine.search(P, size, NEEDLE)
    assert tuple(plain) == (len(want), want)
    assert tuple(warm.search(NEEDLE)) == tuple(plain)
    s = warm.scan_stats()
    assert (s["staged"], s["decoded"], s["passes"]) == (WARM, NFR - WARM, 1), s
    assert gpu_engine.search_stats()["decoded"] == NFR - WARM
    pats = [NEEDLE, bytes([201, 202]), b"\x01\x02\x03"]
    wm = MM.matches_multi(a, pats)
    plain = gpu_engine.search_multi(P, size, pats)
    assert (plain[0], plain[1]) == (len(wm), wm)
    assert tuple(warm.search_multi(pats)) == tuple(plain)
    _, sel, _ = GM.grep(a, pats, NL, False, 0, None)
    plain = gpu_engine.grep(P, size, pats)
    assert tuple(plain) == (len(sel), sel) and len(sel) >= 4
    assert tuple(warm.grep(pats)) == tuple(plain)
    s = warm.scan_stats()
    assert (s["staged"], s["decoded"], s["passes"]) == (WARM, NFR - WARM, 1), s
    assert warm.stats() == before


def test_update(zra, gpu_engine, lists):
    """One byte written into every flagged frame, so each keeps old bytes and needs its decode, and an append that fills the short last
    frame and adds three frames."""
    a, xa = lists["a"], lists["xa"]
    rng = np.random.RandomState(11)
    writes = [(f * FS + 3, bytes([int(rng.randint(128, 256))])) for f in FLAGGED]
    app = rng.randint(128, 256, size=7 + 2 * FS + 5).astype(np.uint8).tobytes()
    st, out, size = _update(gpu_engine, zra, xa, writes, app, d_arc=lists["A"][0])
    assert st == (0, 0)
    s = gpu_engine.update_stats()
    assert (s["frames"], s["touched"], s["decoded"], s["compressed"], s["passes"]) == (NFR + 3, len(FLAGGED) + 3, len(FLAGGED), len(FLAGGED) + 3, 1), s
    new = out[:size]
    assert VM.crc_ok(new) and VM.structure_faults(new) == {}
    assert _decompress(gpu_engine, new) == _patched(a, writes, app)


# ---- the additive scans
FS_S = 8192
NFR_S = 1100
U_S = (NFR_S - 1) * FS_S + 5000
TILES = (0, 1023, 1024, NFR_S - 1)                                             # the first tile, both sides of the chunk edge, the last
LONG = bytes(range(210, 218))
SHORT = bytes([230, 231])


@pytest.fixture(scope="module")
def scans(zra, gpu_engine):
    """1,100 frames of 8,192 bytes, the last one short: one tile of the scans and of the compare per frame. Content a holds three
    occurrences of an 8-byte and of a 2-byte pattern in each of four tiles; content b differs from a in the same four tiles."""
    x = np.frombuffer(_data(np.random.RandomState(1100), U_S), dtype=np.uint8).copy()
    for t in TILES:
        for k, p in enumerate((17, 2500, 4800)):
            x[t * FS_S + p:t * FS_S + p + 8] = np.frombuffer(LONG, dtype=np.uint8)
            x[t * FS_S + p + 100 + k:t * FS_S + p + 102 + k] = np.frombuffer(SHORT, dtype=np.uint8)
    a = x.tobytes()
    for t in TILES:
        for lo, n in ((0, 1), (300, 70), (4000, 3), (4999, 1)):
            x[t * FS_S + lo:t * FS_S + lo + n] ^= 0x80
    b = x.tobytes()
    xa, xb = _compress(gpu_engine, zra, a, 3, FS_S, True), _compress(gpu_engine, zra, b, 3, FS_S, True)
    return dict(a=a, b=b, A=(_dev(xa), len(xa)), B=(_dev(xb), len(xb)))


def test_search_scans_more_than_1024_tiles(zra, gpu_engine, scans):
    a, A = scans["a"], scans["A"]
    want = SM.matches(a, LONG)
    assert [p // FS_S for p in want] == [t for t in TILES for _ in range(3)]
    got = gpu_engine.search(A[0].data_ptr(), A[1], LONG)
    assert tuple(got) == (len(want), want)
    s = gpu_engine.search_stats()
    assert (s["frames"], s["decoded"], s["content_bytes"], s["passes"]) == (NFR_S, NFR_S, U_S, 1), s
    pats = [LONG, SHORT, LONG[2:7], bytes([250, 251])]
    wm = MM.matches_multi(a, pats)
    n, at, per = gpu_engine.search_multi(A[0].data_ptr(), A[1], pats)
    assert (n, at) == (len(wm), wm) and per == [12, 12, 12, 0]
    assert gpu_engine.search_multi_stats()["passes"] == 1


def test_compare_and_diff_scan_more_than_1024_items(zra, gpu_engine, scans):
    """Every frame decoded: 1,100 tiles and the pass's item 0 in one launch of the scan: 551 lanes of two items, one chunk."""
    a, b, A, B = (scans[k] for k in ("a", "b", "A", "B"))
    want = _want(a, b)
    assert want[1] == 4 * len(TILES) and sorted({o // FS_S for o, _ in want[3]}) == list(TILES)
    got = _cmp(gpu_engine, zra, A, B, decode_all=True)
    assert got == want, got[:3]
    s = gpu_engine.compare_stats()
    assert (s["decoded"], s["passes"], s["ranges"]) == (NFR_S, 1, want[1]), s
    writes, _, _, _ = _diff(gpu_engine, zra, A, B, a, b, FS_S, 64, mode=1)
    assert sorted({o // FS_S for o, _ in writes}) == list(TILES)
    s = gpu_engine.diff_stats()
    assert (s["decoded"], s["passes"], s["writes"]) == (NFR_S, 1, len(writes)), s


# ---- the table scan of compare and diff across its chunk edges
NFR_C = 4200
U_C = (NFR_C - 1) * FS + 9
# item 0 is the pass's head and item i tile i - 1; at 16 bytes a frame is a tile. Differing tiles: the first, a block around each of the
# chunk edges 2,047 | 2,048 and 4,095 | 4,096 of the items (both items of the lanes on either side), the last
DIFFER = sorted({0, NFR_C - 1} | set(range(2040, 2057)) | set(range(4088, 4105)))


@pytest.fixture(scope="module")
def chunks(zra, gpu_engine):
    """4,200 frames of 16 bytes, the last one short; content b differs from a in bytes 0, 5 .. 7 and the last byte of every tile of
    DIFFER (starts, ends and dirty bytes on both sides of each edge; neighbouring tiles' runs touch)."""
    x = np.frombuffer(_data(np.random.RandomState(4200), U_C), dtype=np.uint8).copy()
    a = x.tobytes()
    for t in DIFFER:
        n = min(FS, U_C - t * FS)
        for p in (0, 5, 6, 7, n - 1):
            x[t * FS + p] ^= 0x80
    b = x.tobytes()
    xa, xb = _compress(gpu_engine, zra, a, 3, FS, True), _compress(gpu_engine, zra, b, 3, FS, True)
    return dict(a=a, b=b, A=(_dev(xa), len(xa)), B=(_dev(xb), len(xb)))


@pytest.mark.parametrize("staging", [0, 3000 * 2 * FS])
def test_compare_and_diff_scan_across_two_chunk_edges(zra, gpu_engine, chunks, staging):
    """Every frame decoded. One pass: 4,201 items in one launch, chunks of 2,048 + 2,048 + 105, a total carried twice. Two passes of
    3,000 and 1,200 frame pairs: 3,001 and 1,201 items, the second launch behind the first one's totals."""
    a, b, A, B = (chunks[k] for k in ("a", "b", "A", "B"))
    want = _want(a, b)
    assert sorted({o // FS for o, _ in want[3]}) == DIFFER and want[1] > 2 * len(DIFFER)
    got = _cmp(gpu_engine, zra, A, B, staging_bytes=staging, decode_all=True)
    assert got == want, (got[:3], [(x, y) for x, y in zip(got[3], want[3]) if x != y][:6])
    s = gpu_engine.compare_stats()
    assert s == CM.stats(a, b, FS, slots=_slots(staging, 2 * FS)) and s["decoded"] == NFR_C, s
    for grain in (1, 4):
        writes, _, _, _ = _diff(gpu_engine, zra, A, B, a, b, FS, grain, staging=staging, mode=1)
        assert sorted({o // FS for o, _ in writes}) == DIFFER
        s = gpu_engine.diff_stats()
        assert s == DM.stats(a, b, FS, grain, slots=_slots(staging, 2 * FS)) and s["decoded"] == NFR_C, (grain, s)
