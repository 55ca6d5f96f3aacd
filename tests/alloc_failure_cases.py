"""The child process of tests/test_gpu_alloc_failure.py: `python alloc_failure_cases.py GROUP` runs the cases of one group on cuda:0 and
prints one JSON line per case, {"case", "ok", "problems", "s"}. ZRA_ALLOC_LIMIT_MIB is read once per process, so the parent sets it (and
the other knobs of a group) in the environment it starts this file with. The child stops at the first case that does not hold (exit 1)
and synchronises the device after every case: a failed synchronise ends it at once (exit 3).

What a failing call must leave behind is checked in one place, must_fail(): the status {ZStdError, 64}; every output word 0 (*outSize of the compress and the updates: untouched, as zra_hip.h has it); every host
array and device buffer of the caller with its 0xEE fill, 64 guard bytes on both sides included; the call's own row of counters and
its milliseconds zero, the rows of the other calls what they were; and the same again when the call is repeated. A call that returns
Success where it was built to fail is reported as "sizes no longer straddle the limit". What follows a failing call is the caller's:
the call that fits on the same engine, held to its CPU model, and once more behind release_scratch().

Archives come from the CPU oracle (tests/oracle_lib.py; byte for byte what the engine writes, tests/test_gpu_parity.py): the encoder's
scratch of a whole archive would not fit under the limits these groups run with. A large archive is a small one's frames repeated
behind a stitched header, its content the small content repeated."""
import ctypes
import json
import os
import re
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

GUARD = 64
MAXU64 = (1 << 64) - 1
NL = 10
LIMITED = "ZRA_ALLOC_LIMIT_MIB" in os.environ
NO_MEMORY = (1, 64)
U64P = ctypes.POINTER(ctypes.c_uint64)

Z = L = torch = O = None        # zra_amd, its library, torch, the oracle: main()


# ---- the caller's side of a call
class Host:
    """a host array of n bytes the caller hands to a call: 0xEE-filled, between two guards. A failing call leaves all of it alone."""
    fill = 0xEE

    def __init__(self, n):
        self.n = n
        self.raw = (ctypes.c_ubyte * (n + 2 * GUARD))()
        ctypes.memset(self.raw, 0xEE, n + 2 * GUARD)
        ctypes.memset(ctypes.addressof(self.raw) + GUARD, self.fill, n)
        self.addr = ctypes.addressof(self.raw) + GUARD

    def problem(self):
        want = b"\xEE" * GUARD + bytes([self.after]) * self.n + b"\xEE" * GUARD
        got = bytes(self.raw)
        if got == want:
            return None
        at = next(i for i in range(len(got)) if got[i] != want[i]) - GUARD
        return "%s of %d bytes: byte %d is 0x%02X, not 0x%02X" % (type(self).__name__, self.n, at, got[at + GUARD], want[at + GUARD])
    after = 0xEE


class Words(Host):
    """k output words of a call: 0xEE-filled, between two guards; a failing call leaves them 0 (entry_call's rule, zra_host.h)"""
    after = 0

    def __init__(self, k=1):
        Host.__init__(self, 8 * k)


class SizeWord(Host):
    """*outSize of the compress and of the two updates, which no entry_call governs: they write it on Success and on OutputBufferTooSmall
    (the size needed) and nowhere else (zra_hip.h; tests/test_gpu_update.py pins the same for their refusals), so behind a failure it is
    the caller's 0xEE still"""

    def __init__(self):
        Host.__init__(self, 8)


class Dev:
    """a device buffer of n bytes the caller hands to a call: 0xEE-filled, between two guards"""

    def __init__(self, n):
        self.n = n
        self.t = torch.full((n + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        self.addr = self.t.data_ptr() + GUARD

    def problem(self):
        if bool((self.t == 0xEE).all().item()):
            return None
        at = int((self.t != 0xEE).nonzero()[0].item()) - GUARD
        return "device buffer of %d bytes: byte %d is not 0xEE" % (self.n, at)

    def head(self, k):
        return self.t[GUARD:GUARD + k].cpu().numpy().tobytes()

    def rest_problem(self, k):
        """the guard in front and everything behind the first k bytes"""
        if bool((self.t[:GUARD] == 0xEE).all().item()) and bool((self.t[GUARD + k:] == 0xEE).all().item()):
            return None
        return "device buffer: bytes outside the first %d are not 0xEE" % k


def dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).to("cuda:0")


def u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(U64P)


def call(fn, args):
    """fn(*args) with every Host / Dev among the arguments passed as the pointer the entry point declares; (status, those arguments)"""
    conv = []
    for a, typ in zip(args, fn.argtypes):
        if isinstance(a, (Host, Dev)):
            a = a.addr if typ is ctypes.c_void_p else ctypes.cast(ctypes.c_void_p(a.addr), typ)
        conv.append(a)
    assert len(conv) == len(fn.argtypes), (fn.__name__, len(args), len(fn.argtypes))
    return fn(*conv).tup(), [a for a in args if isinstance(a, (Host, Dev))]


ROWS = {"search": ("ZraHipGetSearchStats", "ZraHipDebugSearchScanMs"), "search_multi": ("ZraHipGetSearchMultiStats", "ZraHipDebugSearchMultiScanMs"),
        "grep": ("ZraHipGetGrepStats", "ZraHipDebugGrepScanMs"), "extract": ("ZraHipGetExtractStats", "ZraHipDebugExtractMs"),
        "compare": ("ZraHipGetCompareStats", "ZraHipDebugCompareMs"), "diff": ("ZraHipGetDiffStats", "ZraHipDebugDiffMs"),
        "sign": ("ZraHipGetSignStats", "ZraHipDebugSignMs"), "diff_signature": ("ZraHipGetDiffSignatureStats", "ZraHipDebugDiffSignatureMs"),
        "index_records": ("ZraHipGetIndexRecordsStats", "ZraHipDebugIndexRecordsMs"), "locate_records": ("ZraHipGetLocateRecordsStats", "ZraHipDebugLocateRecordsMs"),
        "read_records": ("ZraHipGetReadRecordsStats", "ZraHipDebugReadRecordsMs"), "verify": ("ZraHipGetVerifyStats", None),
        "tally": ("ZraHipGetTallyStats", "ZraHipDebugTallyMs"), "update": ("ZraHipGetUpdateStats", None)}


def rows(eng):
    """every call's row of counters and its milliseconds, as they stand"""
    out = {}
    for k, (get, ms) in ROWS.items():
        a = (ctypes.c_uint64 * 8)()
        getattr(L, get)(eng.h, a)
        out[k] = (tuple(int(v) for v in a), float(getattr(L, ms)(eng.h)) if ms else 0.0)
    return out


def sync(eng, what):
    try:
        torch.cuda.synchronize()
        st = L.ZraHipSynchronize(eng.h).tup()
    except Exception as e:                                                     # (a HIP error: nothing more runs on the device)
        st = "%s: %s" % (type(e).__name__, e)
    if st != (0, 0):
        print(json.dumps({"case": what, "ok": False, "problems": ["synchronise: %s" % (st,)], "s": 0}), flush=True)
        os._exit(3)


def must_fail(eng, fn, make_args, own=(), also=None):
    """The contract of a call built to fail, items 1 to 4 and 6 (module docstring). make_args() -> the argument list, fresh buffers
    each time; own: the rows the call writes; also() -> more problems (a handle's counters). Returns the problems, [] if it held."""
    probs = []
    for attempt in ("", "repeated: "):
        args = make_args()
        before = rows(eng)
        eng._order()
        st, outs = call(fn, args)
        sync(eng, fn.__name__)
        after = rows(eng)
        if st == (0, 0):
            probs.append(attempt + "%s succeeded: sizes no longer straddle the limit" % fn.__name__)
        elif st != NO_MEMORY:
            probs.append(attempt + "%s returned %s, not (1, 64)" % (fn.__name__, st))
        probs += [attempt + p for p in (o.problem() for o in outs) if p]
        for k in after:
            if k in own:
                if any(after[k][0]) or after[k][1] != 0:
                    probs.append(attempt + "own row %s is %s" % (k, after[k]))
            elif after[k] != before[k]:
                probs.append(attempt + "row %s changed: %s -> %s" % (k, before[k], after[k]))
        if also:
            probs += [attempt + p for p in also()]
        if probs:
            break
    return probs


def then_fits(eng, fit):
    """items 5 and 7: the fitting call on the same engine gives its model's answer, and again behind release_scratch(). fit() -> problems"""
    probs = fit()
    if not probs:
        eng.release_scratch()
        probs = ["after release_scratch: " + p for p in fit()]
    return probs


def case(eng, name, fn):
    t = time.time()
    try:
        probs = fn()
    except Exception as e:                                                     # (an unexpected status raises ZraError)
        probs = ["%s: %s" % (type(e).__name__, e)]
    sync(eng, name)
    print(json.dumps({"case": name, "ok": not probs, "problems": [str(p)[:300] for p in probs[:6]], "s": round(time.time() - t, 3)}), flush=True)
    if probs:
        sys.exit(1)


def same(what, got, want):
    if got == want:
        return []
    if isinstance(got, (bytes, list)) and isinstance(want, (bytes, list)):
        n = min(len(got), len(want))
        at = next((i for i in range(n) if got[i] != want[i]), n)
        return ["%s differs from the model at %d (sizes %d, %d)" % (what, at, len(got), len(want))]
    return ["%s is %r, the model says %r" % (what, got, want)]


# ---- archives
class Unit:
    """`base` (a whole number of frames) compressed by the oracle, its frames at hand: archive(n) is n frames, frame i a copy of frame
    i % F, behind a header stitched from their sizes (ZraHipStitchHeader); its content is base repeated."""

    def __init__(self, base, fs, level=3):
        assert len(base) % fs == 0
        self.base, self.fs, self.F = base, fs, len(base) // fs
        st, arc = O.zra_compress(base, level, fs, True, 0, "zo")
        assert st == (0, 0), st
        hsz, nent, meta = int.from_bytes(arc[4:8], "little") + 8, int.from_bytes(arc[26:30], "little"), int.from_bytes(arc[34:38], "little")
        assert nent == self.F + 1 and meta == 0
        off = [int.from_bytes(arc[38 + 5 * i:43 + 5 * i], "little") for i in range(nent)]
        body = arc[hsz:]
        self.frames = [body[off[i] - off[0]:off[i + 1] - off[0]] for i in range(self.F)]

    def archive(self, n, swap=None, damage=None):
        """swap: {frame: (another Unit, its frame)}, whose content the frame then holds; damage: {frame: the compressed bytes it gets}"""
        pick = [(swap or {}).get(i, (self, i % self.F)) for i in range(n)]
        frames = [(damage or {}).get(i, u.frames[k]) for i, (u, k) in enumerate(pick)]
        arc = Z.stitch_header([len(f) for f in frames], n * self.fs, self.fs) + b"".join(frames)
        return arc, b"".join(u.base[k * self.fs:(k + 1) * self.fs] for u, k in pick)


def lz_bytes(seed, n):
    from test_gpu_update import _data
    return _data(np.random.RandomState(seed), n)


# ---- group: decode (ZraHipDecompressBuffer, device pointers), ZRA_DEC_SMALL_MAX=0, with and without ZRA_ALLOC_LIMIT_MIB=11
# Engine::decode_scratch (rounds) for n frames of 256 KiB: perFrame = min(262144 + 16, 131072 + 16) = 131088;
#   decLits_ asks n * 131088 / 2 + 64 (at least 1 Mi + 64), decSeqs_ 8 * max(n * 131088 * 3 / 32, 1 Mi) + 64.
# Engine::decode_launch (block pass, taken from 64 jobs of at least two 128 KiB blocks): decLits_ asks n * 262160 / 2 + 64, decSeqs_
#   8 * (n * 262160 * 3 / 32) + 64. DevBuf::reserve pads a request r to r + r / 8 + 256; the limit is 11 MiB = 11,534,336.
#   n    rounds decLits_  rounds decSeqs_   pass decLits_     pass decSeqs_
#   64    4,719,496        9,437,512         9,438,088 fits    14,156,968 FAILS (decLits_ has moved)
#   96    7,079,080       10,618,456        14,156,968 FAILS   (not reached)
#  256   18,877,000 FAILS: the call answers {ZStdError, 64}
# (the other buffers of both: 5,120 bytes of tables per job, records and lists of a few bytes per job: under 1.5 MiB)
def group_decode(eng):
    import corpus as C
    fs = 256 << 10
    # (log lines: their literals stay under half of a block and their sequences under three quarters, what the rounds' scratch is sized
    # for, so no frame is deferred to a third round)
    unit = Unit(C.gen_loglike(4 * fs, seed=5), fs)
    arcs = {n: unit.archive(n) for n in (64, 96, 256)}
    st, plain = O.zra_decompress(arcs[64][0])
    assert st == (0, 0) and plain == arcs[64][1]                               # (the codec's yardstick: the oracle reads the stitched archive)
    d = {n: dev(a) for n, (a, _) in arcs.items()}

    def decode(n, rounds):
        arc, content = arcs[n]
        out = Dev(len(content))
        eng.decompress(d[n].data_ptr(), len(arc), out.addr, len(content))
        sync(eng, "decode")
        probs = same("output of %d frames" % n, out.head(len(content)), content)
        p = out.rest_problem(len(content))
        got = eng.decode_stage_stats()["rounds"]                               # (reset by every call: the call's own launches)
        if rounds is not None and got != rounds:
            probs.append("%d frames: rounds word %d, not %d (1: the block pass alone, 2: two rounds)" % (n, got, rounds))
        return probs + ([p] if p else [])

    # with the limit the pass's reservation fails and the rounds decode; without it the same call takes the block pass (the premise)
    want = 2 if LIMITED else 1
    case(eng, "decode 64 frames: pass fails at decSeqs_ behind a moved decLits_", lambda: decode(64, want))
    case(eng, "decode 96 frames: pass fails at decLits_", lambda: decode(96, want))
    if not LIMITED:
        case(eng, "decode 256 frames", lambda: decode(256, 1))
        return
    arc, content = arcs[256]
    case(eng, "decode 256 frames: the rounds' scratch does not fit",
         lambda: must_fail(eng, L.ZraHipDecompressBuffer, lambda: [eng.h, d[256].data_ptr(), len(arc), Dev(len(content)), len(content)])
         or then_fits(eng, lambda: decode(64, want)))


# ---- group: ra (ZraHipDecompressRABatch, ZraHipArchiveRead, ZraHipUpdateArchive, ZraHipArchiveUpdate), ZRA_ALLOC_LIMIT_MIB=11
# 256 frames of 64 KiB. Engine::ra_batch_body and UpdateImpl::run ask stage_ for touched * 65536 + 64: 200 touched frames are
# 13,107,264 -> 14,745,928 padded, over the limit; 100 are 7,373,096, 8 are 590,152. The decoder's scratch of 100 jobs (decSeqs_'
# floor, 9,437,512) and the encoder's of 8 frames fit. A handle without a cache reads through ra_batch_body.
def group_ra(eng):
    fs, F = 64 << 10, 256
    unit = Unit(lz_bytes(12, 16 * fs), fs)
    arc, content = unit.archive(F)
    d_arc = dev(arc)

    def queries(frames):
        off = [f * fs + 100 + f % 7 for f in frames]
        size = [3000 + f for f in frames]
        return off, size, [int(v) for v in np.cumsum([0] + size[:-1])], sum(size)

    many, few = queries(range(200)), queries(range(5, 205, 2))

    def batch_args(q, head):
        (_, po), (_, ps), (_, pd) = keep = [u64(a) for a in q[:3]]
        return list(head) + [Dev(q[3]), po, ps, pd, len(q[0])], keep

    def held(fn, q, head, **kw):
        keep = []

        def make():
            args, k = batch_args(q, head)
            keep.append(k)
            return args
        return must_fail(eng, fn, make, **kw)

    def read_fits(read, q, plain):
        out = Dev(q[3])
        read(out.addr, q[0], q[1], q[2])
        sync(eng, "read")
        p = out.rest_problem(q[3])
        return same("answers", out.head(q[3]), b"".join(plain[o:o + n] for o, n in zip(q[0], q[1]))) + ([p] if p else [])

    case(eng, "ra batch: stage_",
         lambda: held(L.ZraHipDecompressRABatch, many, (eng.h, d_arc.data_ptr(), len(arc)))
         or then_fits(eng, lambda: read_fits(lambda *a: eng.decompress_ra_batch(d_arc.data_ptr(), len(arc), *a), few, content)))

    h = Z.Archive(eng, d_arc.data_ptr(), len(arc), 0)
    s0 = h.stats()
    case(eng, "handle read without a cache: stage_",
         lambda: held(L.ZraHipArchiveRead, many, (h.h,), also=lambda: same("handle stats", h.stats(), s0))
         or then_fits(eng, lambda: read_fits(h.read, few, content)))
    h.close()

    # ---- update: writes of 100 bytes into `frames`, one per frame
    rng = np.random.RandomState(5)

    def writes(frames):
        off = [f * fs + 1000 + f for f in frames]
        data = bytes(rng.randint(0, 256, size=100 * len(off), dtype=np.uint8))
        patched = bytearray(content)
        for i, o in enumerate(off):
            patched[o:o + 100] = data[100 * i:100 * i + 100]
        return off, [100] * len(off), [100 * i for i in range(len(off))], dev(data), bytes(patched)

    w_many, w_few = writes(range(200)), writes(range(40, 200, 20))
    cap = len(arc) + (1 << 20)

    def update_args(w, head):
        keep = [u64(a) for a in w[:3]]
        return list(head) + [w[3].data_ptr(), keep[0][1], keep[1][1], keep[2][1], len(w[0]), None, 0, Dev(cap), cap, SizeWord(), 3, True], keep

    def update_held(fn, head, **kw):
        keep = []

        def make():
            args, k = update_args(w_many, head)
            keep.append(k)
            return args
        return must_fail(eng, fn, make, own=("update",), **kw)

    def update_fits(update):
        out = Dev(cap)
        n = update(out.addr, cap, writes=w_few[:3], d_data=w_few[3].data_ptr())
        sync(eng, "update")
        st, plain = O.zra_decompress(out.head(n))
        p = out.rest_problem(n)
        return same("status of the oracle's decode", st, (0, 0)) + same("content of the updated archive", plain, w_few[4]) + ([p] if p else [])

    case(eng, "update: stage_ / upd_.packed",
         lambda: update_held(L.ZraHipUpdateArchive, (eng.h, d_arc.data_ptr(), len(arc)))
         or then_fits(eng, lambda: update_fits(lambda *a, **k: eng.update(d_arc.data_ptr(), len(arc), *a, **k))))

    # through a handle with a cache: a failing update leaves it bound to the old archive, counters and resident frames as they were
    hu = Z.Archive(eng, d_arc.data_ptr(), len(arc), 32 * fs)
    warm = queries(range(30, 50))
    mixed = queries(range(40, 60))                                             # ten resident frames, ten that are not

    def handle_update():
        probs = read_fits(hu.read, warm, content)
        s1, u1 = hu.stats(), hu.update_stats()
        probs += update_held(L.ZraHipArchiveUpdate, (hu.h,), also=lambda: same("handle stats", hu.stats(), s1) + same("handle update stats", hu.update_stats(), u1))
        probs += read_fits(hu.read, mixed, content)                            # (bound to the old archive)
        if probs:
            return probs
        out = Dev(cap)
        n = hu.update(out.addr, cap, writes=w_few[:3], d_data=w_few[3].data_ptr())
        st, plain = O.zra_decompress(out.head(n))
        hot = queries(range(35, 65, 5))                                        # (40 and 60 hold new bytes)
        return same("content of the handle's updated archive", plain, w_few[4]) + read_fits(hu.read, hot, w_few[4])
    case(eng, "handle update: stage_, the handle stays bound", handle_update)
    hu.close()

    # ---- a read through a handle WITH a cache: it has no staging window (misses are decoded into the arena), so the aim is the piece
    # list. 4,096 frames of 256 bytes; 300,000 queries of 258 bytes from a frame's last byte on, three slices each. The tuples fit:
    # qmeta_ asks 32 * 300,000 + 64 = 9,600,064 -> 10,800,328 padded; raPieces_ asks 16 * 900,000 + 64 = 14,400,064 -> 16,200,328, over
    # the limit. The reservation stands in front of the lookup kernel, which copies the hits: dOut, the counters and the cache stay.
    fs2, F2, nq = 256, 4096, 300000
    arc2, content2 = Unit(lz_bytes(13, 64 * fs2), fs2).archive(F2)
    d_arc2 = dev(arc2)
    hc = Z.Archive(eng, d_arc2.data_ptr(), len(arc2), 64 * fs2)

    def spans(first):
        off = [int(f) * fs2 + fs2 - 1 for f in first]
        return off, [fs2 + 2] * len(off), [i * (fs2 + 2) for i in range(len(off))], len(off) * (fs2 + 2)
    wide = spans(np.arange(nq) * 7 % (F2 - 3))

    def cached_read():
        probs = read_fits(hc.read, spans(range(100, 120)), content2)           # frames 100 to 121 resident
        s1 = hc.stats()
        probs += held(L.ZraHipArchiveRead, wide, (hc.h,), also=lambda: same("handle stats", hc.stats(), s1))
        return probs or then_fits(eng, lambda: read_fits(hc.read, spans(range(110, 130)), content2))       # (resident frames and others)
    case(eng, "handle read with a cache: raPieces_", cached_read)
    hc.close()


# ---- group: scan (the range scans, zra_scan.h ScanImpl::passes), ZRA_ALLOC_LIMIT_MIB=11
# 768 frames of 16 KiB, 12 MiB of log lines. staging_bytes = 0 is a window of all 768 frames: stage_ is asked for 256 + 12,582,912 + 64
# = 12,583,232 -> 14,156,392 padded, over the limit of 11,534,336. staging_bytes = 4 MiB is 256 slots: 4,194,624 -> 4,719,208; the
# decoder's scratch of a pass of 256 jobs is decSeqs_' floor, 9,437,512. The fitting call scans [LO, HI), frames 192 to 480, in two
# passes: the Python models take seconds on all of it.
SCAN_FS, SCAN_FRAMES, STAGING = 16 << 10, 768, 4 << 20
LO = (3 << 20) + 1234
HI = LO + (4 << 20) + (1 << 19)
PATS = [b"ERROR", b"user=42 ", b"latency_ms=7"]
EXPR = [b"ERROR req=[0-9a-f]+ user=4[0-9] ", b"items/77+ "]


class ReMatcher:
    """regex_model.Matcher's answers for EXPR from Python's re (the same language for these two expressions; main() holds the two
    against each other on the first records): the model's own automaton walks a byte at a time, too slowly for 45,000 records"""

    def __init__(self, exprs):
        self.r = [re.compile(e) for e in exprs]

    def matches(self, record):
        return any(r.search(record) for r in self.r)


def scan_corpus():
    import corpus as C
    unit = Unit(C.gen_loglike(64 * SCAN_FS, seed=3), SCAN_FS)
    return unit.archive(SCAN_FRAMES)


def group_scan(eng, which):
    import context_model as XM
    import cut_model as CM
    import extract_model as EM
    import extract_regex_model as ERM
    import grep_model as GM
    import msearch_model as MM
    import regex_model as RM
    import search_model as SM
    import tally_model as TM
    import where_model as WM
    arc, content = scan_corpus()
    d_arc = dev(arc)
    A = (eng.h, d_arc.data_ptr(), len(arc))
    P = b"".join(PATS)
    sizes = (ctypes.c_uint32 * len(PATS))(*(len(p) for p in PATS))
    X = b"".join(EXPR)
    xsizes = (ctypes.c_uint32 * len(EXPR))(*(len(p) for p in EXPR))
    R0 = (0, MAXU64, 0)                                                        # the whole content in one window
    kw = dict(offset=LO, length=HI - LO, staging_bytes=STAGING)
    # (a list is scratch too, 16 bytes an entry of the caller's capacity: the wrappers' default of 2^20 entries would not fit either)
    few, many = dict(max_matches=1 << 17), dict(max_records=1 << 16)
    cap, dcap = 4096, 8 << 20
    where = [((0,), (), (1,)), ((), (1, 2), ())]                               # ERROR and not user=42, or one of the other two
    clauses, ncl = Z._clauses(where)
    wmasks = [tuple(WM.mask(t) for t in c) for c in where]
    mask = CM.field_mask("2,4")
    rm = ReMatcher(EXPR)
    some = [content[o:o + n] for o, n in GM.records(content, NL, LO, LO + 40000)]
    slow = RM.Matcher(EXPR, False, NL)
    assert [rm.matches(r) for r in some] == [slow.matches(r) for r in some] and len(some) > 300

    def packed(fn, d_cap=dcap):
        """an extract-like call's (n, size, list) and the bytes it packed, with the buffer's rest checked"""
        out = Dev(d_cap)
        n, size, recs = fn(out.addr, d_cap)
        sync(eng, "extract")
        p = out.rest_problem(size)
        return n, recs, out.head(size), ([p] if p else [])

    def passes(row, n):
        return same("passes", getattr(eng, row + "_stats")()["passes"], n)

    def search():
        want = SM.matches(content, PATS[0], LO, HI)
        n, got = eng.search(A[1], A[2], PATS[0], **few, **kw)
        return same("matches", n, len(want)) + same("match list", got, want) + passes("search", 2)

    def search_multi():
        want = MM.matches_multi(content, PATS, LO, HI)
        n, got, per = eng.search_multi(A[1], A[2], PATS, **few, **kw)
        return same("matches", n, len(want)) + same("match list", got, want) + same("per pattern", per, [sum(1 for _, i in want if i == k) for k in range(len(PATS))])

    def grep():
        _, sel, _ = GM.grep(content, PATS, NL, False, LO, HI)
        n, got = eng.grep(A[1], A[2], PATS, **many, **kw)
        return same("records", n, len(sel)) + same("record list", got, sel) + passes("grep", 2)

    def grep_where():
        _, sel, _ = WM.grep_where(content, PATS, wmasks, NL, False, LO, HI)
        n, got = eng.grep(A[1], A[2], PATS, where=where, **many, **kw)
        return same("records", n, len(sel)) + same("record list", got, sel)

    def grep_regex():
        _, sel, _ = RM.grep_regex(content, EXPR, NL, False, False, LO, HI, matcher=rm)
        n, got = eng.grep_regex(A[1], A[2], EXPR, **many, **kw)
        return same("records", n, len(sel)) + same("record list", got, sel)

    def grep_context():
        listed, nsel, groups, _, _ = XM.context(content, PATS[1:], NL, False, 2, 1, LO, HI)
        n, ns, ng, got = eng.grep_context(A[1], A[2], PATS[1:], before=2, after=1, **many, **kw)
        return same("counts", (n, ns, ng), (len(listed), nsel, groups)) + same("record list", got, listed)

    def extract():
        _, sel, _, text = EM.extract(content, PATS, NL, False, LO, HI)
        n, recs, got, p = packed(lambda a, c: eng.extract(A[1], A[2], PATS, a, c, max_records=1 << 16, **kw))
        return same("records", n, len(sel)) + same("record list", recs, sel) + same("packed text", got, text) + p + passes("extract", 2)

    def extract_regex():
        _, sel, _, text = ERM.extract_regex(content, EXPR, NL, False, False, LO, HI, matcher=rm)
        n, recs, got, p = packed(lambda a, c: eng.extract_regex(A[1], A[2], EXPR, a, c, max_records=1 << 16, **kw))
        return same("records", n, len(sel)) + same("record list", recs, sel) + same("packed text", got, text) + p

    def cut():
        _, sel, _, text = CM.cut(content, PATS, 0x20, mask, NL, False, LO, HI)
        n, recs, got, p = packed(lambda a, c: eng.cut(A[1], A[2], PATS, a, c, separator=0x20, fields=mask, max_records=1 << 16, **kw))
        return same("records", n, len(sel)) + same("record list", recs, sel) + same("packed text", got, text) + p

    def tally():
        text, (nrec, nskip, entries, keys) = TM.tally_fields(content, PATS, 0x20, mask, NL, False, LO, HI)
        work, kbuf = Dev(dcap), Dev(1 << 16)
        n, skipped, got = eng.tally(A[1], A[2], PATS, work.addr, dcap, separator=0x20, fields=mask, d_keys=kbuf.addr, key_cap=1 << 16, **kw)
        sync(eng, "tally")
        lt = eng.last_tally
        probs = same("records, skipped", (n, skipped), (nrec, nskip)) + same("entries", got, entries) + same("workspace", work.head(lt["work_size"]), text)
        probs += same("keys", kbuf.head(lt["key_size"]), keys)
        return probs + [p for p in (work.rest_problem(lt["work_size"]), kbuf.rest_problem(lt["key_size"])) if p]

    lst = lambda: Host(16 * cap)
    multi = (P, sizes, len(PATS))
    cases = {
        "search": ("search", L.ZraHipSearchArchive, lambda: [*A, PATS[0], len(PATS[0]), *R0, Host(8 * cap), cap, Words()], search),
        "search_multi": ("search_multi", L.ZraHipSearchArchiveMulti, lambda: [*A, *multi, *R0, lst(), cap, Words(), Host(8 * len(PATS))], search_multi),
        "grep": ("grep", L.ZraHipGrepArchive, lambda: [*A, *multi, NL, 0, *R0, lst(), cap, Words()], grep),
        "grep where": ("grep", L.ZraHipGrepArchiveWhere, lambda: [*A, *multi, 0, NL, 0, clauses, ncl, *R0, lst(), cap, Words()], grep_where),
        "grep_regex": ("grep", L.ZraHipGrepArchiveRegex, lambda: [*A, X, xsizes, len(EXPR), 0, NL, 0, *R0, lst(), cap, Words()], grep_regex),
        "grep_context": ("grep", L.ZraHipGrepArchiveContext, lambda: [*A, *multi, 0, NL, 0, 2, 1, *R0, lst(), cap, Words(), Words(), Words()], grep_context),
        "extract": ("extract", L.ZraHipExtractRecords, lambda: [*A, *multi, NL, 0, *R0, lst(), cap, Words(), Dev(dcap), dcap, Words()], extract),
        "extract_regex": ("extract", L.ZraHipExtractRecordsRegex, lambda: [*A, X, xsizes, len(EXPR), 0, NL, 0, *R0, lst(), cap, Words(), Dev(dcap), dcap, Words()],
                          extract_regex),
        "cut": ("extract", L.ZraHipCutRecords, lambda: [*A, *multi, 0, NL, 0, 0x20, mask, *R0, lst(), cap, Words(), Dev(dcap), dcap, Words()], cut),
    }
    for name in which:
        if name in cases:
            row, fn, make, fit = cases[name]
            case(eng, "%s: the window" % name, lambda: must_fail(eng, fn, make, own=(row,)) or then_fits(eng, fit))
    if "tally" in which:
        # the composite: its cut fails, so the tally's row and the extract's are zero, the five words too, dWork and dKeys untouched
        make = lambda: [*A, *multi, 0, NL, 0, 0x20, mask, *R0, Dev(dcap), dcap, Words(), 0, Host(24 * 64), 64, Dev(4096), 4096, Words(), Words(), Words(), Words()]
        case(eng, "tally (ZraHipTallyFields): the window of its cut", lambda: must_fail(eng, L.ZraHipTallyFields, make, own=("tally", "extract")) or then_fits(eng, tally))
    if "handle grep" in which:
        # the handle twin: frames 200 to 229 resident, so a pass of the fitting call stages some frames from the cache and decodes the rest
        h = Z.Archive(eng, d_arc.data_ptr(), len(arc), 40 * SCAN_FS)
        fs = SCAN_FS

        def read(frames, plain=content):
            off, size = [f * fs + 7 for f in frames], [fs - 9] * len(frames)
            out = Dev(sum(size))
            h.read(out.addr, off, size, [int(v) for v in np.cumsum([0] + size[:-1])])
            sync(eng, "read")
            return same("handle read", out.head(sum(size)), b"".join(plain[o:o + n] for o, n in zip(off, size)))

        def handle_grep():
            probs = read(range(200, 230))
            s1, c1 = h.stats(), h.scan_stats()
            probs += must_fail(eng, L.ZraHipArchiveGrep, lambda: [h.h, *multi, NL, 0, *R0, lst(), cap, Words()], own=("grep",),
                               also=lambda: same("handle stats", h.stats(), s1) + same("handle scan stats", h.scan_stats(), c1))
            if probs:
                return probs
            _, sel, _ = GM.grep(content, PATS, NL, False, LO, HI)

            def fit():
                n, got = h.grep(PATS, **many, **kw)
                return same("records", n, len(sel)) + same("record list", got, sel) + same("frames staged from the cache", h.scan_stats()["staged"], 30)
            return then_fits(eng, fit) + same("handle stats", h.stats(), s1) + read(range(220, 240))       # (ten resident, ten not)
        case(eng, "handle grep (ZraHipArchiveGrep): the window, some frames resident", handle_grep)
        h.close()


# ---- group: tally_text (ZraHipTallyRecords), ZRA_ALLOC_LIMIT_MIB=11
# 330,000 records of two bytes and a newline, 990,000 bytes, 242 tiles of 4,096. Without a promise the table is sized for 330,000 keys:
# 1.5 * 330,000 + 64 = 495,064 -> 2^19 slots; tally_.tables is asked for 16 * 243 + 2 * 242 * 512 + 3 * 8 * 2^19 = 12,834,608 ->
# 14,439,190 padded, over the limit. The text has 600 distinct keys; max_distinct = 600 sizes 1,024 slots and 276,272 bytes.
# tally_.entries cannot be the first to fail: it asks 24 bytes per distinct key, the table before it at least 36 (3 * 8 * 1.5), and
# both are padded alike.
def group_tally_text(eng):
    import tally_model as TM
    rng = np.random.RandomState(9)
    keys = [bytes([97 + k // 25, 97 + k % 25]) for k in range(600)]
    text = b"".join(keys[i] + b"\n" for i in rng.randint(0, 600, size=330000))
    assert len(set(text.split(b"\n"))) == 601
    nrec, nskip, entries, ktext = TM.tally(text)
    t = dev(b"\xEE" * GUARD + text + b"\xEE" * GUARD)
    p = t.data_ptr() + GUARD

    def fit():
        kbuf = Dev(4096)
        n, skipped, got = eng.tally_text(p, len(text), max_distinct=600, d_keys=kbuf.addr, key_cap=4096)
        sync(eng, "tally")
        probs = same("records, skipped", (n, skipped), (nrec, nskip)) + same("entries", got, entries) + same("keys", kbuf.head(len(ktext)), ktext)
        probs += same("table slots", eng.tally_stats()["table_slots"], TM.slots(nrec, 600))
        r = kbuf.rest_problem(len(ktext))
        return probs + ([r] if r else []) + same("the text and its guards", t.cpu().numpy().tobytes(), b"\xEE" * GUARD + text + b"\xEE" * GUARD)
    make = lambda: [eng.h, p, len(text), NL, 0, Host(24 * 1024), 1024, Dev(4096), 4096, Words(), Words(), Words(), Words()]
    case(eng, "tally_text: tally_.tables", lambda: must_fail(eng, L.ZraHipTallyRecords, make, own=("tally",)) or then_fits(eng, fit))


# ---- group: frames (the calls on whole frames: zra_framepass.h FramePasses::open, zra_verify.hip, zra_records.hip), ZRA_ALLOC_LIMIT_MIB=11
# The scan group's 768 frames of 16 KiB. staging_bytes = 0 is one pass over all of them: sign, diff_signature, index_records, verify
# and the locate sweep (400 record numbers: min(768, 2 * 400) boundary frames at most) ask stage_ for 768 * 16,384 + 64 = 12,582,976
# -> 14,156,104 padded, compare and diff for two halves of that; the limit is 11,534,336. staging_bytes = 4 MiB is 256 slots (128
# pairs): 4,194,368 -> 4,718,920. The byte fetch of read_records is a batch over at most 400 touched frames: 6,553,664 -> 7,373,128.
def group_frames(eng, which):
    import compare_model as PM
    import corpus as C
    import diff_model as DM
    import records_model as RM
    import sign_model as SG
    fs, F, grain = SCAN_FS, SCAN_FRAMES, 4096
    ua, ub = Unit(C.gen_loglike(64 * fs, seed=3), fs), Unit(C.gen_loglike(64 * fs, seed=4), fs)
    arc_a, a = ua.archive(F)
    differ = (5, 200, 201, 447, 448, 600, 767)
    arc_b, b = ua.archive(F, swap={f: (ub, f % 64) for f in differ})
    d_a, d_b = dev(arc_a), dev(arc_b)
    A, B = (d_a.data_ptr(), len(arc_a)), (d_b.data_ptr(), len(arc_b))
    U = len(a)
    wc, dc = 1 << 17, 1 << 20
    three = lambda: [Host(8 * 1024), Host(8 * 1024), Host(8 * 1024), 1024]
    patch_out = lambda: [*three(), Words(), Dev(dc), dc, Words(), Words(), Words()]

    def patch_same(got, want):
        (o, s, do), ao, asz, ds = got
        writes, data, wao, wasz = want
        return (same("writes", list(zip((int(v) for v in o), (int(v) for v in s))), writes) + same("append", (ao, asz, ds), (wao, wasz, len(data))) +
                same("data offsets", [int(v) for v in do], [int(v) for v in np.cumsum([0] + [n for _, n in writes[:-1]])] if writes else []))

    def compare():
        want = PM.ranges(a, b, LO, HI)
        n, nbytes, got = eng.compare(*A, *B, offset=LO, length=HI - LO, staging_bytes=STAGING, max_ranges=wc)
        model = PM.stats(a, b, fs, LO, HI, decoded={f for f in differ if LO // fs <= f <= (HI - 1) // fs}, slots=128, cap=wc)
        return same("ranges", (n, nbytes), (len(want), sum(k for _, k in want))) + same("range list", got, want) + same("stats", eng.compare_stats(), model)

    def diff():
        want = DM.patch(a, b, fs, grain)
        data = Dev(dc)
        got = eng.diff(*A, *B, data.addr, dc, grain=grain, staging_bytes=STAGING)
        sync(eng, "diff")
        r = data.rest_problem(got[3])
        return patch_same(got, want) + same("data", data.head(got[3]), want[1]) + ([r] if r else []) + same("passes", eng.diff_stats()["passes"], 6)

    sig_a = []                                                                 # (the model's signature of A: half a second of Python, once)

    def signature():
        if not sig_a:
            sig_a.append(SG.signature(arc_a, a, fs, grain))
        return sig_a[0]
    W = SG.words(U, fs, grain)
    stride = 1 + fs // grain

    def sign():
        first, count = 250, 270
        out = Dev(8 * W)
        info = eng.sign(A[0], A[1], out.addr, W, grain=grain, first_frame=first, frame_count=count, staging_bytes=STAGING)
        sync(eng, "sign")
        got = np.frombuffer(out.head(8 * W), dtype=np.uint64)
        lo, hi = first * stride, (first + count) * stride
        probs = same("signature", tuple(info), (U, fs, grain, 0, F, W)) + same("words of the range", [int(v) for v in got[lo:hi]], signature()[lo:hi])
        if not (bool((got[:lo] == 0xEEEEEEEEEEEEEEEE).all()) and bool((got[hi:] == 0xEEEEEEEEEEEEEEEE).all())) or out.rest_problem(8 * W):
            probs.append("words outside the range were written")
        return probs + same("passes", eng.sign_stats()["passes"], 2)

    def diff_signature():
        d_sig = dev(np.asarray(signature(), dtype=np.uint64).tobytes())
        want = SG.patch(SG.grain_words(a, fs, grain), U, b, fs, grain)
        data = Dev(dc)
        got = eng.diff_signature((U, fs, grain, 0, F, W), d_sig.data_ptr(), W, *B, data.addr, dc, staging_bytes=STAGING)
        sync(eng, "diff_signature")
        return patch_same(got, want) + same("data", data.head(got[3]), want[1]) + same("writes of the byte diff at this grain", want[0], DM.patch(a, b, fs, grain)[0])

    # the record index of A from the model: a frame's word depends on its content alone, and frame i holds the content of frame i % 64
    w64 = RM.index_words(ua.base, fs, NL)
    words = [w64[i % 64] for i in range(F)]
    D = sum(w & ~RM.BIT63 for w in words)
    index = (U, fs, NL, F, D, D + (a[-1] != NL))
    d_index = dev(np.asarray(words, dtype=np.uint64).tobytes())
    info = Z.ZraHipRecordIndex(*index)
    numbers = [int(v) for v in np.random.RandomState(8).randint(0, index[5], size=400)]
    nums = u64(numbers)
    located = []

    def locate_model():
        if not located:
            located.append(RM.locate(a, NL, numbers))
        return located[0]

    def index_records():
        out = Dev(8 * F)
        got = eng.index_records(A[0], A[1], out.addr, F, staging_bytes=STAGING)
        sync(eng, "index")
        return same("index", tuple(got), index) + same("words", [int(v) for v in np.frombuffer(out.head(8 * F), dtype=np.uint64)], words) + same(
            "passes", eng.index_records_stats()["passes"], 3) + ([out.rest_problem(8 * F)] if out.rest_problem(8 * F) else [])

    def locate_records():
        return same("ranges", eng.locate_records(A[0], A[1], index, d_index.data_ptr(), F, numbers, staging_bytes=STAGING), locate_model())

    def read_records():
        want = locate_model()
        text = b"".join(a[o:o + n] + b"\n" for o, n in want)
        data = Dev(dc)
        size, got = eng.read_records(A[0], A[1], index, d_index.data_ptr(), F, numbers, data.addr, dc, staging_bytes=STAGING)
        sync(eng, "read_records")
        r = data.rest_problem(size)
        return same("ranges", got, want) + same("packed records", data.head(size), text) + ([r] if r else [])

    def verify():
        n, faults = eng.verify(A[0], A[1], staging_bytes=STAGING)
        probs = same("faults of a sound archive", (n, faults), (0, [])) + same(
            "stats", eng.verify_stats(), dict(frames=F, checked=F, structure_faults=0, content_faults=0, decoded=F, content_bytes=U, passes=3))
        frame = ua.frames[300 % 64]
        bad = frame[:-1] + bytes([frame[-1] ^ 0x40])                          # (its content checksum: the block walk is sound, the decode is not)
        plain, code = O.decompress(bad, fs)
        arc_d, _ = ua.archive(F, damage={300: bad})
        d_d = dev(arc_d)
        n, faults = eng.verify(d_d.data_ptr(), len(arc_d), staging_bytes=STAGING)
        return probs + same("the oracle refuses the damaged frame", plain, None) + same("faults of the damaged archive", (n, faults), (1, [(300, code, Z.VERIFY_CONTENT)]))

    ref = ctypes.byref
    sig_info = Z.ZraHipSignature(U, fs, grain, 0, F, W)
    d_zero_sig = dev(bytes(8 * W))
    cases = {
        "compare": ("compare", L.ZraHipCompareArchives, lambda: [eng.h, *A, *B, 0, 0, MAXU64, 0, Host(16 * 1024), 1024, Words(), Words()], compare),
        "diff": ("diff", L.ZraHipDiffArchives, lambda: [eng.h, *A, *B, 0, grain, 0, *patch_out()], diff),
        "sign": ("sign", L.ZraHipSignArchive, lambda: [eng.h, *A, grain, 0, 0, MAXU64, 0, Dev(8 * W), W, Words(5)], sign),
        "diff_signature": ("diff_signature", L.ZraHipDiffSignature, lambda: [eng.h, ref(sig_info), d_zero_sig.data_ptr(), W, *B, 0, 0, *patch_out()], diff_signature),
        "index_records": ("index_records", L.ZraHipIndexRecords, lambda: [eng.h, *A, NL, 0, MAXU64, 0, Dev(8 * F), F, Words(5)], index_records),
        "locate_records": ("locate_records", L.ZraHipLocateRecords, lambda: [eng.h, *A, ref(info), d_index.data_ptr(), F, nums[1], 400, 0, Host(16 * 400)], locate_records),
        "read_records": ("read_records", L.ZraHipReadRecords,
                         lambda: [eng.h, *A, ref(info), d_index.data_ptr(), F, nums[1], 400, 0, Host(16 * 400), Dev(dc), dc, Words()], read_records),
        "verify": ("verify", L.ZraHipVerifyArchive, lambda: [eng.h, *A, Z.VERIFY_CONTENT, 0, MAXU64, 0, Host(16 * 64), 64, Words()], verify),
    }
    for name in which:
        row, fn, make, fit = cases[name]
        case(eng, "%s: the window" % name, lambda: must_fail(eng, fn, make, own=(row,)) or then_fits(eng, fit))


# ---- group: compress (ZraHipCompressBuffer, device pointers), ZRA_ALLOC_LIMIT_MIB=24 (the limit of the host-pointer test in
# tests/test_gpu_parity.py). 64 MiB in frames of 64 KiB are 1,024 frames: at level 3 the persistent path asks for a 384 KiB table slot
# per resident wave (hundreds of MiB) and gives up behind its halved budgets, at level 9 the batch path asks for 1,024 frames' tables at
# once. 180,000 bytes are three frames, whose scratch fits. The input of the failed call is overwritten and freed before the next call.
def group_compress(eng):
    import corpus as C
    fs = 65536
    big = C.gen_E(1 << 20) * 64
    small = C.gen_E(1 << 20)[100000:280000]
    cap_big, cap_small = Z.GetOutputBufferSize(len(big), fs) + 64, Z.GetOutputBufferSize(len(small), fs) + 64
    d_small = dev(small)
    for level in (3, 9):
        st, ref_arc = O.zra_compress(small, level, fs, True, 0, "zo")
        assert st == (0, 0)
        d_big = [dev(big)]

        def fit():
            out = Dev(cap_small)
            n = eng.compress(d_small.data_ptr(), len(small), out.addr, level, fs, True)
            sync(eng, "compress")
            r = out.rest_problem(n)
            return same("archive against the oracle's", out.head(n), ref_arc) + ([r] if r else [])

        def run():
            probs = must_fail(eng, L.ZraHipCompressBuffer, lambda: [eng.h, d_big[0].data_ptr(), len(big), Dev(cap_big), SizeWord(), level, fs, True])
            d_big[0].fill_(0xEE)                                               # what a caller does after an error: the buffer is gone
            d_big.clear()
            return probs or then_fits(eng, fit)
        case(eng, "compress level %d: the encoder's scratch" % level, run)


GROUPS = {"decode": group_decode, "ra": group_ra, "tally_text": group_tally_text,
          "scan_a": lambda eng: group_scan(eng, ("search", "search_multi", "grep", "grep where", "grep_regex", "grep_context")),
          "scan_b": lambda eng: group_scan(eng, ("extract", "extract_regex", "cut", "tally", "handle grep")),
          "frames_a": lambda eng: group_frames(eng, ("compare", "diff", "sign", "diff_signature")),
          "frames_b": lambda eng: group_frames(eng, ("index_records", "locate_records", "read_records", "verify")), "compress": group_compress}


def main(group):
    global Z, L, torch, O
    import torch as _torch
    import oracle_lib
    import zra_amd
    Z, torch, O = zra_amd, _torch, oracle_lib
    L = Z.load()
    eng = Z.Engine(0)
    GROUPS[group](eng)
    sync(eng, "end of " + group)
    print(json.dumps({"case": "end of " + group, "ok": True, "problems": [], "s": 0}), flush=True)
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1])
