"""Frame writer for the decoder's conformance suite — TEST INFRASTRUCTURE ONLY (nothing in zra_amd/ may import it).

Assembles VALID zstd frames from an explicit description, written from the format specification (RFC 8878): frames that no
one-shot encoder of libzstd 1.4.9 writes, but that every conforming decoder has to take. The writer REFUSES (CraftError) whatever it
cannot encode exactly as asked; it never substitutes an easier form.

A frame is a dict:
  single_segment (bool), window ((exponent, mantissa) or None), fcs_width (0/1/2/4/8), checksum (bool), dict_width (0/1/2/4),
  blocks: a list of
    ("raw", bytes) | ("rle", byte, count) | ("compressed", {...}) with
      lits (bytes), lit_mode ("raw" | "rle" | "huf1" | "huf4" | "treeless1" | "treeless4"), size_format (None = minimal, or 0..3),
      weights ("direct" | "fse"), max_bits (<= 11),
      seqs [(litLength, matchLength, offsetValue)] — offsetValue as on the wire: 1..3 are the repeat codes, offset + 3 otherwise,
      modes {"ll" | "of" | "ml": "predef" | "rle" | "fse" | "repeat"}, logs {table: accuracy log}, extra {table: [unused codes that get
      a "less than one" probability]}, count_width (None = minimal, or 1 / 2 / 3).
  For the error cases only: reserved (bool) sets the reserved header bit, dict_value puts a non-zero dictionary ID, invalid_offset
  lets an offset reach before the frame. over_limit (bool) lets a block regenerate more than 128 KiB — not a valid frame either: the
  largest match length (131,074) and literal length (131,071) the codes can express exist only in such a block, and what libzstd does
  with it is the expectation.

plaintext(frame) computes what the frame regenerates from the description alone (literals plus a plain LZ copy loop with the repeat
offset rules); it calls neither the writer nor any decoder.
"""
import bisect
import heapq
import struct

BLOCK_MAX = 128 << 10
M64 = (1 << 64) - 1


class CraftError(ValueError):
    """the description asks for something the format cannot hold as asked"""


# ------------------------------------------------------------------------------------------------ code tables (RFC 8878, 3.1.1.3.2.1)
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
PREDEF = {
    "ll": (6, [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]),
    "ml": (6, [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7),
    "of": (5, [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5),
}
MAX_SYM = {"ll": 35, "of": 31, "ml": 52}
MAX_LOG = {"ll": 9, "of": 8, "ml": 9}
MODE_ID = {"predef": 0, "rle": 1, "fse": 2, "repeat": 3}


def ll_code(v):
    if v > 131071:
        raise CraftError("literal length %d has no code" % v)
    c = bisect.bisect_right(LL_BASE, v) - 1
    return c, v - LL_BASE[c], LL_BITS[c]


def ml_code(v):
    if v < 3 or v > 131074:
        raise CraftError("match length %d has no code" % v)
    c = bisect.bisect_right(ML_BASE, v) - 1
    return c, v - ML_BASE[c], ML_BITS[c]


def of_code(v):
    if v < 1 or v >= (1 << 32):
        raise CraftError("offset value %d has no code" % v)
    c = v.bit_length() - 1
    return c, v - (1 << c), c


# ------------------------------------------------------------------------------------------------ bit streams
class BackBits:
    """A stream the decoder reads backward. Fields are collected in the DECODER's read order and written out in reverse, closed by
    the end mark (a single 1 bit above the last field)."""

    def __init__(self):
        self.f = []

    def read(self, value, nbits):
        if nbits:
            if value >> nbits:
                raise CraftError("field does not fit its width")
            self.f.append((value, nbits))

    def bytes(self):
        out = bytearray()
        acc = n = 0
        for v, k in reversed(self.f):
            acc |= v << n
            n += k
            while n >= 8:
                out.append(acc & 0xFF)
                acc >>= 8
                n -= 8
        acc |= 1 << n
        out.append(acc)
        return bytes(out)


# ------------------------------------------------------------------------------------------------ FSE (RFC 8878, 4.1)
def fse_normalize(counts, log, extra=()):
    """{symbol: count} -> normalised counts (list up to the last symbol present) summing to 1 << log; `extra` symbols get -1."""
    size = 1 << log
    used = {s: c for s, c in counts.items() if c > 0}
    low = [s for s in extra if s not in used]
    room = size - len(low)
    if not used or len(used) > room:
        raise CraftError("%d symbols do not fit an accuracy log of %d" % (len(used) + len(low), log))
    if len(used) == 1 and not low:
        raise CraftError("a single symbol needs RLE mode")
    total = sum(used.values())
    norm = {s: max(1, c * room // total) for s, c in used.items()}
    diff = room - sum(norm.values())
    order = sorted(used, key=lambda s: -used[s])
    k = 0
    while diff:
        s = order[k % len(order)]
        if diff > 0:
            norm[s] += 1
            diff -= 1
        elif norm[s] > 1:
            norm[s] -= 1
            diff += 1
        k += 1
    for s in low:
        norm[s] = -1
    top = max(norm)
    return [norm.get(s, 0) for s in range(top + 1)]


def fse_write_ncount(norm, log):
    """the table description: accuracy log, then every count in a field whose width follows what is left, zero runs by 2-bit flags"""
    acc = log - 5
    n = 4
    remaining = (1 << log) + 1
    threshold = 1 << log
    nbits = log + 1
    sym = 0
    prev0 = False
    alpha = len(norm)
    while sym < alpha and remaining > 1:
        if prev0:
            start = sym
            while sym < alpha and norm[sym] == 0:
                sym += 1
            if sym == alpha:
                raise CraftError("distribution ends in a zero run")
            while sym >= start + 24:
                start += 24
                acc |= 0xFFFF << n
                n += 16
            while sym >= start + 3:
                start += 3
                acc |= 3 << n
                n += 2
            acc |= (sym - start) << n
            n += 2
        c = norm[sym]
        sym += 1
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        c += 1
        if c >= threshold:
            c += mx
        acc |= c << n
        n += nbits - (1 if c < mx else 0)
        prev0 = c == 1
        if remaining < 1:
            raise CraftError("distribution exceeds its table")
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
    if remaining != 1 or sym != alpha:
        raise CraftError("distribution does not fill its table")
    return acc.to_bytes((n + 7) // 8, "little")


class FseTable:
    """decoding table of a distribution, and the encoder derived from it: for a symbol and the state the decoder goes to next, the one
    state that emits the symbol and whose transition reaches that next state"""

    def __init__(self, norm=None, log=0, rle=None):
        self.norm, self.log, self.rle = norm, log, rle
        if rle is not None:
            self.log = 0
            self.syms = {rle}
            return
        size = 1 << log
        table = [None] * size
        high = size - 1
        for s, c in enumerate(norm):
            if c == -1:
                table[high] = s
                high -= 1
        pos = 0
        step = (size >> 1) + (size >> 3) + 3
        for s, c in enumerate(norm):
            for _ in range(max(c, 0)):
                table[pos] = s
                pos = (pos + step) & (size - 1)
                while pos > high:
                    pos = (pos + step) & (size - 1)
        if pos != 0 or None in table:
            raise CraftError("distribution does not fill its table")
        nxt = [1 if c == -1 else c for c in norm]
        self.by_sym = {}
        for state, s in enumerate(table):
            x = nxt[s]
            nxt[s] += 1
            nb = log - (x.bit_length() - 1)
            base = (x << nb) - size
            self.by_sym.setdefault(s, []).append((base, nb, state))
        for v in self.by_sym.values():
            v.sort()
        self.syms = set(self.by_sym)
        self.nb_of = {}
        for v in self.by_sym.values():
            for base, nb, state in v:
                self.nb_of[state] = nb

    def last_state(self, sym):
        if self.rle is not None:
            return 0
        return max(self.by_sym[sym], key=lambda e: e[1])[2]          # any state of the symbol will do; one that has bits to read

    def prev_state(self, sym, nxt):
        """(state, transition bits value, width) of the state that emits `sym` and then moves to `nxt`"""
        if self.rle is not None:
            return 0, 0, 0
        v = self.by_sym[sym]
        i = bisect.bisect_right(v, (nxt, 99, 1 << 30)) - 1
        base, nb, state = v[i]
        assert base <= nxt < base + (1 << nb)
        return state, nxt - base, nb


# ------------------------------------------------------------------------------------------------ Huffman (RFC 8878, 4.2)
def huf_lengths(counts, max_bits):
    """code lengths of a complete prefix code for {symbol: count}, none above max_bits"""
    syms = sorted(counts)
    if len(syms) < 2:
        raise CraftError("a Huffman tree needs two symbols")
    if len(syms) > (1 << max_bits):
        raise CraftError("%d symbols do not fit %d bits" % (len(syms), max_bits))
    heap = [(counts[s], s, None, None) for s in syms]
    heapq.heapify(heap)
    tick = 256
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, a, b))
        tick += 1
    ln = {}
    stack = [(heap[0], 0)]
    while stack:
        (c, s, a, b), d = stack.pop()
        if a is None:
            ln[s] = d
        else:
            stack.append((a, d + 1))
            stack.append((b, d + 1))
    L = max_bits
    for s in ln:
        ln[s] = min(ln[s], L)
    kraft = sum(1 << (L - v) for v in ln.values())
    full = 1 << L
    while kraft > full:                                      # too many short codes after the clamp: lengthen the longest one below L
        s = max((s for s in ln if ln[s] < L), key=lambda s: (ln[s], -counts[s]))
        kraft -= 1 << (L - ln[s] - 1)
        ln[s] += 1
    while kraft < full:                                      # room left: shorten whatever fits the gap
        cand = [s for s in ln if ln[s] > 1 and (1 << (L - ln[s])) <= full - kraft]
        if not cand:
            raise CraftError("no complete code within %d bits" % max_bits)
        s = max(cand, key=lambda s: (-ln[s], counts[s]))
        kraft += 1 << (L - ln[s])
        ln[s] -= 1
    return ln


class HufTable:
    def __init__(self, lengths):
        self.max_bits = max(lengths.values())
        self.weights = {s: self.max_bits + 1 - l for s, l in lengths.items()}
        self.code = {}
        pos = 0
        for w in range(1, self.max_bits + 1):
            for s in sorted(lengths):
                if self.weights[s] == w:
                    nb = self.max_bits + 1 - w
                    self.code[s] = (pos >> (w - 1), nb)
                    pos += 1 << (w - 1)
        if pos != 1 << self.max_bits:
            raise CraftError("code lengths are not a complete code")

    def describe(self, how):
        """tree description: the weights of every symbol below the last one (whose weight is implied)"""
        last = max(self.weights)
        ws = [self.weights.get(s, 0) for s in range(last)]
        if how == "direct":
            if len(ws) > 128:
                raise CraftError("%d weights do not fit the direct form" % len(ws))
            out = bytearray([127 + len(ws)])
            for i in range(0, len(ws), 2):
                out.append((ws[i] << 4) | (ws[i + 1] if i + 1 < len(ws) else 0))
            return bytes(out)
        if how != "fse":
            raise CraftError("weights form %r" % (how,))
        if len(ws) < 2:
            raise CraftError("the compressed form needs two weights")
        cnt = {}
        for w in ws:
            cnt[w] = cnt.get(w, 0) + 1
        if len(cnt) < 2:
            raise CraftError("weights of one value only: the compressed form cannot hold them")
        log = 6
        while log > 5 and (1 << (log - 1)) >= len(ws):
            log -= 1
        norm = fse_normalize(cnt, log)
        t = FseTable(norm, log)
        # two interleaved states; the decoder's last two symbols come from states that have no transition left to read
        chains = (ws[0::2], ws[1::2])
        states = []
        for ch in chains:
            st = [0] * len(ch)
            tr = [None] * len(ch)
            st[-1] = t.last_state(ch[-1])
            for k in range(len(ch) - 2, -1, -1):
                st[k], v, nb = t.prev_state(ch[k], st[k + 1])
                tr[k] = (v, nb)
            states.append((st, tr))
        bb = BackBits()
        bb.read(states[0][0][0], log)
        bb.read(states[1][0][0], log)
        for k in range(len(ws) - 2):
            v, nb = states[k & 1][1][k >> 1]
            bb.read(v, nb)
        stop = states[len(ws) & 1][0][-1]                    # the state that emits the last symbol but one: its read must overrun
        if t.nb_of[stop] == 0:
            raise CraftError("weight stream cannot end here")
        body = fse_write_ncount(norm, log) + bb.bytes()
        if len(body) >= 128:
            raise CraftError("compressed weights take %d bytes" % len(body))
        return bytes([len(body)]) + body

    def stream(self, lits):
        bb = BackBits()
        for b in lits:
            c = self.code.get(b)
            if c is None:
                raise CraftError("literal %d is not in the tree in force" % b)
            bb.read(c[0], c[1])
        return bb.bytes()


# ------------------------------------------------------------------------------------------------ XXH64 (the frame checksum)
_P1, _P2, _P3, _P4, _P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc, v):
    return (_rotl((acc + v * _P2) & M64, 31) * _P1) & M64


def xxh64(data, seed=0):
    n = len(data)
    p = 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & M64, (seed + _P2) & M64, seed, (seed - _P1) & M64]
        words = struct.unpack_from("<%dQ" % (n // 32 * 4), data)
        for i in range(0, len(words), 4):
            v[0] = _round(v[0], words[i]); v[1] = _round(v[1], words[i + 1]); v[2] = _round(v[2], words[i + 2]); v[3] = _round(v[3], words[i + 3])
        p = n // 32 * 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
        for x in v:
            h = ((h ^ _round(0, x)) * _P1 + _P4) & M64
    else:
        h = (seed + _P5) & M64
    h = (h + n) & M64
    while p + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, p)[0]), 27) * _P1 + _P4) & M64
        p += 8
    if p + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, p)[0] * _P1 & M64), 23) * _P2 + _P3) & M64
        p += 4
    while p < n:
        h = (_rotl(h ^ (data[p] * _P5 & M64), 11) * _P1) & M64
        p += 1
    h ^= h >> 33; h = h * _P2 & M64
    h ^= h >> 29; h = h * _P3 & M64
    h ^= h >> 32
    return h


# ------------------------------------------------------------------------------------------------ the reference of the operation
def block_sizes(frame):
    """regenerated size of every block, from the description alone"""
    out = []
    for b in frame["blocks"]:
        if b[0] == "raw":
            out.append(len(b[1]))
        elif b[0] == "rle":
            out.append(b[2])
        else:
            out.append(len(b[1]["lits"]) + sum(s[1] for s in b[1].get("seqs", ())))
    return out


def rep_step(rep, ll, ov):
    """(offset, repeat offsets afterwards) of a sequence with offset value `ov` behind `ll` literals (RFC 8878, 3.1.1.5)"""
    if ov > 3:
        return ov - 3, [ov - 3, rep[0], rep[1]]
    k = ov - 1 + (1 if ll == 0 else 0)
    if k == 0:
        return rep[0], rep
    off = rep[k] if k < 3 else rep[0] - 1
    if off == 0:
        off = 1                                              # not valid; libzstd takes the offset for 1 and goes on (the one case whose expectation is libzstd's)
    return off, [off, rep[0], rep[2] if k == 1 else rep[1]]


def plaintext(frame, check=True):
    """What the frame regenerates. check=False: an offset beyond the output is not an error here (None is returned instead)."""
    out = bytearray()
    rep = [1, 4, 8]
    for b in frame["blocks"]:
        if b[0] == "raw":
            out += b[1]
            continue
        if b[0] == "rle":
            out += bytes([b[1]]) * b[2]
            continue
        lits = b[1]["lits"]
        lp = 0
        for ll, ml, ov in b[1].get("seqs", ()):
            out += lits[lp:lp + ll]
            lp += ll
            off, rep = rep_step(rep, ll, ov)
            if off > len(out):
                if check:
                    raise CraftError("offset %d beyond the %d bytes produced" % (off, len(out)))
                return None
            st = len(out) - off
            if off >= ml:
                out += out[st:st + ml]
            else:
                chunk = bytes(out[st:])
                out += (chunk * (ml // off + 1))[:ml]
        if lp > len(lits):
            raise CraftError("sequences use more literals than the block has")
        out += lits[lp:]
    return bytes(out)


# ------------------------------------------------------------------------------------------------ the writer
class _State:
    def __init__(self):
        self.huf = None
        self.tab = {"ll": None, "of": None, "ml": None}


def _literals(c, st):
    lits = c["lits"]
    mode = c.get("lit_mode", "raw")
    sf = c.get("size_format")
    n = len(lits)
    if mode in ("raw", "rle"):
        if mode == "rle" and (n < 1 or lits != lits[:1] * n):
            raise CraftError("RLE literals of more than one value")
        need = 0 if n < 32 else 1 if n < 4096 else 3
        if sf is None:
            sf = need
        if sf not in (0, 1, 3) or sf < need or n >= (1 << 20):
            raise CraftError("size format %r cannot hold %d literals" % (sf, n))
        t = 0 if mode == "raw" else 1
        if sf == 0:
            h = bytes([t | (n << 3)])
        elif sf == 1:
            h = struct.pack("<H", t | (1 << 2) | (n << 4))
        else:
            h = (t | (3 << 2) | (n << 4)).to_bytes(3, "little")
        return h + (lits if mode == "raw" else lits[:1])
    if mode not in ("huf1", "huf4", "treeless1", "treeless4"):
        raise CraftError("literals mode %r" % (mode,))
    if n == 0:
        raise CraftError("no literals to compress")
    treeless = mode.startswith("treeless")
    four = mode.endswith("4")
    if treeless:
        if st.huf is None:
            raise CraftError("treeless literals with no tree in force")
        tree = b""
        huf = st.huf
    else:
        cnt = {}
        for b in lits:
            cnt[b] = cnt.get(b, 0) + 1
        huf = HufTable(huf_lengths(cnt, c.get("max_bits", 11)))
        if huf.max_bits > 11:
            raise CraftError("tree deeper than 11 bits")
        tree = huf.describe(c.get("weights", "fse"))
    if four:
        seg = (n + 3) // 4
        if 3 * seg > n:
            raise CraftError("%d literals do not split into four streams" % n)
        parts = [huf.stream(lits[k * seg:(k + 1) * seg]) for k in range(3)] + [huf.stream(lits[3 * seg:])]
        if any(len(p) > 0xFFFF for p in parts[:3]):
            raise CraftError("stream above 64 KiB")
        body = struct.pack("<3H", *(len(p) for p in parts[:3])) + b"".join(parts)
    else:
        body = huf.stream(lits)
    csize = len(tree) + len(body)
    need = 0 if not four else 1
    if max(n, csize) >= 1024:
        if not four:
            raise CraftError("one stream holds at most 1,023 literals")
        need = 2 if max(n, csize) < 16384 else 3
    if max(n, csize) >= (1 << 18):
        raise CraftError("literals section too large")
    if sf is None:
        sf = need
    if sf not in (0, 1, 2, 3) or (sf == 0) != (not four) or sf < need:
        raise CraftError("size format %r cannot hold %d / %d" % (sf, n, csize))
    bits = 10 if sf < 2 else 14 if sf == 2 else 18
    t = 3 if treeless else 2
    h = (t | (sf << 2) | (n << 4) | (csize << (4 + bits))).to_bytes(3 if sf < 2 else sf + 2, "little")
    st.huf = huf
    return h + tree + body


def _sequences(c, st):
    seqs = c.get("seqs", [])
    n = len(seqs)
    cw = c.get("count_width")
    need = 1 if n < 128 else 2 if n < 0x7F00 else 3
    if cw is None:
        cw = need
    if n == 0:
        if cw != 1:
            raise CraftError("zero sequences take the one-byte count")
        return b"\0"
    if n > 0x7F00 + 0xFFFF or cw < need or cw > 3 or (cw == 3 and n < 0x7F00):
        raise CraftError("count of %d does not fit the %d-byte field" % (n, cw))
    out = bytearray([n] if cw == 1 else [0x80 + (n >> 8), n & 0xFF] if cw == 2 else [0xFF, (n - 0x7F00) & 0xFF, (n - 0x7F00) >> 8])
    codes = {"ll": [ll_code(s[0]) for s in seqs], "ml": [ml_code(s[1]) for s in seqs], "of": [of_code(s[2]) for s in seqs]}
    modes = c.get("modes", {})
    tabs = {}
    desc = {}
    for k in ("ll", "of", "ml"):
        m = modes.get(k, "predef")
        used = {}
        for code, _, _ in codes[k]:
            used[code] = used.get(code, 0) + 1
        extra = [s for s in c.get("extra", {}).get(k, ())]
        if any(s > MAX_SYM[k] for s in extra) or max(used) > MAX_SYM[k]:
            raise CraftError("%s code above %d" % (k, MAX_SYM[k]))
        if m == "predef":
            log, norm = PREDEF[k]
            t = FseTable(norm, log)
            desc[k] = b""
        elif m == "rle":
            if len(used) != 1:
                raise CraftError("RLE mode for %d distinct %s codes" % (len(used), k))
            sym = next(iter(used))
            t = FseTable(rle=sym)
            desc[k] = bytes([sym])
        elif m == "fse":
            log = c.get("logs", {}).get(k, 6)
            if log < 5 or log > MAX_LOG[k]:
                raise CraftError("accuracy log %d for %s" % (log, k))
            norm = fse_normalize(used, log, extra)
            t = FseTable(norm, log)
            desc[k] = fse_write_ncount(norm, log)
        elif m == "repeat":
            t = st.tab[k]
            if t is None:
                raise CraftError("repeat mode with no %s table in force" % k)
            desc[k] = b""
        else:
            raise CraftError("table mode %r" % (m,))
        if not set(used) <= t.syms:
            raise CraftError("%s codes %s are not in the table in force" % (k, sorted(set(used) - t.syms)))
        tabs[k] = t
    out.append((MODE_ID[modes.get("ll", "predef")] << 6) | (MODE_ID[modes.get("of", "predef")] << 4) | (MODE_ID[modes.get("ml", "predef")] << 2))
    out += desc["ll"] + desc["of"] + desc["ml"]
    # the decoder's states, found backward from the last sequence
    states = {}
    trans = {}
    for k in ("ll", "of", "ml"):
        t = tabs[k]
        s = [0] * n
        tr = [None] * n
        s[-1] = t.last_state(codes[k][-1][0])
        for i in range(n - 2, -1, -1):
            s[i], v, nb = t.prev_state(codes[k][i][0], s[i + 1])
            tr[i] = (v, nb)
        states[k], trans[k] = s, tr
    bb = BackBits()
    for k in ("ll", "of", "ml"):
        bb.read(states[k][0], tabs[k].log)
    for i in range(n):
        for k in ("of", "ml", "ll"):
            bb.read(codes[k][i][1], codes[k][i][2])
        if i + 1 < n:
            for k in ("ll", "ml", "of"):
                bb.read(*trans[k][i])
    out += bb.bytes()
    for k in ("ll", "of", "ml"):
        st.tab[k] = tabs[k]
    return bytes(out)


def window_size(frame):
    if frame.get("single_segment"):
        return sum(block_sizes(frame))
    e, m = frame["window"]
    return (1 << (10 + e)) + ((1 << (10 + e)) >> 3) * m


def write_frame(frame, info=None):
    """the frame's bytes; CraftError for whatever cannot be written as described. info: a list that receives, per compressed block,
    (regenerated literals, size of the literals section's payload) — what libzstd's choice between its two Huffman decoders goes by."""
    content = plaintext(frame, check=not frame.get("invalid_offset"))
    sizes = block_sizes(frame)
    total = sum(sizes)
    ss = bool(frame.get("single_segment"))
    fw = frame.get("fcs_width", 0)
    dw = frame.get("dict_width", 0)
    if fw not in (0, 1, 2, 4, 8) or dw not in (0, 1, 2, 4):
        raise CraftError("field width")
    if (fw == 1 and not ss) or (fw == 0 and ss):
        raise CraftError("content-size width %d %s single-segment" % (fw, "with" if ss else "without"))
    if ss == ("window" in frame and frame["window"] is not None):
        raise CraftError("a frame has a window descriptor or is single-segment")
    if fw == 1 and total > 255 or fw == 2 and not 256 <= total <= 65535 + 256 or fw == 4 and total >= (1 << 32):
        raise CraftError("content size %d does not fit %d bytes" % (total, fw))
    if not ss and not (0 <= frame["window"][0] <= 31 and 0 <= frame["window"][1] <= 7):
        raise CraftError("window descriptor")
    win = window_size(frame)
    if not frame["blocks"]:
        raise CraftError("a frame has at least one block")
    fhd = ({0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fw] << 6) | (ss << 5) | (bool(frame.get("reserved")) << 3) | (bool(frame.get("checksum")) << 2) | {0: 0, 1: 1, 2: 2, 4: 3}[dw]
    out = bytearray(struct.pack("<IB", 0xFD2FB528, fhd))
    if not ss:
        out.append((frame["window"][0] << 3) | frame["window"][1])
    out += int(frame.get("dict_value", 0)).to_bytes(dw, "little")
    if fw:
        out += (total - 256 if fw == 2 else total).to_bytes(fw, "little")
    st = _State()
    for i, b in enumerate(frame["blocks"]):
        last = i == len(frame["blocks"]) - 1
        size = sizes[i]
        if (size > BLOCK_MAX and not frame.get("over_limit")) or size > win:
            raise CraftError("block of %d bytes above the block limit or the window" % size)
        if b[0] == "raw":
            out += (int(last) | (0 << 1) | (size << 3)).to_bytes(3, "little") + b[1]
        elif b[0] == "rle":
            out += (int(last) | (1 << 1) | (size << 3)).to_bytes(3, "little") + bytes([b[1]])
        elif b[0] == "compressed":
            c = b[1]
            if sum(s[0] for s in c.get("seqs", ())) > len(c["lits"]):
                raise CraftError("sequences use more literals than the block has")
            if not frame.get("invalid_offset"):
                for s in c.get("seqs", ()):
                    if s[2] > 3 and s[2] - 3 > win:
                        raise CraftError("offset %d beyond the window" % (s[2] - 3))
            lsec = _literals(c, st)
            if info is not None:
                sf = (lsec[0] >> 2) & 3                          # header length of the section just written
                hl = (3 if sf < 2 else sf + 2) if lsec[0] & 2 else (1, 2, 1, 3)[sf]
                info.append((len(c["lits"]), len(lsec) - hl))
            body = lsec + _sequences(c, st)
            if len(body) >= BLOCK_MAX or len(body) < 3:
                raise CraftError("compressed block of %d bytes" % len(body))
            out += (int(last) | (2 << 1) | (len(body) << 3)).to_bytes(3, "little") + body
        else:
            raise CraftError("block type %r" % (b[0],))
    if frame.get("checksum"):
        out += struct.pack("<I", xxh64(content if content is not None else b"") & 0xFFFFFFFF)
    return bytes(out)


# ================================================================================================ descriptions: helpers
def _rng(seed):
    import numpy as np
    return np.random.RandomState(seed)


def _pick(rng, seq):
    return seq[int(rng.randint(0, len(seq)))]


def _bytes(rng, n, alpha=256, lo=0):
    import numpy as np
    return bytes(rng.randint(lo, lo + alpha, size=n).astype(np.uint8).tolist()) if n else b""


def to_wire(rng, rep, ll, off, p_rep=1.0):
    """offset value for `off` behind `ll` literals: a repeat code where one stands for it (with probability p_rep)"""
    if rng.rand() < p_rep:
        for ov in (1, 2, 3):
            if rep_step(rep, ll, ov)[0] == off and not (ov == 3 and ll == 0 and rep[0] == 1):
                return ov
    return off + 3


def gen_block(rng, size, produced, rep, first=(), alpha=40, max_off=1 << 17, max_seq=400, p_rep=0.5, lens=(3, 4, 5, 8, 12, 40, 300), ll_max=12):
    """(lits, seqs, rep afterwards) of a compressed block that regenerates exactly `size` bytes behind `produced` bytes of output;
    `first`: sequences the block opens with, as (ll, ml, offsetValue)."""
    seqs = []
    nl = 0
    done = 0
    rep = list(rep)
    for ll, ml, ov in first:
        off, rep = rep_step(rep, ll, ov)
        if off > produced + done + ll:
            raise CraftError("opening sequence reaches before the frame")
        seqs.append((ll, ml, ov))
        nl += ll
        done += ll + ml
    if done > size:
        raise CraftError("opening sequences exceed the block")
    while len(seqs) < max_seq:
        ll = int(rng.randint(0, ll_max + 1))
        ml = int(_pick(rng, lens))
        if done + ll + ml > size:
            break
        here = produced + done + ll
        if here == 0:
            ll = max(ll, 1)
            continue
        r = rng.rand()
        if r < p_rep:                                        # one of the offsets that a repeat code stands for here
            off = rep_step(rep, ll, int(rng.randint(1, 4)))[0]
        elif r < p_rep + 0.1:
            off = int(rng.randint(1, 17))
        else:
            off = int(rng.randint(1, min(here, max_off) + 1))
        if off > min(here, max_off):
            off = int(rng.randint(1, min(here, max_off) + 1))
        ov = to_wire(rng, rep, ll, off, 0.9)
        _, rep = rep_step(rep, ll, ov)
        seqs.append((ll, ml, ov))
        nl += ll
        done += ll + ml
    nl += size - done
    return _bytes(rng, nl, alpha), seqs, rep


def cblock(lits, seqs=(), **kw):
    return ("compressed", dict(lits=lits, seqs=list(seqs), **kw))


def frame_of(blocks, **kw):
    fr = dict(blocks=blocks)
    fr.update(kw)
    if "window" not in fr and "single_segment" not in fr:
        fr["single_segment"] = True
        fr.setdefault("fcs_width", 4)
    return fr


def _geometry(rng, sizes, kinds=None, **kw):
    """a frame whose blocks regenerate `sizes`; kinds[i] in "c" (compressed), "r" (raw), "l" (RLE), "z" (compressed, no sequences)"""
    blocks = []
    produced = 0
    rep = [1, 4, 8]
    for i, n in enumerate(sizes):
        k = kinds[i] if kinds else "c"
        if k == "r":
            blocks.append(("raw", _bytes(rng, n, 7)))
        elif k == "l":
            blocks.append(("rle", int(rng.randint(0, 256)), n))
        elif k == "z":
            blocks.append(cblock(_bytes(rng, n, 9), lit_mode="huf4" if n > 64 else "raw"))
        else:
            lits, seqs, rep = gen_block(rng, n, produced, rep, alpha=30, lens=(3, 4, 5, 8, 12, 40, 300, 3000) if n > 20000 else (3, 4, 5, 8, 12, 40))
            lm = "huf4" if len(lits) > 64 and len(set(lits)) > 1 else "raw"
            blocks.append(cblock(lits, seqs, lit_mode=lm))
        produced += n
    return frame_of(blocks, **kw)


def _case(out, name, tags, frame, error=False):
    out.append(dict(name=name, tags=tags, frame=frame, error=error))


# ================================================================================================ directed cases
def directed_cases():
    """[{name, tags, frame, error}] — every entry a frame description; error: the frame is invalid on purpose (status compared)"""
    C = []
    rng = _rng(20240)
    # ---- block geometry
    _case(C, "geom_short_nonlast_mixed", ["geometry", "short_nonlast"], _geometry(rng, [1, 1000, 65536, 131071, 131072, 777], checksum=True))
    _case(C, "geom_only_second_to_last_short", ["geometry", "short_nonlast"], _geometry(rng, [131072, 100000, 31072]))
    _case(C, "geom_first_short_then_full", ["geometry", "short_nonlast"], _geometry(rng, [5, 131072, 131067], checksum=True))
    _case(C, "geom_40_blocks", ["geometry", "many_blocks"], _geometry(rng, [6144 + 13 * i for i in range(40)], checksum=True))
    _case(C, "geom_interleaved_kinds", ["geometry", "short_nonlast"], _geometry(rng, [3000, 500, 70000, 131072, 40000, 9, 17000], "crlczrc", checksum=True))
    _case(C, "geom_empty_raw_last", ["geometry"], _geometry(rng, [131072, 50000, 0], "ccr"))
    _case(C, "geom_empty_raw_last_checksum", ["geometry"], _geometry(rng, [131072, 0], "cr", checksum=True))
    _case(C, "geom_zero_seq_middle_and_last", ["geometry", "short_nonlast"], _geometry(rng, [131072, 20000, 60000, 300], "czcz"))
    for n in (1, 2, 3):
        lits, seqs, _ = gen_block(rng, 4000, 131072, [1, 4, 8], max_seq=n, lens=(3, 40, 300), p_rep=0.0)
        fr = _geometry(rng, [131072])
        fr["blocks"].append(cblock(lits, seqs))
        _case(C, "geom_%d_sequences" % n, ["geometry", "short_bitstream"], fr)
    for n in (127, 128, 0x7EFF, 0x7F00, 0x7F01 + 5):
        # 3-byte matches over a 4-symbol alphabet: ll 1, ml 3, offsets 1..16
        lits = _bytes(rng, n + 40, 4, 97)
        seqs = [(20, 3, 4)] + [(1, 3, int(rng.randint(1, 17)) + 3) for _ in range(n - 1)]
        fr = frame_of([cblock(lits, seqs, lit_mode="huf4" if n > 1000 else "raw", modes=dict(ll="fse", of="fse", ml="rle")), ("raw", b"tail")])
        _case(C, "geom_count_%d" % n, ["geometry", "count3" if n >= 0x7F00 else "count12"], fr)
    fr = frame_of([cblock(_bytes(rng, 300, 4, 97), [(20, 3, 4)] + [(1, 3, 5)] * 99, count_width=2)])
    _case(C, "geom_count_100_in_two_bytes", ["geometry", "count12"], fr)
    # every position of the end mark: one more single-bit field per case (ll code 16 has 1 extra bit; vary through the match-length extra)
    seen = set()
    k = 0
    while len(seen) < 8 and k < 400:
        ll = [0, 16, 24, 64][k % 4]
        ml = [3, 35, 43, 51, 67, 99, 131, 259, 515][k % 9]
        of = [4, 5, 7, 11, 19][k % 5]
        lits = _bytes(rng, ll + 3, 5)
        fr = frame_of([("raw", _bytes(rng, 64, 5)), cblock(lits, [(ll, ml, of)])])
        bits = 6 + 5 + 6 + LL_BITS[ll_code(ll)[0]] + ML_BITS[ml_code(ml)[0]] + of_code(of)[2]
        k += 1
        if bits % 8 in seen:
            continue
        seen.add(bits % 8)
        _case(C, "endmark_seq_bit_%d" % (bits % 8), ["endmark"], fr)
    seen = set()
    for n in range(40, 140):
        lits = _bytes(rng, n, 6)
        try:
            h = HufTable(huf_lengths({b: lits.count(b) for b in set(lits)}, 11))
        except CraftError:
            continue
        bits = sum(h.code[b][1] for b in lits) % 8
        if bits in seen:
            continue
        seen.add(bits)
        _case(C, "endmark_huf_bit_%d" % bits, ["endmark", "huf1"], frame_of([cblock(lits, lit_mode="huf1", weights="direct")]))
    # ---- repeat offsets
    for nb in (2, 3, 4):
        for ov in (1, 2, 3):
            for ll in (0, 7):
                for between in ("", "r", "l", "z"):
                    if between and nb != 3:
                        continue
                    blocks = []
                    produced = 0
                    rep = [1, 4, 8]
                    for b in range(nb):
                        size = 131072 if b < nb - 1 else 5000
                        first = [(ll, 9, ov)] if b == nb - 1 else []
                        if b == nb - 1 and between:
                            blocks.append(("raw", _bytes(rng, 50, 9)) if between == "r" else ("rle", 65, 50) if between == "l" else cblock(_bytes(rng, 50, 9)))
                            produced += 50
                        lits, seqs, rep = gen_block(rng, size, produced, rep, first, p_rep=0.4, lens=(3, 8, 40, 300, 3000))
                        blocks.append(cblock(lits, seqs, lit_mode="huf4"))
                        produced += size
                    _case(C, "rep_b%d_v%d_ll%d%s" % (nb, ov, ll, "_" + between if between else ""), ["repcode", "ll0_rep" if ll == 0 else "rep_start"] + (["rep_across_" + between] if between else []), frame_of(blocks, checksum=bool(ov & 1)))
    for between in ("", "r", "l", "z"):
        blocks = []
        lits, seqs, rep = gen_block(rng, 131072, 0, [1, 4, 8], p_rep=0.3, lens=(8, 40, 300, 3000))
        blocks.append(cblock(lits, seqs, lit_mode="huf4"))
        produced = 131072
        if between:
            blocks.append(("raw", _bytes(rng, 33, 9)) if between == "r" else ("rle", 66, 33) if between == "l" else cblock(_bytes(rng, 33, 9)))
            produced += 33
        if rep[0] < 7:
            raise AssertionError("the seed gives a short repeat offset here")
        lits, seqs, rep = gen_block(rng, 9000, produced, rep, [(0, 4, 3)] * 5, p_rep=0.4)
        blocks.append(cblock(lits, seqs))
        _case(C, "rep_five_ll0_v3" + ("_" + between if between else ""), ["repcode", "ll0_rep"], frame_of(blocks))
    # a repeat offset carried over three blocks unchanged
    b0 = cblock(_bytes(rng, 5000, 20), [(3000, 10, 1234 + 3)])
    carry = [cblock(_bytes(rng, 300, 20), [(100, 5, 1), (50, 6, 1)]), ("raw", _bytes(rng, 10, 3)), cblock(_bytes(rng, 40, 20)), cblock(_bytes(rng, 300, 20), [(0, 40, 2 - 1), (9, 4, 1)])]
    _case(C, "rep_carried_three_blocks", ["repcode", "ll0_rep"], frame_of([b0] + carry, checksum=True))
    _case(C, "rep_ll0_v3_at_rep1_of_1", ["repcode", "libzstd_answer"], frame_of([cblock(b"abcdefgh" * 4, [(8, 5, 1 + 3), (0, 6, 3), (2, 4, 1)])]))
    # ---- matches
    for ml in (3, 64, 70000):
        lits = _bytes(rng, 16 * 3 + 20, 50)
        seqs = [(3 if o > 1 else 20, ml, o + 3) for o in range(1, 17)]
        if ml == 70000:
            for o in (1, 2, 3, 5, 7, 16):
                _case(C, "match_off%d_ml70000" % o, ["match", "overlap"], frame_of([cblock(_bytes(rng, 30, 50), [(20, 70000, o + 3)]), cblock(_bytes(rng, 30, 50), [(5, 70000, 1)])], fcs_width=8))
        else:
            _case(C, "match_off1to16_ml%d" % ml, ["match", "overlap"], frame_of([cblock(lits, seqs)]))
    _case(C, "match_reaches_first_byte", ["match"], frame_of([cblock(_bytes(rng, 600, 50), [(500, 30, 500 + 3), (20, 8, 550 + 3)])]))
    _case(C, "match_starts_in_previous_block", ["match"], frame_of([("raw", _bytes(rng, 1000, 50)), cblock(_bytes(rng, 30, 50), [(0, 900, 1000 + 3), (10, 30, 1900 + 3)])]))
    _case(C, "match_one_match_per_block_131072_131070_131065", ["match", "ml52"], frame_of([("raw", _bytes(rng, 100, 50)), cblock(b"", [(0, 131072, 7 + 3)]), cblock(b"xy", [(2, 131074 - 4, 100 + 3)]), cblock(b"", [(0, 131072 - 7, 1)])]))
    _case(C, "match_length_131072_rle_tables", ["match", "ml52", "rle_mode"], frame_of([("raw", b"abc"), cblock(b"", [(0, 131072, 6)], modes=dict(ll="rle", of="rle", ml="rle"))]))
    _case(C, "literal_length_131069_code_35", ["match", "ll35"], frame_of([cblock(_bytes(rng, 131069, 3, 48), [(131069, 3, 9)], lit_mode="huf4")]))
    _case(C, "ll35_ml52_of17_rle", ["match", "ll35", "ml52", "rle_mode"], frame_of([("raw", _bytes(rng, 131072, 2, 48)), cblock(_bytes(rng, 65536, 2, 48), [(65536, 65536, (1 << 17) + 1)], lit_mode="huf4", modes=dict(ll="rle", of="rle", ml="rle"))], fcs_width=8))
    # The largest lengths the codes express — match length 131,074 (code 52, all 16 extra bits set) and literal length 131,071 (code 35,
    # all extra bits set) — cannot occur in a valid frame: either makes its block regenerate more than 128 KiB. libzstd's one-shot
    # decoder does not enforce that limit on what a block regenerates, so these decode; its answer is the expectation (error=None).
    _case(C, "overlimit_match_length_131074_last_block", ["match", "ml52", "over_limit", "libzstd_answer"],
          frame_of([("raw", _bytes(rng, 140, 50)), cblock(b"", [(0, 131074, 7 + 3)])], over_limit=True), error=None)
    _case(C, "overlimit_match_length_131074_rle_tables_middle_block", ["match", "ml52", "rle_mode", "over_limit", "libzstd_answer"],
          frame_of([("raw", b"abc"), cblock(b"", [(0, 131074, 6)], modes=dict(ll="rle", of="rle", ml="rle")), cblock(_bytes(rng, 300, 9), [(100, 30, 1), (0, 9, 2)])], over_limit=True, checksum=True), error=None)
    _case(C, "overlimit_literal_length_131071", ["match", "ll35", "over_limit", "libzstd_answer"],
          frame_of([cblock(_bytes(rng, 131071, 3, 48), [(131071, 3, 9)], lit_mode="huf4"), cblock(_bytes(rng, 50, 9), [(10, 30, 2)])], over_limit=True), error=None)
    _case(C, "offset_one_beyond_output", ["match", "error"], frame_of([cblock(_bytes(rng, 100, 50), [(50, 10, 51 + 3)])], invalid_offset=True), error=True)
    # ---- sequence tables
    def tb(n, produced, rep, **kw):
        lits, seqs, rep2 = gen_block(rng, n, produced, rep, alpha=12, max_seq=kw.pop("max_seq", 300))
        return cblock(lits, seqs, **kw), rep2
    for m in ("predef", "rle", "fse", "repeat"):
        if m == "rle":
            blocks = [("raw", _bytes(rng, 500, 20)), cblock(_bytes(rng, 200, 9), [(4, 7, 100 + 3)] * 30, modes=dict(ll=m, of=m, ml=m))]
        elif m == "repeat":
            b1, rep = tb(20000, 0, [1, 4, 8], modes=dict(ll="fse", of="fse", ml="fse"), extra=dict(ll=range(36), of=range(18), ml=range(53)), logs=dict(ll=9, of=8, ml=9))
            b2, rep = tb(20000, 20000, rep, modes=dict(ll=m, of=m, ml=m))
            blocks = [b1, b2]
        else:
            blocks = [tb(20000, 0, [1, 4, 8], modes=dict(ll=m, of=m, ml=m))[0]]
        _case(C, "tables_all_" + m, ["tables", m + "_mode"], frame_of(blocks))
    k = 0
    for ll in ("predef", "rle", "fse"):
        for of in ("predef", "rle", "fse"):
            for ml in ("predef", "rle", "fse"):
                if len({ll, of, ml}) == 1:
                    continue
                seqs = []
                for i in range(60):
                    seqs.append((4 if ll == "rle" else int(rng.randint(0, 30)), 7 if ml == "rle" else int(rng.randint(3, 90)), (100 if of == "rle" else int(rng.randint(1, 400))) + 3))
                fr = frame_of([("raw", _bytes(rng, 500, 20)), cblock(_bytes(rng, 2000, 9), seqs, modes=dict(ll=ll, of=of, ml=ml)),
                               ("rle", 1, 20) if k % 3 == 0 else ("raw", b"between") if k % 3 == 1 else cblock(b"only literals"),
                               cblock(_bytes(rng, 2000, 9), seqs, modes=dict(ll="repeat", of="repeat", ml="repeat"))])
                _case(C, "tables_%s_%s_%s_then_repeat" % (ll, of, ml), ["tables", "repeat_mode", "repeat_across_" + "lrz"[k % 3]], fr)
                k += 1
    for name, logs in (("min", dict(ll=5, of=5, ml=5)), ("max", dict(ll=9, of=8, ml=9))):
        seqs = [(int(rng.randint(0, 16)), int(rng.randint(3, 20)), int(rng.randint(1, 60)) + 3) for i in range(500)]
        _case(C, "tables_fse_log_" + name, ["tables", "fse_mode"], frame_of([("raw", _bytes(rng, 100, 20)), cblock(_bytes(rng, 9000, 9), seqs, modes=dict(ll="fse", of="fse", ml="fse"), logs=logs)]))
    # "less than one" symbols, zero runs of 3, 24 and 27+, a description ending on the table's maximum symbol
    seqs = [(0, 3, 4)] * 30 + [(3, 3 + 3, 4)] * 20 + [(3 + 24 + 1, 3 + 3 + 24 + 1, 5)] * 9 + [(0, 3 + 34 + 27 + 1 - 3, 4)] * 3
    fr = frame_of([("raw", _bytes(rng, 100, 20)), cblock(_bytes(rng, 600, 9), seqs, modes=dict(ll="fse", of="fse", ml="fse"), extra=dict(ll=[35], ml=[52], of=[28, 31]), logs=dict(ll=6, of=6, ml=7))])
    _case(C, "tables_zero_runs_and_low_symbols", ["tables", "fse_mode", "lowprob"], fr)
    # ---- literals
    for n, sf in ((5, 0), (5, 1), (5, 3), (31, 0), (32, 1), (4095, 1), (4096, 3), (40, 3)):
        for mode in ("raw", "rle"):
            lits = _bytes(rng, n, 30) if mode == "raw" else b"\x07" * n
            _case(C, "lits_%s_%d_format%d" % (mode, n, sf), ["literals", "lit_" + mode], frame_of([("raw", b"0123456789"), cblock(lits, [(2, 4, 3 + 3)], lit_mode=mode, size_format=sf)]))
    for n in (6, 100, 1023):
        _case(C, "lits_huf1_%d" % n, ["literals", "huf1"], frame_of([cblock(_bytes(rng, n, 6 if n < 50 else 40), lit_mode="huf1", weights="direct" if n < 50 else "fse")]))
    for n, sf in ((700, 1), (700, 2), (700, 3), (9000, 2), (9000, 3), (40000, 3)):
        _case(C, "lits_huf4_%d_format%d" % (n, sf), ["literals", "huf4"], frame_of([cblock(_bytes(rng, n, 50), [(10, 5, 9 + 3)], lit_mode="huf4", size_format=sf)]))
    for n in (6, 7, 8, 9, 10, 11):
        _case(C, "lits_huf4_regen_%d" % n, ["literals", "huf4", "libzstd_answer"], frame_of([cblock((b"abcabcabcab" * 2)[:n], lit_mode="huf4", weights="direct")]), error=None)
    for nw in (2, 3, 127, 128):
        lits = bytes(list(range(nw + 1)) * 3) + _bytes(rng, 2000, min(nw + 1, 7))
        _case(C, "lits_direct_%d_weights" % nw, ["literals", "direct_weights"], frame_of([cblock(lits, lit_mode="huf4", weights="direct")]))
    for nw in (129, 255):
        lits = bytes(list(range(nw + 1)) * 3) + _bytes(rng, 3000, 9)
        _case(C, "lits_fse_%d_weights" % nw, ["literals", "fse_weights"], frame_of([cblock(lits, lit_mode="huf4", weights="fse")]))
    _case(C, "lits_two_symbols_one_bit", ["literals", "huf1"], frame_of([cblock(_bytes(rng, 500, 2, 65), lit_mode="huf1", weights="direct", max_bits=1)]))
    deep = b"".join(bytes([i]) * (1 << i) for i in range(12))
    _case(C, "lits_tree_depth_11", ["literals", "huf4"], frame_of([cblock(deep, lit_mode="huf4", max_bits=11)]))
    # treeless literals behind a new tree, across other literal sections and other blocks; X1 and X2 tables inherited
    for first, then in (("huf4", "treeless1"), ("huf1", "treeless4"), ("huf4", "treeless4"), ("huf1", "treeless1")):
        for wide in (False, True):
            a = 25 if wide else 3                            # (at these sizes libzstd picks its double-symbol decoder for the 4-stream blocks of both)
            n1 = 900 if first == "huf1" else 20000
            blocks = [cblock(bytes(range(a)) + _bytes(rng, n1, a), [(5, 5, 4)], lit_mode=first, weights="fse" if wide else "direct"),
                      cblock(_bytes(rng, 40, 200), [(5, 5, 4)], lit_mode="raw"), cblock(b"\x01" * 50, [(5, 5, 4)], lit_mode="rle"),
                      ("raw", b"raw block"), ("rle", 3, 30),
                      cblock(_bytes(rng, 800, a), [(5, 5, 4)], lit_mode=then), cblock(_bytes(rng, 1000, a), lit_mode="treeless4")]
            _case(C, "lits_%s_then_%s_%s" % (first, then, "wide" if wide else "narrow"), ["literals", then, "treeless_across"], frame_of(blocks))
    # ---- frame headers
    small = [cblock(_bytes(rng, 300, 20), [(100, 50, 60 + 3), (0, 9, 2)])]
    tiny = [cblock(_bytes(rng, 100, 20), [(70, 50, 60 + 3), (0, 9, 2)])]
    for fw in (0, 1, 2, 4, 8):
        for ss in (False, True):
            if (fw == 1 and not ss) or (fw == 0 and ss):
                continue
            kw = dict(single_segment=True) if ss else dict(window=(0, 0))
            _case(C, "header_fcs%d_%s" % (fw, "single" if ss else "window"), ["header", "fcs%d" % fw], frame_of(tiny if fw == 1 else small, fcs_width=fw, checksum=bool(fw & 2), **kw))
    for e in (0, 7, 10):
        for m in (0, 7):
            _case(C, "header_window_e%d_m%d" % (e, m), ["header", "fcs0"], frame_of(small, window=(e, m), fcs_width=0))
    for dw in (1, 2, 4):
        _case(C, "header_dict_field_%d_zero" % dw, ["header", "dict_field"], frame_of(small, dict_width=dw, checksum=True))
    _case(C, "header_reserved_bit", ["header", "error"], frame_of(small, reserved=True), error=True)
    _case(C, "header_dictionary_id", ["header", "error"], frame_of(small, dict_width=2, dict_value=77), error=True)
    for wname, win in (("32MiB", (15, 0)), ("2GiB", (21, 0))):
        for share in (True, False):
            lits, seqs, _ = gen_block(rng, 50000, 0, [1, 4, 8], max_seq=2000, alpha=30)
            extra = dict(of=[23, 24, 26]) if share else {}
            fr = frame_of([cblock(lits, seqs, lit_mode="huf4", modes=dict(ll="predef", of="fse", ml="predef"), extra=extra, logs=dict(of=6))], window=win, fcs_width=0 if share else 4, checksum=share)
            _case(C, "header_window_%s_%s" % (wname, "long_offsets" if share else "short_offsets"), ["header", "bigwindow"] + (["long_mode"] if share else []), fr)
    return C


# ================================================================================================ randomised descriptions
RANDOM_TAGS = (["lit_raw", "lit_rle", "lit_huf1", "lit_huf4", "lit_treeless1", "lit_treeless4", "direct_weights", "fse_weights", "x1", "x2"]
               + ["%s_%s" % (k, m) for k in ("ll", "of", "ml") for m in ("predef", "rle", "fse", "repeat")]
               + ["repeat_across_raw", "repeat_across_rle", "repeat_across_zero_seq", "ll0_rep_block_start", "short_nonlast", "many_blocks",
                  "fcs0", "fcs1", "fcs2", "fcs4", "fcs8", "count3", "long_mode"])
FRAME_SIZE = 262144                                          # of the archives the randomised frames go into: two blocks per frame


def _abs_sequences(content, level):
    """the frame's sequences as (ll, ml, offset) with the offsets resolved, and the literals behind the last one"""
    import oracle_lib as O
    rep = [1, 4, 8]
    out = []
    pending = 0
    for ll, ml, ov in O.sequences(content, level):
        if ml == 0:
            pending += ll
            continue
        off, rep = rep_step(rep, ll, ov)
        out.append((pending + ll, ml, off))
        pending = 0
    return out, pending


def _proto_from_content(rng, content):
    """proto blocks ("seq", lits, [(ll, ml, offset)]) cut at random places of a real encoder's sequences"""
    seqs, tail = _abs_sequences(content, int(_pick(rng, [1, 3, 5])))
    n = len(content)
    style = rng.rand()

    def limit():
        if style < 0.3:
            return BLOCK_MAX
        if style < 0.6:
            return int(_pick(rng, [BLOCK_MAX, BLOCK_MAX, int(rng.randint(1, BLOCK_MAX + 1)), int(rng.randint(1, 3000))]))
        return max(1, min(BLOCK_MAX, int(n / rng.randint(1, 31) * (0.5 + rng.rand()))))
    blocks = []
    lits = bytearray()
    cur = []
    size = 0
    lim = limit()
    pos = 0

    def close():
        nonlocal lits, cur, size, lim
        if size:
            blocks.append(("seq", bytes(lits), cur))
        lits, cur, size, lim = bytearray(), [], 0, limit()
    for ll, ml, off in seqs + [(tail, 0, 0)]:
        while True:
            if size + ll + ml <= lim:
                lits += content[pos:pos + ll]
                pos += ll + ml
                if ml:
                    cur.append((ll, ml, off))
                size += ll + ml
                break
            take = min(ll, lim - size)
            lits += content[pos:pos + take]
            pos += take
            ll -= take
            size += take
            close()
            if ll + ml > BLOCK_MAX:
                lim = BLOCK_MAX
            elif ll + ml > lim:
                lim = ll + ml
    close()
    return blocks


def _proto_synthetic(rng, n):
    """proto blocks with sequences of the generator's own: many repeat codes, blocks without sequences, raw and RLE blocks between"""
    blocks = []
    produced = 0
    rep = [1, 4, 8]
    nb = int(rng.randint(1, 31))
    alpha = int(_pick(rng, [2, 4, 16, 64, 200, 256]))
    tiny = rng.rand() < 0.25
    while produced < n:
        left = n - produced
        r = rng.rand()
        size = min(left, BLOCK_MAX, int(_pick(rng, [BLOCK_MAX, max(1, n // nb), int(rng.randint(1, 4000)), int(rng.randint(1, BLOCK_MAX + 1))])))
        if tiny and left >= 100000 and produced:
            size = min(left, BLOCK_MAX)
        if r < 0.08 and produced:
            size = min(size, 3000)
            blocks.append(("raw", _bytes(rng, size, alpha)))
        elif r < 0.16 and produced:
            blocks.append(("rle", int(rng.randint(0, 256)), size))
        elif r < 0.24 and produced:
            size = min(size, 3000)
            blocks.append(("seq", _bytes(rng, size, alpha), []))
        elif tiny and size > 100000 and produced:
            # more sequences than the two-byte count holds: three-byte matches
            k = 0x7F00 + int(rng.randint(0, 40))
            lits, seqs, rep = gen_block(rng, size, produced, rep, alpha=4, max_seq=k, lens=(3,), ll_max=0, p_rep=0.3, max_off=16)
            blocks.append(("wire", lits, seqs))
            tiny = False
        else:
            first = []
            if produced > 20 and rng.rand() < 0.5 and size > 40:
                first = [(0, int(rng.randint(3, 12)), int(rng.randint(1, 4)))] * int(_pick(rng, [1, 1, 2, 5]))
                if rep_step(rep, 0, first[0][2])[0] > produced or (first[0][2] == 3 and rep[0] <= len(first)):
                    first = []
            lits, seqs, rep = gen_block(rng, size, produced, rep, first, alpha=alpha, max_seq=int(_pick(rng, [3, 50, 400, 3000])), p_rep=0.4,
                                        lens=(3, 4, 5, 8, 12, 40, 300, 3000, 20000), max_off=int(_pick(rng, [16, 5000, 1 << 18])))
            blocks.append(("wire", lits, seqs))
        produced += size
    return blocks


def random_description(rng):
    """(frame description, set of feature tags that do not depend on the written bytes)"""
    import corpus
    tags = set()
    r = rng.rand()
    n = FRAME_SIZE if r < 0.4 else int(rng.randint(1, 256)) if r < 0.48 else int(rng.randint(256, 65792)) if r < 0.56 else int(rng.randint(1, 300001))
    if rng.rand() < 0.5:
        content = (corpus.random_lz_input if rng.rand() < 0.5 else corpus.random_lz_input_far)(rng, n)
        proto = _proto_from_content(rng, content)
    else:
        content = None
        proto = _proto_synthetic(rng, n)
    # ---- blocks: every free choice among what is valid at that point
    blocks = []
    rep = [1, 4, 8]
    tree = None                                              # symbols of the Huffman tree in force
    tab = {"ll": None, "of": None, "ml": None}               # codes of the tables in force
    since = {"ll": set(), "of": set(), "ml": set()}          # block kinds seen since the table was last used
    big = rng.rand() < 0.12
    max_off = 1
    ncomp = 0
    for pb in proto:
        if pb[0] in ("raw", "rle"):
            blocks.append(pb)
            for k in since:
                since[k].add(pb[0])
            continue
        lits = pb[1]
        if pb[0] == "seq":
            seqs = []
            for ll, ml, off in pb[2]:
                ov = to_wire(rng, rep, ll, off)
                _, rep = rep_step(rep, ll, ov)
                seqs.append((ll, ml, ov))
        else:
            seqs = pb[2]
        if not seqs and rng.rand() < 0.5 and len(lits):
            if lits == lits[:1] * len(lits) and rng.rand() < 0.7:
                blocks.append(("rle", lits[0], len(lits)))
                kind = "rle"
            else:
                blocks.append(("raw", lits))
                kind = "raw"
            for k in since:
                since[k].add(kind)
            continue
        c = dict(lits=lits, seqs=seqs)
        # literals
        nl = len(lits)
        syms = set(lits)
        opts = ["raw"]
        if nl and len(syms) == 1:
            opts += ["rle"] * 4
        if len(syms) >= 2 and nl >= 6:
            opts += ["huf4"] * 2
            if nl <= 900:
                opts += ["huf1"] * 2
        if tree is not None and syms <= tree and nl >= 6:
            opts += ["treeless4"] * 3
            if nl <= 900:
                opts += ["treeless1"] * 3
        lm = opts[int(rng.randint(0, len(opts)))]
        c["lit_mode"] = lm
        tags.add("lit_" + lm)
        if lm in ("raw", "rle"):
            need = 0 if nl < 32 else 1 if nl < 4096 else 3
            c["size_format"] = int(_pick(rng, [f for f in (0, 1, 3) if f >= need]))
        else:
            if lm in ("huf1", "huf4"):
                c["max_bits"] = int(_pick(rng, [11, 11, 10, 8]))
                try:                                         # which forms can hold this tree's weights
                    ln = huf_lengths({b: lits.count(b) for b in syms}, c["max_bits"])
                    ws = {ln[b] for b in syms if b != max(syms)} | ({0} if len(syms) < max(syms) + 1 else set())
                    forms = (["direct"] if max(syms) <= 128 else []) + (["fse"] if len(ws) > 1 and max(syms) >= 2 else [])
                except CraftError:
                    forms = []
                if not forms:
                    c["lit_mode"] = "raw"
                    c["size_format"] = 0 if nl < 32 else 1 if nl < 4096 else 3
                    tags.discard("lit_" + lm)
                    tags.add("lit_raw")
                    forms = [None]
                    lm = "raw"
                w = forms[int(rng.randint(0, len(forms)))]
                if w is None:
                    pass
                else:
                    c["weights"] = w
                    tags.add(w + "_weights")
                    tree = syms
            if lm.endswith("4"):
                need = 1 if nl < 800 else 2 if nl < 16000 else 3
                c["size_format"] = int(_pick(rng, [f for f in (1, 2, 3) if f >= need]))
        # sequence tables
        if seqs:
            ncomp += 1
            if ncomp > 1 and seqs[0][0] == 0 and seqs[0][2] <= 3:
                tags.add("ll0_rep_block_start")
            codes = {"ll": {ll_code(s[0])[0] for s in seqs}, "ml": {ml_code(s[1])[0] for s in seqs}, "of": {of_code(s[2])[0] for s in seqs}}
            max_off = max([max_off] + [s[2] - 3 for s in seqs if s[2] > 3])
            modes, logs, extra = {}, {}, {}
            for k in ("ll", "of", "ml"):
                opts = []
                if k != "of" or max(codes[k]) <= 28:
                    opts += ["predef"] * 2
                if len(codes[k]) == 1:
                    opts += ["rle"] * 6
                if tab[k] is not None and codes[k] <= tab[k]:
                    opts += ["repeat"] * 3
                free = [s for s in range(MAX_SYM[k] + 1) if s not in codes[k]]
                ex = [int(x) for x in rng.choice(free, size=int(rng.randint(1, 4)), replace=False)] if rng.rand() < 0.3 else []
                if len(codes[k]) + len(ex) >= 2:
                    opts += ["fse"] * 3
                if big and k == "of" and len(seqs) > 4 and "predef" in opts:
                    opts = ["predef"]
                m = opts[int(rng.randint(0, len(opts)))]
                modes[k] = m
                tags.add("%s_%s" % (k, m))
                if m == "fse":
                    lo = max(5, (len(codes[k]) + len(ex) - 1).bit_length())
                    logs[k] = int(rng.randint(lo, MAX_LOG[k] + 1))
                    extra[k] = ex
                    tab[k] = codes[k] | set(ex)
                elif m == "rle":
                    tab[k] = set(codes[k])
                elif m == "predef":
                    tab[k] = set(range(MAX_SYM[k] + 1 if k != "of" else 29))
                    if big and k == "of" and len(seqs) > 4:
                        tags.add("long_mode")
                else:
                    for kind in since[k]:
                        tags.add("repeat_across_" + kind)
                since[k] = set()
            c.update(modes=modes, logs=logs, extra=extra)
            ns = len(seqs)
            c["count_width"] = 3 if ns >= 0x7F00 else int(_pick(rng, [w for w in (1, 2) if w >= (1 if ns < 128 else 2)]))
            if ns >= 0x7F00:
                tags.add("count3")
        else:
            for k in since:
                since[k].add("zero_seq")
        blocks.append(("compressed", c))
    # ---- header
    fr = dict(blocks=blocks)
    sizes = block_sizes(fr)
    total = sum(sizes)
    if any(s != BLOCK_MAX and blocks[i][0] == "compressed" for i, s in enumerate(sizes[:-1])):
        tags.add("short_nonlast")
    if sum(1 for b in blocks if b[0] == "compressed") > (FRAME_SIZE + BLOCK_MAX - 1) // BLOCK_MAX:
        tags.add("many_blocks")
    ss = rng.rand() < (0.8 if total <= 255 else 0.4) and not big
    widths = [w for w in (0, 1, 2, 4, 8) if not (w == 1 and (not ss or total > 255)) and not (w == 0 and ss) and not (w == 2 and not 256 <= total <= 65791)]
    fr["fcs_width"] = 1 if 1 in widths and rng.rand() < 0.6 else int(_pick(rng, widths))
    tags.add("fcs%d" % fr["fcs_width"])
    if ss:
        fr["single_segment"] = True
    else:
        need = max(max(sizes), max_off, 1)
        e = max(0, (need - 1).bit_length() - 10)
        fr["window"] = (int(rng.randint(15, 22)), int(rng.randint(0, 8))) if big else (min(31, e + int(rng.randint(0, 3))), int(rng.randint(0, 8)))
        if big and fr["window"][0] == 21:
            fr["window"] = (21, 0)
    fr["checksum"] = bool(rng.rand() < 0.5)
    fr["dict_width"] = int(_pick(rng, [0, 0, 0, 1, 2, 4]))
    if content is not None and plaintext(fr) != content:
        raise AssertionError("the cut sequences no longer give the content")
    return fr, tags


RANDOM_SEEDS = (7000, 7001, 7002, 7003, 7004, 7005)
_drawn = {}


def random_frames(seed, count=40):
    """[(description, tags, frame bytes)] of `count` written frames, and how many drawn descriptions the writer refused"""
    if (seed, count) not in _drawn:
        _drawn[(seed, count)] = _random_frames(seed, count)
    return _drawn[(seed, count)]


def _random_frames(seed, count):
    import oracle_lib as O
    rng = _rng(seed)
    out = []
    refused = 0
    while len(out) < count:
        fr, tags = random_description(rng)
        info = []
        try:
            data = write_frame(fr, info)
        except CraftError:
            refused += 1
            continue
        k = 0
        for b in fr["blocks"]:
            if b[0] == "compressed":
                if b[1].get("lit_mode") == "huf4":       # (one stream with a new tree always takes the single-symbol decoder: not counted)
                    tags.add("x2" if O.lib().zo_huf_select_decoder(info[k][0], info[k][1]) else "x1")
                k += 1
        out.append((fr, tags, data))
    return out, refused


def dump(path):
    """every randomised frame (the fixed seeds) and every directed frame as records for the stand-alone sanitizer check of the restated
    decoder (oracle/zo_craft_check.c, `make -C oracle craft-check`); the invalid frames carry the status recorded from libzstd"""
    import json
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crafted_frames.json")
    status = {e["name"]: e["zl_status"] for e in json.load(open(golden))}
    recs = [(fr, data, 0) for seed in RANDOM_SEEDS for fr, _, data in random_frames(seed)[0]]
    recs += [(c["frame"], write_frame(c["frame"]), status[c["name"]]) for c in directed_cases()]
    with open(path, "wb") as f:
        for fr, data, code in recs:
            plain = plaintext(fr, check=False) if not code else bytes(4112)
            f.write(struct.pack("<IIIQ", len(data), len(plain), code, xxh64(plain)) + data)
    return len(recs)


if __name__ == "__main__":
    import sys
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        print("frames written:", dump(sys.argv[2]))
    else:
        sys.exit("usage: frame_craft.py --dump FILE")
