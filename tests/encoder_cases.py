"""Directed inputs for the ENCODER: one seeded input per format decision of the entropy stage (zra_amd/csrc/zra_encode_ent.hip; zstd
1.4.9's ZSTD_compressLiterals / HUF_compress / ZSTD_compressSequences / ZSTD_selectEncodingType), and a reader of zstd frames that
says which decisions an archive shows. The decoder's counterpart is frame_craft.py.

describe_frame(frame) walks the blocks of a frame without decoding any entropy: block type and size, the literals section's mode, size
format, stream count and sizes, whether a Huffman header is FSE-compressed, the sequence count and the width of its field, the three
table modes. features(frame) turns that into a set of tags; directed_cases() names for every input the tags the ORACLE's archive of it
must show, so an input that stops reaching its decision fails on the CPU (test_encoder_cases.py) before it stops testing the GPU.

Tags:
  blk:raw | blk:rle | blk:comp (+ ":first" | ":later")     block types;   blk:comp_after_raw_first
  rawblk:n=N                                                a raw block of N bytes
  tailblk:N                                                 a last block of N bytes (1..7) behind a full block
  lit:MODE:sfF (+ ":later")  MODE raw|rle|comp|treeless     literals section mode and size format
  litn:MODE:N                                               its regenerated size
  lit:streams1 | lit:streams4
  huf:fse | huf:direct                                      the tree description of a "comp" section
  nbseq=N, nbseq:w1|w2|w3                                   sequence count and the bytes of its field
  ll|of|ml:predef|rle|fse|repeat (+ ":first" | ":later")    table modes;   of:rle:nbseq>2;  predef:nbseq<=2
"""
import hashlib

import numpy as np

MAGIC = 0xFD2FB528


class FrameError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------ the frame reader
def archive_frames(arc):
    """the zstd frames of a ZRA archive (38-byte fixed header, meta, 5-byte seek entries, body)"""
    hsize = int.from_bytes(arc[4:8], "little") + 8
    ts = int.from_bytes(arc[26:30], "little")
    ms = int.from_bytes(arc[34:38], "little")
    ent = [int.from_bytes(arc[38 + ms + 5 * i:38 + ms + 5 * i + 5], "little") for i in range(ts)]
    return [arc[hsize + ent[i]:hsize + ent[i + 1]] for i in range(ts - 1)]


def describe_frame(frame):
    """[{type, size, last, ...}] per block of a zstd frame as this project writes them (no dictionary id, no content size field beyond
    what the descriptor says)"""
    if int.from_bytes(frame[:4], "little") != MAGIC:
        raise FrameError("magic")
    fhd = frame[4]
    single, cs_flag, did = (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    fcs = fhd >> 6
    p = 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0), 2, 4, 8)[fcs]
    out = []
    while True:
        h = int.from_bytes(frame[p:p + 3], "little")
        p += 3
        last, typ, size = h & 1, (h >> 1) & 3, h >> 3
        b = {"type": ("raw", "rle", "comp")[typ], "size": size, "last": bool(last)}
        if typ == 0:
            p += size
        elif typ == 1:
            p += 1
        elif typ == 2:
            _describe_block(frame[p:p + size], b)
            p += size
        else:
            raise FrameError("reserved block type")
        out.append(b)
        if last:
            break
    if p + (4 if cs_flag else 0) != len(frame):
        raise FrameError("frame length: %d + checksum != %d" % (p, len(frame)))
    return out


def _describe_block(c, b):
    b0 = c[0]
    mode, sf = b0 & 3, (b0 >> 2) & 3
    b["lit_mode"] = ("raw", "rle", "comp", "treeless")[mode]
    b["lit_sf"] = sf
    if mode < 2:
        hl = (1, 2, 1, 3)[sf]
        sf = b["lit_sf"] = sf if hl > 1 else 0               # (a one-byte header has a one-bit size format)
        regen = int.from_bytes(c[:hl], "little") >> (3 if hl == 1 else 4)
        comp = regen if mode == 0 else 1
        b["lit_streams"] = 0
    else:
        hl, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
        v = int.from_bytes(c[:hl], "little") >> 4
        regen, comp = v & ((1 << bits) - 1), v >> bits
        b["lit_streams"] = 1 if sf == 0 else 4
        if mode == 2:
            b["huf_fse"] = c[hl] < 128
    b["lit_regen"], b["lit_comp"] = regen, comp
    p = hl + comp
    if p >= len(c) + 1:
        raise FrameError("literals section beyond the block")
    n0 = c[p]
    if n0 == 0:
        nb, w = 0, 1
    elif n0 < 128:
        nb, w = n0, 1
    elif n0 < 255:
        nb, w = ((n0 - 128) << 8) + c[p + 1], 2
    else:
        nb, w = c[p + 1] + (c[p + 2] << 8) + 0x7F00, 3
    b["nb_seq"], b["nb_seq_width"] = nb, w
    if nb:
        m = c[p + w]
        names = ("predef", "rle", "fse", "repeat")
        b["ll_mode"], b["of_mode"], b["ml_mode"] = names[m >> 6], names[(m >> 4) & 3], names[(m >> 2) & 3]


def features(frame):
    """the tags of one frame (module docstring)"""
    t = set()
    blocks = describe_frame(frame)
    for i, b in enumerate(blocks):
        pos = "first" if i == 0 else "later"
        t.add("blk:" + b["type"])
        t.add("blk:%s:%s" % (b["type"], pos))
        if b["type"] == "raw":
            t.add("rawblk:n=%d" % b["size"])
        if b["type"] == "comp" and i and blocks[0]["type"] == "raw" and all(x["type"] != "comp" for x in blocks[:i]):
            t.add("blk:comp_after_raw_first")
        if b["last"] and i and 1 <= (b["size"] if b["type"] != "comp" else 99) <= 7:
            t.add("tailblk:%d" % b["size"])
        if b["type"] != "comp":
            continue
        m = b["lit_mode"]
        t.add("lit:%s:sf%d" % (m, b["lit_sf"]))
        if i:
            t.add("lit:%s:sf%d:later" % (m, b["lit_sf"]))
        t.add("litn:%s:%d" % (m, b["lit_regen"]))
        if b["lit_streams"]:
            t.add("lit:streams%d" % b["lit_streams"])
        if "huf_fse" in b:
            t.add("huf:fse" if b["huf_fse"] else "huf:direct")
        t.add("nbseq=%d" % b["nb_seq"])
        t.add("nbseq:w%d" % b["nb_seq_width"])
        if b["nb_seq"]:
            for k in ("ll", "of", "ml"):
                t.add("%s:%s" % (k, b[k + "_mode"]))
                t.add("%s:%s:%s" % (k, b[k + "_mode"], pos))
                if b[k + "_mode"] == "predef" and b["nb_seq"] <= 2:
                    t.add("predef:nbseq<=2")
            if b["of_mode"] == "rle" and b["nb_seq"] > 2:
                t.add("of:rle:nbseq>2")
    return t


def archive_features(arc):
    t = set()
    for f in archive_frames(arc):
        t |= features(f)
    return t


# ------------------------------------------------------------------------------------------------ sources
def _rs(*key):
    return np.random.RandomState(int.from_bytes(hashlib.sha256(repr(key).encode()).digest()[:4], "little"))


def skewed(n, nsym, seed=0, flip=False):
    """i.i.d. bytes, P(k) proportional to 1 / (1 + k) over nsym symbols (flip: to 1 / (nsym - k))"""
    p = 1.0 / (1.0 + np.arange(nsym))
    return _rs("skew", nsym, seed).choice(nsym, size=n, p=(p[::-1] if flip else p) / p.sum()).astype(np.uint8).tobytes()


def uniform(n, seed=0, alpha=256):
    return _rs("uni", seed, alpha).randint(0, alpha, size=n).astype(np.uint8).tobytes()


def words(nwords, wlen, count, seed=0):
    """`count` words drawn from a dictionary of nwords random words of wlen bytes, back to back; (dictionary bytes, text)"""
    r = _rs("words", nwords, wlen, seed)
    d = r.randint(0, 256, size=(nwords, wlen)).astype(np.uint8)
    return d.tobytes(), d[r.randint(0, nwords, size=count)].tobytes()


def dense_words(n, nwords, seed=0):
    """n bytes of 3-byte words from nwords words: more sequences than a quarter of the bytes wherever minMatch is 3"""
    return words(nwords, 3, (n + 2) // 3, seed)[1][:n]


def fibonacci(seed=0, times=1):
    """Fibonacci counts (times `times`) over 20 symbols, shuffled: 17,710 bytes whose unlimited Huffman tree is 19 deep"""
    f = [1, 1]
    while len(f) < 20:
        f.append(f[-1] + f[-2])
    a = np.repeat(np.arange(20, dtype=np.uint8), np.array(f) * times)
    _rs("fib", seed).shuffle(a)
    return a.tobytes()


def seq_count(k, gap, seed=0, wlen=8):
    """k dictionary words between stretches of unique random filler: the first occurrence of a word is literals, so a one-word dictionary
    placed k + 1 times gives k matches"""
    r = _rs("seqcount", k, gap, seed)
    w = r.randint(0, 256, size=wlen).astype(np.uint8).tobytes()
    out = bytearray()
    for i in range(k + 1):
        out += r.randint(0, 256, size=gap).astype(np.uint8).tobytes() + w
    return bytes(out)


def raw_literals(n, seed=0):
    """n literals that do not compress, in a block that does: an 8-byte word, then random bytes in stretches of at most 200 with the word
    between them (behind 256 literals the fast finders start to skip positions, and a match then starts some bytes late), and the word
    six times more: the last match runs to the end of the block"""
    r = _rs("rawlits", n, seed)
    w = r.randint(0, 256, size=8).astype(np.uint8).tobytes()
    out, left = bytearray(r.randint(0, 256, size=8).astype(np.uint8).tobytes() + w), n - 16
    while left > 0:
        k = min(left, 200)
        out += r.randint(0, 256, size=k).astype(np.uint8).tobytes() + w
        left -= k
    return bytes(out + w * 6)


def ll_rle_frame(seed=0):
    """block 1: a dictionary of 2048 six-byte words + random filler to 128 KiB (stored raw); block 2: 3,000 of the words back to back"""
    d, text = words(2048, 6, 3000, seed)
    return d + uniform(131072 - len(d), ("fill", seed)) + text


# ------------------------------------------------------------------------------------------------ the directed cases
# Random filler now and then holds a match of its own, extends a word by a byte or loses one to a hash collision: the seed of a
# construction is the first one at which the oracle's archive shows exactly the case's tags (found by tools/bringup/encoder_case_seeds.py;
# test_encoder_cases.py holds every case to its tags, so a seed that stops working fails there).
SEEDS = {"lit-comp-255": 1, "of-rle": 20, "ml-rle-first": 13, "prefer-l3-1024": 30, "prefer-l3-1025": 7}
_seed_override = {}


def _seed(name):
    return _seed_override.get(name, SEEDS.get(name, 0))


def _c(out, name, data, level, fs, must_hit, checksum=True):
    out.append((name, data, level, fs, checksum, set(must_hit)))


def directed_cases():
    """[(name, data, level, frame_size, checksum, must_hit)]"""
    out = []
    # compressed literal counts on the edges of the size formats, zero sequences (63: ZSTD_compressLiterals' floor, the block is raw)
    for n, nsym, sf, st in ((63, 40, None, 0), (64, 40, 0, 1), (255, 40, 0, 1), (256, 40, 1, 4), (1023, 40, 1, 4), (1024, 40, 2, 4),
                            (16383, 200, 2, 4), (16384, 200, 3, 4)):
        hit = {"rawblk:n=63"} if sf is None else {"litn:comp:%d" % n, "lit:comp:sf%d" % sf, "lit:streams%d" % st, "nbseq=0"}
        _c(out, "lit-comp-%d" % n, skewed(n, nsym, (n, _seed("lit-comp-%d" % n))), 1, n, hit, checksum=bool(n & 1))
    # raw blocks, and raw literals inside a compressed block (a few dictionary words behind n random bytes), at the header widths' edges
    for n, sf in ((31, 0), (32, 1), (4095, 1), (4096, 3)):
        _c(out, "raw-block-%d" % n, uniform(n, n), 3, n, {"rawblk:n=%d" % n})
        _c(out, "raw-lits-%d" % n, raw_literals(n, _seed("raw-lits-%d" % n)), 3, 65536, {"litn:raw:%d" % n, "lit:raw:sf%d" % sf})
    # treeless literals in the four size formats, repeat tables, an RLE table in a later block: a second block of the same source
    for extra, sf in ((200, 0), (600, 1), (5000, 2), (45000, 3)):
        d = skewed(131072 + extra, 40, 77)
        _c(out, "treeless-l3-%d" % extra, d, 3, len(d), {"lit:treeless:sf%d:later" % sf})
        _c(out, "treeless-l7-%d" % extra, d, 7, len(d), {"blk:comp:later"})
    _c(out, "ml-rle-later", skewed(131072, 40, 77) + one_word(12, 8, _seed("ml-rle-later"), 40), 3, 65536 * 4, {"ml:rle:later"})
    # the previous tree is preferred up to 1,024 literals below the lazy strategies, and judged by cost elsewhere: a second block of
    # exactly 1,024 / 1,025 literals (1,100 bytes less what the seed's chance matches take) of the first block's 40 symbols, all equally likely
    for n in (1024, 1025):
        d = skewed(131072, 40, 77) + uniform(1100, ("prefer", _seed("prefer-l3-%d" % n)), 40)
        _c(out, "prefer-l3-%d" % n, d, 3, len(d), {"litn:treeless:1024"} if n == 1024 else {"litn:comp:1025"})
    _c(out, "prefer-l7", skewed(131072, 40, 77) + uniform(1000, "prefer7", 40), 7, 132072, {"lit:comp:sf1:later"})
    # LL table in RLE mode; a compressed block behind a raw first block (no tables to inherit)
    for level in (5, 9, 16):
        d = ll_rle_frame(level)
        _c(out, "ll-rle-l%d" % level, d, level, len(d), {"ll:rle", "blk:raw:first", "blk:comp_after_raw_first"}, checksum=level != 9)
    # direct (nibble) tree description; a tree deeper than 11 bits before the limit (the witness is computed in the test)
    _c(out, "fibonacci", fibonacci(), 1, 17710, {"huf:direct"})
    # (twice the counts: more than 8,192 literals, where the 11-bit limit and not the literal count bounds the tree's depth)
    _c(out, "fibonacci-x2", fibonacci(1, 2), 1, 35420, {"huf:direct"})
    # three-byte sequence count; more sequences than blockSize / 4 (minMatch 3: the optimal parsers)
    for level in (16, 19):
        _c(out, "dense-128k-l%d" % level, dense_words(131072, 512, level), level, 131072, {"nbseq:w3"})
    # (the count exactly on the edge: 0x7EFF takes two bytes, 0x7F00 three; the lengths were found by bisection with the oracle)
    for n, k in ((100745, 0x7EFF), (100749, 0x7F00)):
        _c(out, "nbseq-0x%X" % k, dense_words(131072, 512, "edge")[:n], 16, 131072, {"nbseq=%d" % k, "nbseq:w%d" % (2 if k < 0x7F00 else 3)})
    for name, fs, level, nw, nframes, last_dense in (("dense-4k-l12", 4096, 12, 128, 3, False), ("dense-16k-l12", 16384, 12, 512, 3, False),
                                                     ("dense-16k-l22", 16384, 22, 512, 3, False), ("dense-64k-l16", 65536, 16, 512, 3, False),
                                                     ("dense-64k-l16-last", 65536, 16, 512, 3, True)):
        if last_dense:
            d = skewed(2 * fs, 40, 5) + dense_words(fs, nw, name)
        else:
            d = dense_words(nframes * fs, nw, name)
        _c(out, name, d, level, fs, {"dense"})
    # RLE blocks: the first block, and behind a full block; last blocks of 1..7 bytes behind a full block
    _c(out, "rle-blocks", b"q" * (131072 + 5000), 3, 131072 + 5000, {"blk:comp:first", "blk:rle:later", "litn:raw:2"})
    _c(out, "rle-behind-comp", skewed(131072, 40, 9) + b"z" * 3000, 3, 131072 + 3000, {"blk:comp:first", "blk:rle:later"})
    for k in range(1, 8):
        _c(out, "tail-block-%d" % k, skewed(131072 + k, 40, k), 3, 131072 + k, {"tailblk:%d" % k}, checksum=bool(k & 1))
    # ---- found by search with the oracle
    # sequence counts on the edges: k + 1 placements of one word between unique filler. 127 / 128: the count's second byte; 1, 2 / 3: the
    # first count at which one symbol taking all means an RLE table; 31 / 32 and 63 / 64: below dfast's floor of 32 (offsets) and 64
    # (lengths) sequences the tables stay predefined
    for k in (1, 2, 3, 31, 32, 63, 64, 127, 128):
        hit = {"nbseq=%d" % k, "nbseq:w%d" % (1 if k < 128 else 2)} | ({"predef:nbseq<=2"} if k <= 2 else {"ml:rle:first"} if k == 3 else set())
        hit |= {31: {"of:predef"}, 32: {"of:fse"}, 63: {"ll:predef"}, 64: {"ll:fse"}}.get(k, set())
        d = seq_count(k, 40, (k, _seed("nbseq-%d" % k)), 40 if k <= 2 else 8)
        _c(out, "nbseq-%d" % k, d, 3, len(d), hit)
    # offsets of one power-of-two bracket with more than two sequences
    _c(out, "of-rle", _same_bracket(40, _seed("of-rle")), 3, 65536, {"of:rle:nbseq>2"})
    # ML table in RLE mode in a first block: every match is the same 8-byte word
    _c(out, "ml-rle-first", one_word(40, 8, _seed("ml-rle-first")), 3, 65536, {"ml:rle:first"})
    # literal RLE in size format 3: 4,096 and more literals of one byte in a second block whose words all lie in the first
    _c(out, "lit-rle-sf3", lit_rle(4200), 9, 262144, {"lit:rle:sf3"})
    _c(out, "lit-rle-sf1", lit_rle(300), 9, 262144, {"lit:rle:sf1"})
    # near-flat histogram: largest <= (n >> 7) + 4 leaves HUF_compress before a tree is built; the literals go raw. The two sides of the
    # bound: 16 symbols four times each (largest == (64 >> 7) + 4: raw), and one of them a fifth time
    _c(out, "flat-edge-4", even_counts(16, 4, 0, _seed("flat-edge-4")), 3, 64, {"rawblk:n=64"})
    _c(out, "flat-edge-5", even_counts(16, 4, 1, _seed("flat-edge-5")), 3, 65, {"litn:comp:65", "nbseq=0"})
    # (and far inside it, in a block that compresses: every byte value equally often, the first 3,000 bytes again)
    d = flat(20000)
    _c(out, "flat-histogram", d + d[:3000], 3, 65536, {"litn:raw:20000"})
    # a table description that ends fewer than 4 bytes in front of the block's end makes the block raw: thirteen sequences of one literal
    # and the repeat offset each (LL and OF tables in RLE mode, no extra bits), match lengths twelve times 3 and once 4 (a two-byte
    # description; the likely length's states emit next to nothing), in a second block, optimal parser (minMatch 3)
    _c(out, "short-bitstream", short_bitstream(), 16, 262144, {"blk:raw:later", "rawblk:n=61"})
    # more than 128 symbols of two neighbouring weights: inside the same exit (DESIGN.md 26 on why the weights of more than 128 symbols
    # always compress)
    d = two_level(200, 30000)
    _c(out, "two-weights-200", d + d[:3000], 1, 65536, {"blk:comp"})
    return out


def one_word(nrep, wlen, seed=0, gap=400):
    """unique filler of 5..gap bytes and one random word, nrep + 1 times: nrep matches of wlen bytes (the frame's first bytes are filler:
    position 0 is never a match candidate)"""
    r = _rs("oneword", nrep, wlen, seed)
    w = r.randint(0, 256, size=wlen).astype(np.uint8).tobytes()
    out = bytearray()
    for i in range(nrep + 1):
        out += r.randint(0, 256, size=int(r.randint(5, gap))).astype(np.uint8).tobytes() + w
    return bytes(out)


def _same_bracket(nrep, seed=0):
    """one word at distances of 64..124 bytes, no two successive distances equal: every offset value has the same highest bit and
    none is a repeat offset"""
    r = _rs("samebracket", nrep, seed)
    w = r.randint(0, 256, size=8).astype(np.uint8).tobytes()
    out = bytearray(r.randint(0, 256, size=30).astype(np.uint8).tobytes() + w)
    last = 0
    for i in range(nrep):
        g = last
        while g == last:
            g = int(r.randint(64, 125))
        last = g
        out += r.randint(0, 256, size=g - 8).astype(np.uint8).tobytes() + w
    return bytes(out)


def lit_rle(n):
    """second block: n words of 8 bytes, each once, each followed by 0x7F; first block: the same words in another order, each followed by
    a byte that is not 0x7F, and filler to 128 KiB. The literals of the second block are the n bytes 0x7F."""
    r = _rs("litrle", n)
    w = r.randint(0, 256, size=(n, 8)).astype(np.uint8)
    sep = r.randint(0, 0x7F, size=(n, 1)).astype(np.uint8)
    b1 = np.concatenate([w, sep], axis=1).tobytes()
    b1 = b1 + uniform(131072 - len(b1), ("litrle-fill", n))
    b2 = np.concatenate([w[r.permutation(n)], np.full((n, 1), 0x7F, dtype=np.uint8)], axis=1).tobytes()
    return b1 + b2 + b"\x7f" * 16


def short_bitstream(g=12):
    """first block: a random unit of 2,000 bytes over and over; second block: more of it with every fourth byte changed g times, then a
    fifth byte later once more, then eight changed bytes: g sequences of one literal and a match of 3 at the repeat offset, one with a
    match of 4, eight last literals"""
    u = _rs("shortbits").randint(0, 256, size=2000).astype(np.uint8).tobytes()
    n = 4 * g + 5 + 8
    d = bytearray((u * 70)[:131072 + n])
    for p in tuple(range(0, 4 * g + 1, 4)) + tuple(range(n - 8, n)):
        d[131072 + p] ^= 0x55
    return bytes(d)


def even_counts(nsym, times, extra, seed=0):
    """nsym symbols `times` times each, the first `extra` of them once more, shuffled"""
    a = np.concatenate([np.repeat(np.arange(nsym, dtype=np.uint8), times), np.arange(extra, dtype=np.uint8)]) + 97
    _rs("even", nsym, times, extra, seed).shuffle(a)
    return a.tobytes()


def flat(n):
    """every byte value equally often, shuffled"""
    a = np.tile(np.arange(256, dtype=np.uint8), (n + 255) // 256)[:n]
    _rs("flat", n).shuffle(a)
    return a.tobytes()


def two_level(nsym, n):
    """nsym symbols, half of them twice as likely as the other half: two neighbouring weights, alternating"""
    p = np.where(np.arange(nsym) % 2 == 0, 2.0, 1.0)
    return _rs("twolevel", nsym, n).choice(nsym, size=n, p=p / p.sum()).astype(np.uint8).tobytes()


# ------------------------------------------------------------------------------------------------ the randomised cases
LEVELS = (-5, 1, 2, 3, 4, 5, 6, 7, 9, 12, 13, 16, 19)          # every strategy: fast, dfast, greedy, lazy, lazy2, btlazy2, btopt, btultra, btultra2


def random_cases(seed, count=30):
    """[(name, data, level, frame_size, checksum)]: the constructions above at random sizes around their edges"""
    r = _rs("random", seed)
    out = []
    edges = (31, 32, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 16383, 16384)
    for i in range(count):
        kind = int(r.randint(0, 8))
        level = int(LEVELS[r.randint(0, len(LEVELS))])
        ck = bool(r.randint(0, 2))
        e = int(edges[r.randint(0, len(edges))]) + int(r.randint(-1, 2))
        if kind == 0:                                            # skewed literals, one frame of the edge size and a ragged tail
            d, fs = skewed(e + int(r.randint(0, 3)) * e // 2, int(r.choice([3, 40, 200])), (seed, i)), e
        elif kind == 1:                                          # raw literals in a compressed block
            w = words(4, 16, 1, (seed, i))[0]
            d = w + uniform(max(e - len(w), 1), (seed, i)) + w * int(r.randint(1, 9))
            fs = len(d) + int(r.randint(-1, 2))
        elif kind == 2:                                          # second block of the same source
            level = min(level, 9)
            d = skewed(131072 + e, int(r.choice([20, 40, 120])), (seed, i))
            fs = len(d)
        elif kind == 3:                                          # dictionary text behind a raw block
            level = min(level, 9)
            dct, text = words(int(r.choice([256, 2048])), int(r.choice([4, 6, 9])), int(r.randint(50, 3000)), (seed, i))
            d = dct + uniform(131072 - len(dct), (seed, i, "f")) + text
            fs = len(d)
        elif kind == 4:                                          # dense words: frames of 4 / 16 KiB at the minMatch 3 levels, 64 KiB at 16
            fs = int(r.choice([4096, 16384])) + int(r.randint(-1, 2))
            level = int(r.choice([12, 13, 16, 19, 22, 3, 5]))
            d = dense_words(2 * fs + int(r.randint(0, fs)), int(r.choice([128, 512])), (seed, i))
        elif kind == 5:                                          # few sequences between filler
            k = int(r.choice([1, 2, 3, 126, 127, 128, 129]))
            d = seq_count(k, int(r.randint(20, 60)), (seed, i))
            fs = len(d)
        elif kind == 6:                                          # runs: RLE blocks and RLE literals
            d = bytes([int(r.randint(0, 256))]) * (e * int(r.randint(1, 4))) + skewed(int(r.randint(0, 300)), 40, (seed, i))
            fs = max(1, e + int(r.randint(-1, 2)))
        else:                                                    # flat and two-level histograms
            n = int(r.choice([300, 4000, 20000]))
            d = flat(n) if r.randint(0, 2) else two_level(int(r.choice([100, 129, 200, 256])), n)
            fs = len(d) - int(r.randint(0, 2)) * (len(d) // 3)
        out.append(("random-%d-%d" % (seed, i), d, level, max(fs, 1), ck))
    return out
