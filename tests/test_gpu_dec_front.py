"""The fused front end of the decoder's parse stage (ZRA_DEC_FRONT): the wave that has parsed a block with Huffman-coded literals and a
new tree decodes the literal streams itself; everything else still goes through zra_dec_huf_kernel.

Differential test. Every case runs in two fresh processes (the knob is read once per process), ZRA_DEC_FRONT=1 and =0, both with
ZRA_DEC_SMALL_MAX=0 so that every call takes the throughput pass and not the one-launch kernel. The two runs are compared with each
other and with the CPU oracle's bytes and (zra, zstd) statuses; for a damaged frame the bytes compared are the ones the oracle's call
regenerated before the error. This file run as a script is one such process: it takes all cases from a pickle and writes its results
to another.

Damaged inputs are ones the decoder must answer with a status; nothing here is meant to fault."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import frame_craft as F                                      # noqa: E402

GUARD = 64
RUNS = [{"ZRA_DEC_FRONT": "1"}, {"ZRA_DEC_FRONT": "0"}]


# ------------------------------------------------------------------------------------------------ cases (built once, on the CPU)
def _one_frame_archive(zra, frame, n):
    """a ZRA archive around one zstd frame that regenerates n bytes"""
    return zra.stitch_header([len(frame)], n, max(n, 1)) + frame


def _lits(rng, n, alpha, lo=0):
    return bytes((rng.randint(0, alpha, size=n) + lo).astype(np.uint8))


def _lit_layout(frame):
    """(position of the literals section, header length, tree bytes, [(stream start, stream length)]) of the FIRST block of a crafted
    single-segment frame with a 4-byte content size: 9 bytes of frame header, 3 of block header"""
    p = 12
    b0 = frame[p]
    assert b0 & 3 == 2, "compressed literals with a tree"
    sf = (b0 >> 2) & 3
    lh = 3 if sf < 2 else sf + 2
    v = int.from_bytes(frame[p:p + lh], "little")
    bits = 10 if sf < 2 else 14 if sf == 2 else 18
    comp = v >> (4 + bits)
    hb = frame[p + lh]
    used = 1 + hb if hb < 128 else 1 + (hb - 127 + 1) // 2
    q = p + lh + used
    if sf == 0:
        return p, lh, used, [(q, comp - used)]
    s = [int.from_bytes(frame[q + 2 * k:q + 2 * k + 2], "little") for k in range(3)]
    s.append(comp - used - 6 - sum(s))
    out, at = [], q + 6
    for n in s:
        out.append((at, n))
        at += n
    return p, lh, used, out


def _x2_boundary(O):
    """(n, frames on both sides) of a literal size at which HUF_selectDecoder changes its mind: four streams over 16 equally likely
    symbols, the size stepping over a multiple of 256 (the selector looks at size >> 8)"""
    sel = O.lib().zo_huf_select_decoder
    for d in range(8, 64):
        side = []
        for n in (256 * d - 1, 256 * d):
            info = []
            fr = F.frame_of([F.cblock(_lits(F._rng(77), n, 16, 40), lit_mode="huf4")])
            data = F.write_frame(fr, info)
            side.append((n, fr, data, sel(info[0][0], info[0][1])))
        if side[0][3] != side[1][3]:
            return side
    raise AssertionError("no decoder selection boundary below 16 KiB of literals")


def build_cases(zra, O):
    import corpus
    backend = "zl" if O.have_libzstd() else "zo"
    cases = []

    def add(group, name, arc, cap, **kw):
        want, wbytes = O.zra_decompress(arc, cap, backend, defined_only=True)
        cases.append(dict(group=group, name=name, arc=arc, cap=cap, want=want, wbytes=wbytes, **kw))
        return want

    # ---- frames the oracle's encoder writes: the sizes and levels the issue names
    text = corpus.gen_loglike(1 << 18)
    for n in (1, 7, 255, 256, 1024, 65536, 131072):
        for level in (1, 3, 9):
            data = text[4099:4099 + n]
            assert add("written", "size_%d_level_%d" % (n, level), _one_frame_archive(zra, O.compress_frame(data, level, True), n), n, plain=data) == (0, 0)
    # ---- 300 frames of 4 KiB in one call
    small = (corpus.gen_E(1 << 20) + corpus.gen_loglike(1 << 18, seed=5))[:300 * 4096]
    st, arc = O.zra_compress(small, 3, 4096, True, 0, "zo")
    assert st == (0, 0)
    assert add("batch300", "batch_300_x_4k", arc, len(small), plain=small) == (0, 0)

    # ---- crafted literal sections
    rng = F._rng(4242)
    crafted = {}

    def craft(name, blocks, **kw):
        fr = F.frame_of(blocks, **kw)
        data = F.write_frame(fr)
        plain = F.plaintext(fr)
        crafted[name] = (fr, data, plain)
        assert add("crafted", name, _one_frame_archive(zra, data, len(plain)), len(plain), plain=plain) == (0, 0), name
        return data

    def seq_block(n, produced, mode, **kw):
        lits, seqs, _ = F.gen_block(rng, n, produced, [1, 4, 8], alpha=30)
        return F.cblock(lits, seqs, lit_mode=mode, **kw)

    d = craft("huf1_header3", [F.cblock(_lits(rng, 700, 40), lit_mode="huf1")])
    assert (d[12] >> 2) & 3 == 0
    d = craft("huf4_header3", [F.cblock(_lits(rng, 900, 40), lit_mode="huf4")])
    assert (d[12] >> 2) & 3 == 1
    d = craft("huf4_header4", [F.cblock(_lits(rng, 5000, 40), lit_mode="huf4")])
    assert (d[12] >> 2) & 3 == 2
    d = craft("huf4_header5", [F.cblock(_lits(rng, 20000, 40), lit_mode="huf4")])
    assert (d[12] >> 2) & 3 == 3
    d = craft("huf4_header5_forced_small", [F.cblock(_lits(rng, 300, 40), lit_mode="huf4", size_format=3)])
    assert (d[12] >> 2) & 3 == 3
    craft("huf1_below_a_wave", [F.cblock(_lits(rng, 63, 12), lit_mode="huf1")])          # fewer than 64 literals: the serial decoders
    craft("huf4_with_sequences", [seq_block(30000, 0, "huf4")])
    d = craft("weights_direct", [F.cblock(_lits(rng, 3000, 40), lit_mode="huf4", weights="direct")])
    assert d[12 + 4] >= 128
    d = craft("weights_fse", [F.cblock(_lits(rng, 3000, 200), lit_mode="huf4", weights="fse")])
    assert d[12 + 4] < 128
    # a tree of depth 11, the format's maximum: twelve symbols with counts 1, 1, 2, 4, ...
    deep = bytes([60]) + b"".join(bytes([60 + i]) * (1 << (i - 1)) for i in range(1, 12))        # counts 1, 1, 2, 4, ... 1024
    deep = bytes(np.random.RandomState(3).permutation(np.frombuffer(deep, dtype=np.uint8)))
    cnt = {}
    for b in deep:
        cnt[b] = cnt.get(b, 0) + 1
    assert F.HufTable(F.huf_lengths(cnt, 11)).max_bits == 11
    craft("depth_11", [F.cblock(deep, lit_mode="huf4", max_bits=11)])
    # both sides of the decoder selection boundary
    lo, hi = _x2_boundary(O)
    for n, fr, data, x2 in (lo, hi):
        plain = F.plaintext(fr)
        crafted["select_x%d" % (x2 + 1)] = (fr, data, plain)
        assert add("crafted", "select_boundary_%d_x%d" % (n, x2 + 1), _one_frame_archive(zra, data, n), n, plain=plain) == (0, 0)
    # a treeless block behind a compressed one: 128 KiB + 1 bytes in two blocks (the second block's literals go through the Huffman
    # kernel, the first one's do not), and new tree / kept tree / new tree in three blocks
    first = seq_block(131072, 0, "huf4")
    craft("treeless_second_block_128k_plus_1", [first, F.cblock(first[1]["lits"][:1], lit_mode="treeless1")])
    craft("tree_treeless_tree", [F.cblock(_lits(rng, 1000, 40), lit_mode="huf4"), F.cblock(_lits(rng, 1000, 40), lit_mode="treeless4"),
                                 F.cblock(_lits(rng, 1000, 25, 100), lit_mode="huf4")])

    # ---- damaged literal sections: on both sides of the decoder selection (libzstd's two decoders accept different damaged streams)
    def damaged(name, data, n, plain):
        add("damaged", name, _one_frame_archive(zra, bytes(data), n), n, plain=plain)

    for tag in ("select_x1", "select_x2", "huf1_header3", "huf4_header4", "huf4_header5"):
        fr, data, plain = crafted[tag]
        p, lh, used, streams = _lit_layout(data)
        for k, (at, ln) in enumerate(streams):
            b = bytearray(data)
            b[at + ln // 2] ^= 0x08
            damaged("%s_bit_flip_stream_%d" % (tag, k), b, len(plain), plain)
            b = bytearray(data)
            b[at + ln - 1] ^= 0x01 if data[at + ln - 1] > 1 else 0x02      # (the last byte holds the end mark: the whole stream shifts by a bit)
            damaged("%s_bit_flip_stream_end_%d" % (tag, k), b, len(plain), plain)
            b = bytearray(data)
            b[at + ln - 1] = 0
            damaged("%s_zero_end_stream_%d" % (tag, k), b, len(plain), plain)
        if len(streams) == 4:
            b = bytearray(data)
            b[p + lh + used:p + lh + used + 2] = b"\xFF\xFF"
            damaged("%s_jump_table_past_the_section" % tag, b, len(plain), plain)
        # the section cut short / declared longer than the block, in the header's compressed-size field
        sf = (data[p] >> 2) & 3
        bits = 10 if sf < 2 else 14 if sf == 2 else 18
        v = int.from_bytes(data[p:p + lh], "little")
        for delta in (-3, 1 << (bits - 1)):
            b = bytearray(data)
            comp = ((v >> (4 + bits)) + delta) & ((1 << bits) - 1)
            b[p:p + lh] = ((v & ((1 << (4 + bits)) - 1)) | (comp << (4 + bits))).to_bytes(lh, "little")
            damaged("%s_section_size_%+d" % (tag, delta), b, len(plain), plain)
    # (a flipped bit does not have to be an error: a stream may fall back into step and end where it should, with other bytes)
    assert sum(c["want"] != (0, 0) for c in cases if c["group"] == "damaged") >= 30
    assert sum(c["want"] == (0, 0) and c["wbytes"] != c["plain"] for c in cases if c["group"] == "damaged") >= 4

    # ---- the reference decodes the literals before it looks at the sequence tables: a block that is wrong in both places answers with
    #      the literals' error. The sequences section of this block is the one byte 0x00; 0x80 announces a second byte that is not there.
    fr, data, plain = crafted["huf4_header4"]
    _, _, _, streams = _lit_layout(data)
    seq_only = bytearray(data)
    assert seq_only[-1] == 0
    seq_only[-1] = 0x80
    both = bytearray(seq_only)
    both[streams[1][0] + streams[1][1] - 1] = 0
    lit_only = bytearray(data)
    lit_only[streams[1][0] + streams[1][1] - 1] = 0
    w_seq = add("order", "sequence_header_only", _one_frame_archive(zra, bytes(seq_only), len(plain)), len(plain), plain=plain)
    w_lit = add("order", "literals_only", _one_frame_archive(zra, bytes(lit_only), len(plain)), len(plain), plain=plain)
    w_both = add("order", "literals_and_sequence_header", _one_frame_archive(zra, bytes(both), len(plain)), len(plain), plain=plain)
    assert w_seq[0] and w_lit[0] and w_seq != w_lit and w_both == w_lit, (w_seq, w_lit, w_both)

    # ---- batched random access over 64 frames of 64 KiB
    body = (corpus.gen_loglike(2 << 20, seed=11) + corpus.gen_E(1 << 20) + corpus.gen_struct(1 << 20))[:64 * 65536]
    st, arc = O.zra_compress(body, 3, 65536, True, 0, "zo")
    assert st == (0, 0)
    q = np.random.RandomState(9)
    offs = [0, 65535, 65536 * 63, len(body) - 4097] + [int(x) for x in q.randint(0, len(body) - 4097, size=200)]
    sizes = [1, 2, 4096, 4096] + [int(x) for x in q.choice([1, 100, 4096], size=200)]
    cases.append(dict(group="ra", name="ra_64_x_64k", arc=arc, cap=len(body), plain=body, offs=offs, sizes=sizes, want=(0, 0), wbytes=body))

    # ---- literal scratch exhaustion: the scratch of a round holds half of the output, frames that are nearly all Huffman-coded
    #      literals (64 equally likely byte values: no matches worth taking, 6 bits per byte) need all of it, so about half of the
    #      blocks are deferred to the next round
    lit_heavy = _lits(np.random.RandomState(21), 48 * 65536, 64, 32)
    st, arc = O.zra_compress(lit_heavy, 3, 65536, True, 0, "zo")
    assert st == (0, 0) and len(arc) < len(lit_heavy) * 7 // 8
    cases.append(dict(group="defer", name="literal_scratch_deferral", arc=arc, cap=len(lit_heavy), plain=lit_heavy, want=(0, 0), wbytes=lit_heavy))
    return cases


# ------------------------------------------------------------------------------------------------ one process
def run_cases(path_in, path_out):
    import torch
    import zra_amd as Z
    cases = pickle.load(open(path_in, "rb"))
    L = Z.load()
    eng = Z.Engine(0)
    dev = torch.device("cuda", 0)
    res = {}
    for c in cases:
        arc, cap = c["arc"], c["cap"]
        d_arc = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).to(dev)
        if c["group"] == "ra":
            offs = np.array(c["offs"], dtype=np.uint64)
            sizes = np.array(c["sizes"], dtype=np.uint64)
            oofs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
            total = int(sizes.sum())
            got = {}
            for opt in (0, 8):                               # 0: a frame is decoded as far as its queries reach; 8: whole frames
                d_ra = torch.full((total + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
                L.ZraHipSetOptions(opt)
                try:
                    eng.decompress_ra_batch(d_arc.data_ptr(), len(arc), d_ra.data_ptr(), offs, sizes, oofs)
                    got[opt] = ((0, 0), bytes(d_ra.cpu().numpy()))
                except Z.ZraError as e:
                    got[opt] = ((e.zra, e.zstd), b"")
                finally:
                    L.ZraHipSetOptions(0)
            res[c["name"]] = got
            continue
        d_out = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
        try:
            eng.decompress(d_arc.data_ptr(), len(arc), d_out.data_ptr(), cap)
            st = (0, 0)
        except Z.ZraError as e:
            st = (e.zra, e.zstd)
        res[c["name"]] = (st, bytes(d_out.cpu().numpy()), eng.decode_stage_stats()["rounds"])
    eng.close()
    with open(path_out, "wb") as f:
        pickle.dump(res, f)
    print("cases", len(res))


@pytest.fixture(scope="module")
def runs(zra, oracle, tmp_path_factory):
    """(cases, [results of the ZRA_DEC_FRONT=1 process, results of the =0 process]); the two processes run side by side"""
    tmp = tmp_path_factory.mktemp("dec_front")
    cases = build_cases(zra, oracle)
    path = str(tmp / "cases.pickle")
    with open(path, "wb") as f:
        pickle.dump(cases, f)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), path, str(tmp / ("out%d.pickle" % k))],
                              env=dict(os.environ, ZRA_DEC_SMALL_MAX="0", **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k, env in enumerate(RUNS)]
    out = []
    for k, p in enumerate(procs):
        try:
            so, se = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            so, se = p.communicate()
            se += "\n(killed at its time limit)"
        assert p.returncode == 0, (RUNS[k], so[-1500:], se[-1500:])
        out.append(pickle.load(open(str(tmp / ("out%d.pickle" % k)), "rb")))
    return cases, out


def _check_decode(cases, out, group):
    seen = 0
    for c in cases:
        if c["group"] != group:
            continue
        seen += 1
        n = len(c["wbytes"])
        for k, r in enumerate(out):
            st, got, _ = r[c["name"]]
            assert st == c["want"], (c["name"], RUNS[k], st, c["want"])
            assert got[:n] == c["wbytes"], (c["name"], RUNS[k], "bytes the oracle regenerated")
            assert got[c["cap"]:] == b"\xEE" * GUARD, (c["name"], RUNS[k], "guard behind the output")
            if c["want"] == (0, 0) and group != "damaged":
                assert n == c["cap"] and got[:n] == c["plain"], (c["name"], RUNS[k])
        assert out[0][c["name"]][0] == out[1][c["name"]][0] and out[0][c["name"]][1][:n] == out[1][c["name"]][1][:n], c["name"]
    return seen


@pytest.mark.gpu
def test_frames_written_by_the_oracle(runs):
    """1, 7, 255, 256, 1,024, 65,536 and 131,072 bytes at levels 1, 3 and 9: bytes and status of both runs equal the oracle's."""
    assert _check_decode(*runs, "written") == 21


@pytest.mark.gpu
def test_batch_of_300_small_frames(runs):
    """300 frames of 4 KiB in one call (the throughput pass, several jobs per parse wave)."""
    assert _check_decode(*runs, "batch300") == 1


@pytest.mark.gpu
def test_crafted_literal_sections(runs):
    """One and four streams; the 3-, 4- and 5-byte section headers; both sides of the X1 / X2 decoder selection; directly stored and
    FSE-coded weights; a tree of depth 11; fewer literals than a wave has lanes; a treeless block behind a compressed one (128 KiB + 1
    bytes in two blocks) and between two blocks with trees of their own."""
    cases, out = runs
    assert _check_decode(cases, out, "crafted") == 14
    # the two-block frame took two rounds: its second block's literals went through the Huffman kernel
    assert all(r["treeless_second_block_128k_plus_1"][2] == 2 for r in out)


@pytest.mark.gpu
def test_damaged_literal_sections(runs):
    """A flipped bit in each stream, a stream that ends in a zero byte, a jump table that points past the section, a section cut
    short or declared longer than its block — on a single-stream section and on four-stream ones on both sides of libzstd's decoder
    selection: the status, and the bytes regenerated before the error, equal the oracle's and each other's."""
    assert _check_decode(*runs, "damaged") >= 60


@pytest.mark.gpu
def test_literal_error_comes_before_the_sequence_header_error(runs):
    """A block damaged in a literal stream AND in its sequences header reports the literals' status (hufErr before lateErr), as the
    oracle does; the two damages alone report different statuses (asserted when the cases are built)."""
    assert _check_decode(*runs, "order") == 3


@pytest.mark.gpu
def test_batched_random_access(runs):
    """204 queries over 64 frames of 64 KiB, frames decoded as far as the queries reach (options 0) and whole (option bit 8): every
    answer equals the input, in both runs."""
    cases, out = runs
    c = [x for x in cases if x["group"] == "ra"][0]
    total = sum(c["sizes"])
    for k, r in enumerate(out):
        for opt in (0, 8):
            st, got = r[c["name"]][opt]
            assert st == (0, 0), (RUNS[k], opt, st)
            at = 0
            for o, s in zip(c["offs"], c["sizes"]):
                assert got[at:at + s] == c["plain"][o:o + s], (RUNS[k], opt, o, s)
                at += s
            assert got[total:] == b"\xEE" * GUARD, (RUNS[k], opt)
    assert out[0][c["name"]] == out[1][c["name"]]


@pytest.mark.gpu
def test_blocks_deferred_for_literal_scratch(runs):
    """48 frames of 64 KiB that are nearly all Huffman-coded literals need twice the literal scratch a round has: about half of the
    blocks wait for the next round (asserted: the single-block frames took more than one round) and come back through the same path;
    the output equals the input in both runs. (The shortage comes from the data: the scratch is sized at half of the output by rule.
    ZRA_ALLOC_LIMIT_MIB cannot produce it — a reservation above that limit fails with memory_allocation, it does not shrink.)"""
    cases, out = runs
    assert _check_decode(cases, out, "defer") == 1
    assert all(r["literal_scratch_deferral"][2] >= 2 for r in out)


if __name__ == "__main__":
    run_cases(sys.argv[1], sys.argv[2])
