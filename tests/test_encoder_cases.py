"""The directed encoder inputs (encoder_cases.py) against the CPU oracle: every input compresses and decodes back, the oracle's archive
shows the format decision the input is there for (its must_hit tags, read back by describe_frame), all inputs together cover the
required list, the restatement and libzstd 1.4.9 agree on every byte, and the archives are pinned (tests/golden/encoder_cases.json,
written by tests/golden/make_encoder_cases.py). What the GPU then has to match: test_gpu_encoder_cases.py."""
import hashlib
import json
import os

import pytest

import encoder_cases as E
import frame_craft as F
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))

# one tag per line of the required list (the issue's first table) and per reached line of its second
REQUIRED = {
    # compressed literal counts on the size formats' edges: 1 stream below 256, 4 from there; 63 is a raw block
    "rawblk:n=63", "litn:comp:64", "litn:comp:255", "litn:comp:256", "litn:comp:1023", "litn:comp:1024", "litn:comp:16383", "litn:comp:16384",
    "lit:comp:sf0", "lit:comp:sf1", "lit:comp:sf2", "lit:comp:sf3", "lit:streams1", "lit:streams4", "nbseq=0",
    # raw blocks and raw literals inside a compressed block at the raw header's widths
    "rawblk:n=31", "rawblk:n=32", "rawblk:n=4095", "rawblk:n=4096", "litn:raw:31", "litn:raw:32", "litn:raw:4095", "litn:raw:4096",
    "lit:raw:sf0", "lit:raw:sf1", "lit:raw:sf3",
    # treeless literals in the four size formats; repeat mode of the three tables and an RLE table in a later block
    "lit:treeless:sf0:later", "lit:treeless:sf1:later", "lit:treeless:sf2:later", "lit:treeless:sf3:later",
    "ll:repeat:later", "of:repeat:later", "ml:repeat:later", "ml:rle:later",
    # LL table in RLE mode, a compressed block behind a raw first block
    "ll:rle", "blk:comp_after_raw_first",
    # direct tree description; three-byte sequence count; RLE blocks; short last blocks
    "huf:direct", "huf:fse", "nbseq:w1", "nbseq:w2", "nbseq:w3", "blk:rle:later", "blk:comp:first",
    "tailblk:1", "tailblk:2", "tailblk:3", "tailblk:4", "tailblk:5", "tailblk:6", "tailblk:7",
    # found by search
    "nbseq=1", "nbseq=2", "nbseq=3", "nbseq=127", "nbseq=128", "nbseq=32511", "nbseq=32512", "of:rle:nbseq>2", "ml:rle:first", "predef:nbseq<=2", "lit:rle:sf3", "lit:rle:sf1",
    "litn:raw:20000", "litn:treeless:1024", "litn:comp:1025", "rawblk:n=61",
}


@pytest.fixture(scope="module")
def directed():
    """[(case, status, archive)] — compressed once for the whole module"""
    return [(c, ) + O.zra_compress(c[1], c[2], c[3], c[4]) for c in E.directed_cases()]


def test_every_case_compresses_and_decodes_back(directed):
    names = [c[0][0] for c in directed]
    assert len(set(names)) == len(names)
    for (name, d, level, fs, ck, must), st, arc in directed:
        assert st == (0, 0), name
        st2, back = O.zra_decompress(arc)
        assert st2 == (0, 0) and back == d, name


def test_the_archives_show_what_the_cases_are_for(directed):
    for (name, d, level, fs, ck, must), st, arc in directed:
        got = E.archive_features(arc)
        assert must - {"dense"} <= got, (name, sorted(must - got))


def test_the_cases_cover_the_required_list(directed):
    got = set()
    for c, st, arc in directed:
        got |= E.archive_features(arc)
    assert REQUIRED <= got, sorted(REQUIRED - got)
    assert sum("dense" in c[5] for c, st, arc in directed) >= 5


def test_the_frame_reader_agrees_with_the_match_finder(directed):
    """describe_frame against the oracle's sequences on the frames of one compressed block: the sequence count it reads is the match
    finder's, the literal count the sum of its literal lengths, and the block sizes add up to the frame's content"""
    seen = 0
    for (name, d, level, fs, ck, must), st, arc in directed:
        frames = E.archive_frames(arc)
        assert len(frames) == (len(d) + fs - 1) // fs, name
        for k, fr in enumerate(frames):
            blocks = E.describe_frame(fr)
            assert all(not b["last"] for b in blocks[:-1]) and blocks[-1]["last"], name
            if len(blocks) != 1 or blocks[0]["type"] != "comp":
                continue
            seqs = O.sequences(d[k * fs:(k + 1) * fs], level)
            assert blocks[0]["nb_seq"] == len(seqs) - 1, name
            assert blocks[0]["lit_regen"] == sum(s[0] for s in seqs), name
            seen += 1
    assert seen >= 30


def test_fibonacci_tree_is_deeper_than_the_limit(directed):
    """the witness of the depth limit: the literals the oracle's parse leaves (rebuilt from its sequences) have an unlimited Huffman tree
    deeper than 11 bits, and the archive carries a tree for them"""
    for (name, d, level, fs, ck, must), st, arc in directed:
        if not name.startswith("fibonacci"):
            continue
        lits, p = bytearray(), 0
        for ll, ml, ov in O.sequences(d, level):
            lits += d[p:p + ll]
            p += ll + ml
        counts = {}
        for b in lits:
            counts[b] = counts.get(b, 0) + 1
        depth = max(F.huf_lengths(counts, 64).values())
        print(name, "literals", len(lits), "unlimited depth", depth)
        assert depth > 11, (name, depth)
        assert "litn:comp:%d" % len(lits) in E.archive_features(arc), name


def test_restatement_and_libzstd_agree(directed):
    if not O.have_libzstd():
        pytest.skip("libzstd 1.4.9 not loadable")
    for (name, d, level, fs, ck, must), st, arc in directed:
        st2, arc2 = O.zra_compress(d, level, fs, ck, 0, "zl")
        assert st2 == (0, 0) and arc2 == arc, name


@pytest.mark.parametrize("seed", range(6))
def test_randomised_cases(seed):
    zl = O.have_libzstd()
    for name, d, level, fs, ck in E.random_cases(seed):
        st, arc = O.zra_compress(d, level, fs, ck)
        assert st == (0, 0), name
        assert O.zra_decompress(arc) == ((0, 0), d), name
        for fr in E.archive_frames(arc):
            E.describe_frame(fr)
        if zl:
            assert O.zra_compress(d, level, fs, ck, 0, "zl") == (st, arc), name


def test_archives_are_pinned(directed):
    pin = {e["name"]: e for e in json.load(open(os.path.join(HERE, "golden", "encoder_cases.json")))["cases"]}
    assert set(pin) == {c[0][0] for c in directed}
    for (name, d, level, fs, ck, must), st, arc in directed:
        e = pin[name]
        assert e["input_sha256"] == hashlib.sha256(d).hexdigest(), name
        assert e["archive_sha256"] == hashlib.sha256(arc).hexdigest(), name
        assert set(e["features"]) == E.archive_features(arc), name
