"""CPU half of the decoder's conformance suite (tests/frame_craft.py writes valid zstd frames that no one-shot encoder of libzstd 1.4.9
produces): for every directed and every randomised frame, the plaintext computed in Python from the description alone, libzstd's
decoder and the restated decoder (oracle/zo_decode.c, which stands in for libzstd where the image lacks it) agree; the writer refuses
what it cannot encode as asked; the randomised descriptions reach every feature; the recorded fixtures pin the writer's bytes."""
import base64
import hashlib
import json
import os

import pytest

import frame_craft as F
import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crafted_frames.json")


def _backends():
    return ("zl", "zo") if O.have_libzstd() else ("zo",)


def _agree(name, fr, data, error):
    plain = F.plaintext(fr, check=False)
    cap = (len(plain) if plain is not None else 4096) + 16
    got = {b: O.decompress(data, cap, b) for b in _backends()}
    if error:
        codes = {b: g[1] for b, g in got.items()}
        assert all(codes.values()) and len(set(codes.values())) == 1, (name, codes)
    else:
        for b, (out, err) in got.items():
            assert err == 0 and out == plain, (name, b, err, len(plain))
    return got


@pytest.fixture(scope="module")
def directed():
    return [(c, F.write_frame(c["frame"])) for c in F.directed_cases()]


def test_directed_frames_three_way(directed):
    """python_plaintext == zl_decompress(frame) == zo_decompress(frame) for every directed frame; equal error codes for the frames that
    are invalid on purpose. error=None marks the frames whose expectation is libzstd's answer whatever it is: both decoders agree, and
    where they decode, with the plaintext."""
    names = [c["name"] for c, _ in directed]
    assert len(names) == len(set(names)) and len(names) > 150
    for c, data in directed:
        if c["error"] is None:
            plain = F.plaintext(c["frame"])
            got = {b: O.decompress(data, len(plain) + 16, b) for b in _backends()}
            assert len({g[1] for g in got.values()}) == 1, (c["name"], got)
            for b, (out, err) in got.items():
                assert err or out == plain, (c["name"], b)
        else:
            _agree(c["name"], c["frame"], data, c["error"])


def test_directed_frames_are_what_they_claim(directed):
    """the properties the cases are named after hold in the written bytes (a change that tames a case shows here)"""
    by = {c["name"]: (c, d) for c, d in directed}
    fr = by["geom_only_second_to_last_short"][0]["frame"]
    assert F.block_sizes(fr) == [131072, 100000, 31072]
    assert sum(1 for b in by["geom_40_blocks"][0]["frame"]["blocks"] if b[0] == "compressed") == 40
    for n, head in ((127, b"\x7f"), (128, b"\x80\x80"), (0x7EFF, b"\xfe\xff"), (0x7F00, b"\xff\x00\x00"), (0x7F06, b"\xff\x06\x00")):
        c, d = by["geom_count_%d" % n]
        blk = c["frame"]["blocks"][0][1]
        assert len(blk["seqs"]) == n and F._sequences(blk, F._State())[:len(head)] == head, n
    assert sorted(n[-1] for n in by if n.startswith("endmark_seq_bit_")) == list("01234567")
    assert sorted(n[-1] for n in by if n.startswith("endmark_huf_bit_")) == list("01234567")
    d = by["header_window_32MiB_long_offsets"][1]
    assert d[4] & 0x20 == 0 and d[5] == 15 << 3
    assert by["header_window_2GiB_long_offsets"][1][5] == 21 << 3
    assert by["lits_direct_128_weights"][1][16] == 255         # the tree description opens with 127 + 128 weights
    # libzstd's choice between its Huffman decoders (HUF_selectDecoder: 0 single-symbol, 1 double-symbol) for 4-stream literals with a
    # new tree, on both sides of its boundary, and a treeless block that inherits a double-symbol table
    def decoder(name, block=0):
        info = []
        F.write_frame(by[name][0]["frame"], info)
        return O.lib().zo_huf_select_decoder(*info[block])
    assert decoder("lits_huf4_700_format1") == 0 and decoder("lits_huf4_9000_format2") == 0
    assert decoder("lits_huf4_40000_format3") == 1
    for name in ("lits_huf4_then_treeless4_narrow", "lits_huf4_then_treeless1_wide"):
        blocks = [b[1] for b in by[name][0]["frame"]["blocks"] if b[0] == "compressed"]
        assert decoder(name) == 1 and blocks[0]["lit_mode"] == "huf4" and blocks[3]["lit_mode"].startswith("treeless")
    # the largest lengths the codes express sit in blocks above 128 KiB, behind an explicit switch
    assert max(s[1] for b in by["overlimit_match_length_131074_last_block"][0]["frame"]["blocks"] if b[0] == "compressed" for s in b[1]["seqs"]) == 131074
    assert by["overlimit_literal_length_131071"][0]["frame"]["blocks"][0][1]["seqs"][0][0] == 131071
    with pytest.raises(F.CraftError):
        F.write_frame(dict(by["overlimit_literal_length_131071"][0]["frame"], over_limit=False))
    assert F.plaintext(by["rep_ll0_v3_at_rep1_of_1"][0]["frame"])[13:19] == b"h" * 6     # libzstd: the zero offset is taken for 1


def test_writer_refuses_what_it_cannot_encode():
    lits = bytes(range(40)) * 3
    two = [(3, 5, 10 + 3), (4, 6, 20 + 3)]

    def refuse(blocks, **kw):
        with pytest.raises(F.CraftError):
            F.write_frame(F.frame_of(blocks, **kw))
    refuse([F.cblock(lits, two, modes=dict(ll="rle"))])                            # RLE mode, two distinct codes
    refuse([F.cblock(lits, two, modes=dict(of="repeat"))])                         # repeat mode, no table in force
    refuse([F.cblock(lits, [(3, 5, 13)], modes=dict(of="rle")), F.cblock(lits, [(3, 5, 300)], modes=dict(of="repeat"))])   # code outside the kept table
    refuse([F.cblock(bytes(range(200)) + b"\0" * 999, lit_mode="huf4", max_bits=7)])  # 200 symbols in 7 bits
    refuse([F.cblock(lits, lit_mode="treeless4")])                                 # no tree in force
    refuse([F.cblock(lits, lit_mode="huf4"), F.cblock(b"\xf0" * 30, lit_mode="treeless1")])   # literal outside the kept tree
    refuse([("raw", b"x" * (F.BLOCK_MAX + 1))])
    refuse([("raw", b"x" * 2000)], window=(0, 0), fcs_width=0)                      # block above the 1 KiB window
    refuse([("raw", b"x" * 1000), F.cblock(lits, [(3, 5, 2000 + 3)])])             # offset beyond the output
    refuse([F.cblock(lits, lit_mode="huf1", size_format=1)])                       # one stream has one format
    refuse([F.cblock(lits * 30, lit_mode="raw", size_format=0)])                   # 3,600 literals in 5 bits
    refuse([F.cblock(lits, two, count_width=3)])                                   # the three-byte count starts at 0x7F00
    refuse([F.cblock(lits, lit_mode="rle")])
    refuse([("raw", b"x" * 300)], fcs_width=1)
    refuse([("raw", b"x" * 30)], fcs_width=2)
    refuse([("raw", b"x" * 30)], single_segment=True, fcs_width=0)
    refuse([F.cblock(lits, two, modes=dict(ll="fse"), logs=dict(ll=10))])
    refuse([F.cblock(lits, [(3, 131075, 4)])])


def test_checksum_restatement():
    for n in (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 1000, 70001):
        d = bytes((i * 131 + (i >> 3)) & 0xFF for i in range(n))
        assert F.xxh64(d) == O.lib().zo_xxh64(d, n, 0), n


@pytest.fixture(scope="module")
def drawn():
    return {seed: F.random_frames(seed) for seed in F.RANDOM_SEEDS}


def test_randomised_frames_three_way(drawn):
    """6 seeds x 40 frames; at most 10 % of a seed's drawn descriptions refused by the writer (refused ones are redrawn, not dropped)"""
    assert len(drawn) == 6
    for seed, (frames, refused) in drawn.items():
        assert len(frames) == 40
        assert refused <= 0.1 * (len(frames) + refused), (seed, refused)
        for k, (fr, tags, data) in enumerate(frames):
            _agree("random_%d_%d" % (seed, k), fr, data, False)


def test_randomised_frames_reach_every_feature(drawn):
    count = {t: 0 for t in F.RANDOM_TAGS}
    full = 0
    for frames, _ in drawn.values():
        for fr, tags, data in frames:
            assert tags <= set(F.RANDOM_TAGS), tags - set(F.RANDOM_TAGS)
            for t in tags:
                count[t] += 1
            full += sum(F.block_sizes(fr)) == F.FRAME_SIZE
    assert min(count.values()) >= 3, sorted((v, t) for t, v in count.items())[:5]
    assert full >= 36                                          # what the long mixed archive of the GPU half is made of


def test_fixtures_pin_the_writer(directed):
    """tests/golden/crafted_frames.json (tests/golden/make_crafted.py): the writer still produces those exact bytes, the plaintext is
    the recorded one, and libzstd (where present) still answers the recorded status"""
    rec = {e["name"]: e for e in json.load(open(GOLDEN))}
    assert set(rec) == {c["name"] for c, _ in directed}
    assert os.path.getsize(GOLDEN) < 200 << 10
    for c, data in directed:
        e = rec[c["name"]]
        assert hashlib.sha256(data).hexdigest() == e["frame_sha256"], c["name"]
        if "frame_b64" in e:
            assert base64.b64decode(e["frame_b64"]) == data and len(data) < 4096, c["name"]
        assert e["tags"] == c["tags"]
        assert bool(e["zl_status"]) == bool(c["error"]) or c["error"] is None, c["name"]
        if e["sha256"]:
            assert hashlib.sha256(F.plaintext(c["frame"])).hexdigest() == e["sha256"], c["name"]
        for b in _backends():                                  # (the restated decoder is held to libzstd's recorded status everywhere)
            assert O.decompress(data, 1 << 19, b)[1] == e["zl_status"], (c["name"], b)
