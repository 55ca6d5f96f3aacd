"""Which format decisions of the entropy stage the encoder's parity inputs reach: walks the ORACLE's archives of a subset of the
existing inputs (twelve (level, frameSize) pairs of test_compress_buffer_bit_exact over the nine generators, seeds 0-23, 2000 and 2001
of test_randomised_differential_compress) and of the directed cases (tests/encoder_cases.py) with describe_frame, and prints per
feature the number of blocks that show it, as a markdown table (profiles/encoder_cases.md keeps the output). CPU only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import corpus as C
import encoder_cases as E
import oracle_lib as O

PAIRS = [(3, 65536), (0, 16384), (3, 16384), (1, 65536), (4, 65536), (5, 65536), (7, 65536), (9, 65536), (3, 262144), (3, 4096), (-1, 65536), (16, 65536)]
EDGES = (31, 32, 63, 64, 255, 256, 1023, 1024, 4095, 4096, 16383, 16384)


def rows():
    r = [("3-byte sequence count (`nbSeq >= 0x7F00`)", lambda b, i: b.get("nb_seq_width") == 3),
         ("`nbSeq == 127` / `nbSeq == 128`", lambda b, i: b.get("nb_seq") in (127, 128)),
         ("`nbSeq` 1 or 2", lambda b, i: b.get("nb_seq") in (1, 2))]
    for k in ("ll", "of", "ml"):
        r.append((k.upper() + " table in RLE mode", lambda b, i, k=k: b.get(k + "_mode") == "rle"))
    for k in ("ll", "of", "ml"):
        r.append((k.upper() + " table in repeat mode", lambda b, i, k=k: b.get(k + "_mode") == "repeat"))
    for sf in range(4):
        r.append(("Treeless literals, size format %d" % sf, lambda b, i, sf=sf: b.get("lit_mode") == "treeless" and b["lit_sf"] == sf))
    for sf in (0, 1, 3):
        r.append(("RLE literals, size format %d" % sf, lambda b, i, sf=sf: b.get("lit_mode") == "rle" and b["lit_sf"] == sf))
    r.append(("Direct (nibble) Huffman header", lambda b, i: b.get("huf_fse") is False))
    for n in EDGES:
        r.append(("Literal count or raw block of exactly %d" % n, lambda b, i, n=n: b.get("lit_regen") == n or (b["type"] == "raw" and b["size"] == n)))
    r.append(("RLE block that is not the first", lambda b, i: b["type"] == "rle" and i > 0))
    r.append(("Compressed block behind a raw first block", lambda b, i: b["type"] == "comp" and i == -1))
    return r


def census(inputs):
    rs = rows()
    counts, blocks = [0] * len(rs), 0
    for d, level, fs, ck in inputs:
        st, arc = O.zra_compress(d, level, fs, ck)
        if st != (0, 0):
            continue
        for fr in E.archive_frames(arc):
            bl = E.describe_frame(fr)
            for i, b in enumerate(bl):
                blocks += 1
                after_raw = i > 0 and bl[0]["type"] == "raw" and all(x["type"] != "comp" for x in bl[:i])
                for k, (name, f) in enumerate(rs):
                    counts[k] += bool(f(b, -1 if after_raw and b["type"] == "comp" else i))
    return blocks, counts


def parity_inputs():
    gens = {"A": C.gen_A(1 << 19), "B": C.gen_B(1 << 19), "C": C.gen_C(1 << 20), "D": C.gen_D(1 << 20), "E": C.gen_E(1 << 20),
            "F": C.gen_struct(1 << 19), "G": C.gen_alpha4(1 << 18), "H": C.gen_litrle(1 << 19), "L": C.gen_loglike(1 << 20)}
    for level, fs in PAIRS:
        for d in gens.values():
            yield (d[: 5 * fs + 777] if fs >= 65536 else d[: 37 * fs + 11]), level, fs, True
    for seed in list(range(24)) + [2000, 2001]:
        rng = np.random.RandomState(1000 + seed)
        for case in range(25):
            fs = int(rng.choice([1024, 4096, 16384, 65536, 65536, 131072, 262144, 50000] + ([300000, 524288] if seed >= 2000 else [])))
            n = int(rng.choice([0, 1, 6, 7, 8, 100, fs - 1, fs, fs + 1, 3 * fs + 17, int(rng.randint(1, 6 * fs))]))
            n = min(n, 600000 if seed < 2000 else 1300000)
            level = int(rng.choice([1, 2, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, -1, -3, -9, -64] + ([11, 12, 13, 15, 17, 19, 22] if seed >= 2000 else [])))
            yield C.random_lz_input(rng, n), level, fs, bool(case & 1)


def main():
    b1, c1 = census(parity_inputs())
    b2, c2 = census((d, level, fs, ck) for name, d, level, fs, ck, must in E.directed_cases())
    print("| Feature | parity inputs (%d blocks) | directed cases (%d blocks) |" % (b1, b2))
    print("|---|---|---|")
    for (name, f), x, y in zip(rows(), c1, c2):
        print("| %s | %d | %d |" % (name, x, y))


if __name__ == "__main__":
    main()
