"""CPU checks of what tests/test_gpu_alloc_failure.py rests on (tests/alloc_failure_cases.py): the archives it builds from repeated
frames behind a stitched header are archives of their content, by the oracle; and the sizes its groups are built on lie on the sides
of their limits the comments there say, by the formulas of the code they quote (DevBuf::reserve pads a request r to r + r / 8 + 256)."""
import numpy as np

import alloc_failure_cases as AC


def padded(r):
    return r + r // 8 + 256


def test_repeated_frames_behind_a_stitched_header_are_an_archive_of_the_repeated_content(oracle, zra):
    AC.Z, AC.O = zra, oracle
    fs = 4096
    a, b = AC.Unit(AC.lz_bytes(1, 3 * fs), fs), AC.Unit(AC.lz_bytes(2, 3 * fs), fs)
    bad = a.frames[1][:-1] + bytes([a.frames[1][-1] ^ 0x40])
    arc, content = a.archive(8, swap={2: (b, 1), 7: (b, 0)})
    assert content == b"".join((b.base[fs:2 * fs] if i == 2 else b.base[:fs] if i == 7 else a.base[(i % 3) * fs:(i % 3 + 1) * fs]) for i in range(8))
    assert oracle.zra_decompress(arc) == ((0, 0), content)
    assert oracle.zra_decompress(a.archive(8, damage={4: bad})[0])[0] == (1, 22)       # (a frame's last four bytes: its content checksum)
    assert oracle.decompress(bad, fs) == (None, 22)


def test_the_sizes_of_the_groups_straddle_their_limits():
    limit = 11 << 20
    # decode_scratch (rounds) and decode_launch (block pass), n frames of 256 KiB
    rounds = lambda n: (padded(max(n * 131088 // 2, 1 << 20) + 64), padded(8 * max(n * 131088 * 3 // 32, 1 << 20) + 64))
    block = lambda n: (padded(max(n * 262160 // 2, 1 << 20) + 64), padded(8 * max(n * 262160 * 3 // 32, 1 << 20) + 64))
    assert max(rounds(64)) < limit and block(64)[0] < limit < block(64)[1]
    assert max(rounds(96)) < limit < block(96)[0]
    assert rounds(256)[0] > limit
    assert (rounds(64), block(64), rounds(96)[1], block(96)[0]) == ((4719496, 9437512), (9438088, 14156968), 10618456, 14156968)
    # stage_ of the batch, the handle read and the update: touched frames of 64 KiB
    assert padded(100 * 65536 + 64) < limit < padded(200 * 65536 + 64)
    # a cached handle's read of 300,000 queries of three slices: 32 bytes a tuple fit, 16 bytes a slice do not
    assert padded(32 * 300000 + 64) == 10800328 < limit < padded(16 * 900000 + 64) == 16200328
    # the scans' window (256 bytes of carry in front), the frame passes' and the locate sweep's; the read's byte fetch; a pair window
    frames, fs, slots = AC.SCAN_FRAMES, AC.SCAN_FS, AC.STAGING // AC.SCAN_FS
    assert padded(256 + slots * fs + 64) < limit < padded(256 + frames * fs + 64) and padded(slots * fs + 64) < limit < padded(frames * fs + 64)
    assert padded(400 * fs + 64) < limit and min(frames, 2 * 400) == frames
    assert frames * fs == 12 << 20 and AC.LO // fs == 192 and (AC.HI - 1) // fs == 480          # two passes of 256 slots, three of 128 pairs
    # the decoder's scratch of a pass of at most 256 jobs: the floor of decSeqs_
    assert padded(8 * (1 << 20) + 64) < limit and 256 * (fs + 16) * 3 // 32 < 1 << 20
    # lists: 16 bytes an entry of the caller's capacity
    assert padded(16 * (1 << 17) + 64) < limit < padded(16 * (1 << 20) + 64)
    # the tally's table: 2^19 slots for 330,000 records, 1,024 for 600 promised keys
    import tally_model as TM
    assert TM.slots(330000) == 1 << 19 and TM.slots(330000, 600) == 1024
    tiles = -(-990000 // 4096)
    assert padded(16 * (tiles + 1) + 2 * tiles * 512 + 24 * 1024) < limit < padded(16 * (tiles + 1) + 2 * tiles * 512 + 24 * (1 << 19))
