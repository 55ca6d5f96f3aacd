"""The directed encoder inputs (encoder_cases.py; what each is for: test_encoder_cases.py) on the GPU: zra.CompressBuffer gives exactly
the oracle's bytes for every directed and randomised case and zra.DecompressBuffer gives the input back; the match finder's sequences
of the single-block cases are pinned one stage earlier (a mismatch then names the finder or the entropy stage); the directed set runs
again through the single-launch entropy kernel and through the front / chain / back kernels; the single-block level 3 / 4 cases run in
batches of 256 frames beside ordinary frames (the persistent pipeline's split path, both widths of the chain kernel); and the decoder
takes an archive with more sequences than its sequence scratch holds in one round.
Times on the MI355X: profiles/encoder_cases.md."""
import os
import subprocess
import sys

import numpy as np
import pytest

import corpus as C
import encoder_cases as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

CASES = E.directed_cases()
NAMES = [c[0] for c in CASES]
# the levels at which the match finder's sequences are pinned elsewhere too (test_match_finder_sequences_equal_the_oracle)
SEQ_LEVELS = (1, 3, 4, 5, 7, 9)


def _parity(zra, name, d, level, fs, ck):
    st, ref = O.zra_compress(d, level, fs, ck)
    assert st == (0, 0), name
    arc = zra.CompressBuffer(d, level, fs, ck)
    assert arc == ref, (name, level, fs, len(arc), len(ref))
    assert zra.DecompressBuffer(arc) == d, name


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_directed_case_bit_exact(zra, case):
    name, d, level, fs, ck, must = case
    _parity(zra, name, d, level, fs, ck)


@pytest.mark.parametrize("seed", range(6))
def test_randomised_cases_bit_exact(zra, seed):
    for name, d, level, fs, ck in E.random_cases(seed):
        _parity(zra, name, d, level, fs, ck)


def _single_block(case):
    name, d, level, fs, ck, must = case
    return 8 <= len(d) <= min(fs, 131072)                   # (one frame, and no longer than the largest block)


def test_match_finder_sequences_of_the_single_block_cases(zra, gpu_engine):
    """Stage pin: what the match finder leaves for the entropy stage, against the oracle's match finder"""
    import torch
    dev = torch.device("cuda", 0)
    seen = 0
    for case in CASES:
        name, d, level, fs, ck, must = case
        if level not in SEQ_LEVELS or not _single_block(case):
            continue
        t = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(dev)
        out = torch.empty(zra.GetOutputBufferSize(len(d), fs) + 64, dtype=torch.uint8, device=dev)
        gpu_engine.compress(t.data_ptr(), len(d), out.data_ptr(), level, fs, ck)
        seqs, (nb, last_ll, skip) = gpu_engine.debug_read_seqs(0)
        ref = O.sequences(d, level)                              # the oracle appends the block's last literals as (ll, 0, 0)
        assert not skip and len(seqs) == nb, name
        assert seqs + [(last_ll, 0, 0)] == ref, name
        seen += 1
    assert seen >= 30


# seconds a child process of the directed set may take: 20 times the 10 s the slowest one took on the MI355X (profiles/encoder_cases.md)
CHILD_TIMEOUT = 200


@pytest.mark.parametrize("env", [{"ZRA_ENT_SPLIT": "0"}, {"ZRA_ENT_SPLIT": "2"}, {"ZRA_MF_WAVES": "18"}],
                         ids=["entropy-one-launch-on-every-call", "entropy-front-chain-back-on-every-call", "chain-kernel-of-five-frames"])
def test_other_entropy_routes_are_bit_exact_too(env):
    """The library reads its knobs once per process: the directed set again in a fresh process, through the single-launch entropy kernel on
    every call, through the front / chain / back kernels on every call (by default: calls of 256 frames and more), and the batches of 256
    frames with 18 finder waves per CU, where the chain kernel takes five frames per wave."""
    sel = "batches_of_256" if "ZRA_MF_WAVES" in env else "directed_case_bit_exact or batches_of_256"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", sel, "-p", "no:cacheprovider"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stdout[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout


def test_single_block_cases_in_batches_of_256_frames(zra):
    """Every single-block level 3 / 4 case as every other frame of an archive of 256 frames of its size, ordinary frames between them: the
    persistent pipeline then takes the case through the split entropy stage, in one batch with frames that take other decisions."""
    plain = C.gen_loglike(1 << 18)
    seen = 0
    for case in CASES:
        name, d, level, fs, ck, must = case
        if level not in (3, 4) or not _single_block(case):
            continue
        n = len(d)
        data = b"".join(d + plain[(k * 977) % 4096:][:n] for k in range(128))
        assert len(data) == 256 * n
        _parity(zra, name + " x128", data, level, n, ck)
        seen += 1
    assert seen >= 20


def test_decoder_takes_more_sequences_than_its_scratch_holds(zra, gpu_engine):
    """The oracle's archive of 8 MiB of dense three-byte words, 128 frames of 64 KiB at level 16, holds some 2.6 M sequences: more than
    the sequence scratch of a decode pass of that size (decode_scratch: 3/32 of the output in entries, at least 2^20). The parse leaves
    the frames that find no room to the next round; the content comes back whole, and so do random-access reads."""
    import torch
    dev = torch.device("cuda", 0)
    fs, n = 65536, 8 << 20
    d = E.dense_words(n, 512, "decoder")
    st, arc = O.zra_compress(d, 16, fs, True)
    assert st == (0, 0)
    nseq = sum(b.get("nb_seq", 0) for fr in E.archive_frames(arc) for b in E.describe_frame(fr))
    print("sequences", nseq)
    assert nseq > max(128 * (fs + 16) * 3 // 32, 1 << 20)
    assert zra.DecompressBuffer(arc) == d
    rng = np.random.RandomState(7)
    q = 400
    sizes = rng.choice([1, 100, 4096, fs, fs + 1, 3 * fs + 5], size=q).astype(np.uint64)
    offs = np.array([rng.randint(0, n - int(s) - 1) for s in sizes], dtype=np.uint64)
    oo = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    d_arc = torch.from_numpy(np.frombuffer(arc, dtype=np.uint8).copy()).to(dev)
    d_out = torch.zeros(int(sizes.sum()) + 64, dtype=torch.uint8, device=dev)
    gpu_engine.decompress_ra_batch(d_arc.data_ptr(), len(arc), d_out.data_ptr(), offs, sizes, oo)
    host = d_out.cpu().numpy().tobytes()
    for i in range(q):
        o, s, p = int(offs[i]), int(sizes[i]), int(oo[i])
        assert host[p:p + s] == d[o:o + s], (i, o, s)
