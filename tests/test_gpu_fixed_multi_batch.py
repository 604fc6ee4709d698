"""GPU parity of gs_motif_sampling_multi_batch_fixed
(Context.motif_sampling_multi_batch(pcv=, ppm=)): R repetitions of the ByPCV pipeline or of
doMotifSamplingWithPPM with Positions lists (motifAmount >= 2) in one call.

On the .fsx:407 set (5 x 27 bp, W = 6, motifAmount 2): under a PCV every row against the
literal restatement's findBestMotifPositionsWithStartPositionsByPCV /
…PositionByPCV (oracle/gibbs_ref.py) fed the oracle's WithBPV starts, under a PPM against
the oracle's sweep_lists / greedy_lists fed its OfPPM starts.  On larger sets against the
sequential entry point gs_motif_sampling_multi on a second context that has the values set
on it: list lengths, positions and pass counts equal, PWMS bit-identical (the same device
functions in the same operation order)."""
import json
from pathlib import Path

import numpy as np
import pytest

from conftest import make_dataset
from fixed_batch_cases import (PC, PROTEIN, SEEDS, bits, pcv49, ppm49, set_fixed, sources_of)
from oracle import gibbs_ref as gr
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
GOLDEN = Path(__file__).resolve().parent / "golden"
CUTOFF = 1.0
KINDS = ("pcv", "ppm", "both")

# name: (alphabet, N, L, W, motifAmount, init_mode, dataset seed)
SHAPES = {
    "dna-m2": (b"ACGT", 40, 60, 7, 2, 0, 31),
    "dna-m3-shared": (b"ACGT", 12, 40, 4, 3, 1, 32),
    "protein-m2": (PROTEIN, 12, 40, 4, 2, 0, 33),
}


def fsx_set():
    seqs = json.loads((GOLDEN / "fsx_sets.json").read_text())["bioTestsWithMultipleSamples"]["seqs"]
    codes = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
    offsets = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    return seqs, codes, offsets


def row(out, r):
    cnt, pos, pwms, passes, status = out
    return cnt[r], pos[r], pwms[r], int(passes[r])


def check_sequential(g, s, what):
    """(cnt, pos, pwms, passes) of one chain against gs_motif_sampling_multi's."""
    gc, gp, gw, gpass = g
    sc, sp, sw, spass = s
    assert np.array_equal(gc, sc) and gpass == spass, what
    for n in range(len(gc)):
        assert np.array_equal(gp[n, :gc[n]], sp[n, :sc[n]]), (what, n)
    assert np.array_equal(bits(gw), bits(sw)), what


def fresh(tuning=None):
    from gibbssampling_amd import Context
    return Context(0, tuning=tuning)


@pytest.fixture(scope="module")
def other_ctx():
    ctx = fresh()
    yield ctx
    ctx.close()


_fsx = {}


def fsx_case(kind, batch_starts):
    """The .fsx:407 set's batch under the values of `kind`, computed once."""
    if (kind, batch_starts) not in _fsx:
        seqs, codes, offsets = fsx_set()
        alpha, W, M = b"ATGC-", 6, 2
        pcv = pcv49(alpha, 407) if kind == "pcv" else None
        ppm = ppm49(W, 408) if kind == "ppm" else None
        ctx = fresh({"batch_starts": batch_starts})
        ctx.set_sequences(codes, offsets, alpha)
        out = ctx.motif_sampling_multi_batch(M, W, PC, CUTOFF, SEEDS, pcv=pcv, ppm=ppm)
        ctx.close()
        _fsx[kind, batch_starts] = (pcv, ppm, out)
    return _fsx[kind, batch_starts]


@pytest.mark.parametrize("batch_starts", [0, 1])
def test_fsx_407_under_a_pcv_equals_the_literal_restatement(batch_starts):
    seqs, codes, offsets = fsx_set()
    alpha, W, M, N = b"ATGC-", 6, 2, len(seqs)
    pcv, _, out = fsx_case("pcv", batch_starts)
    cnt, pos, pwms, passes, status = out
    assert cnt.shape == (len(SEEDS), N) and pos.shape == (len(SEEDS), N, M)
    assert not status.any()
    S = ol.Seqs(codes, offsets, alpha)
    sources = [list(codes[offsets[i]:offsets[i + 1]]) for i in range(N)]
    rows = set()
    for r, seed in enumerate(SEEDS):
        sc, p = ol.random_starts(S, W, PC, seed=seed, mode=0, pcv49=pcv)
        u = [ol.uniform(seed, ol.stream_sweep(0), n) for n in range(N)]
        swept = gr.findBestMotifPositionsWithStartPositionsByPCV(
            M, W, PC, CUTOFF, list(alpha), sources, list(pcv),
            [(float(sc[n]), [int(p[n])]) for n in range(N)], u)
        ref = gr.findBestMotifPositionsWithStartPositionByPCV(
            M, W, PC, CUTOFF, list(alpha), sources, list(pcv),
            [(w, list(ps)) for w, ps in swept])
        for n in range(N):
            assert list(pos[r, n, :cnt[r, n]]) == list(ref[n][1]), (seed, r, n)
            w = ref[n][0]
            assert pwms[r, n] == w or abs(pwms[r, n] - w) <= RTOL * abs(w), (seed, r, n)
        rows.add(pos[r].tobytes())
    assert len(rows) > 1  # the seeds reach the chains
    assert np.array_equal(cnt[1], cnt[3]) and np.array_equal(bits(pwms[1]), bits(pwms[3]))


@pytest.mark.parametrize("batch_starts", [0, 1])
def test_fsx_407_under_a_ppm_equals_the_oracle(batch_starts):
    seqs, codes, offsets = fsx_set()
    alpha, W, M, N = b"ATGC-", 6, 2, len(seqs)
    _, ppm, out = fsx_case("ppm", batch_starts)
    assert not out[4].any()
    S = ol.Seqs(codes, offsets, alpha)
    for r, seed in enumerate(SEEDS):
        sc, p = ol.random_starts(S, W, PC, seed=seed, mode=0, ppm49=ppm)
        u = np.array([ol.uniform(seed, ol.stream_sweep(0), n) for n in range(N)])
        lst = np.full((N, M), -1, np.int32)
        lst[:, 0] = p
        c1, p1, w1 = ol.sweep_lists(S, M, W, PC, CUTOFF, np.ones(N, np.int32), lst, M, u)
        oc, op, ow, opass = ol.greedy_lists(S, M, W, PC, CUTOFF, c1, p1, M, w1)
        gc, gp, gw, gpass = row(out, r)
        assert np.array_equal(gc, oc) and gpass == opass, (seed, r)
        for n in range(N):
            assert list(gp[n, :gc[n]]) == list(op[n, :oc[n]]), (seed, r, n)
        rel = np.abs(gw - ow) / np.maximum(np.abs(ow), 1e-300)
        assert np.all((gw == ow) | (rel <= RTOL)), (seed, r)


def test_fsx_407_many_chains_under_a_pcv(gpu_ctx, other_ctx):
    """More chains than CUs, fewer targets than slots: 300 chains on the .fsx:407 set."""
    seqs, codes, offsets = fsx_set()
    alpha, W, M, R = b"ATGC-", 6, 2, 300
    pcv = pcv49(alpha, 407)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    seeds = [7000 + 3 * r for r in range(R)]
    out = gpu_ctx.motif_sampling_multi_batch(M, W, PC, CUTOFF, seeds, pcv=pcv)
    assert not out[4].any()
    other_ctx.set_fixed_pcv(pcv)
    try:
        for r, seed in enumerate(seeds):
            check_sequential(row(out, r), other_ctx.motif_sampling_multi(M, W, PC, CUTOFF, seed),
                             (seed, r))
    finally:
        other_ctx.set_fixed_pcv(None)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_batch_equals_the_sequential_entry_point(name, kind, other_ctx):
    alpha, N, L, W, M, mode, dseed = SHAPES[name]
    codes, offsets = make_dataset(N, L, W, alpha, seed=dseed, ragged=True, mut=0.1)
    pcv = pcv49(alpha, dseed) if kind in ("pcv", "both") else None
    ppm = ppm49(W, dseed + 1) if kind in ("ppm", "both") else None
    outs = []
    for batch_starts in (0, 1):
        ctx = fresh({"batch_starts": batch_starts})
        ctx.set_sequences(codes, offsets, alpha)
        outs.append(ctx.motif_sampling_multi_batch(M, W, PC, CUTOFF, SEEDS, mode, pcv=pcv, ppm=ppm))
        ctx.close()
        assert not outs[-1][4].any()
    other_ctx.set_sequences(codes, offsets, alpha)
    set_fixed(other_ctx, pcv, ppm, W)
    try:
        for r, seed in enumerate(SEEDS):
            s = other_ctx.motif_sampling_multi(M, W, PC, CUTOFF, seed, init_mode=mode)
            for out in outs:  # both ways of making the starts
                check_sequential(row(out, r), s, (name, kind, seed, r))
    finally:
        set_fixed(other_ctx, None, None, W)
    check_sequential(row(outs[0], 1), row(outs[0], 3), "the duplicate seed")


def test_last_ms_and_info_report_the_fixed_call(gpu_ctx):
    seqs, codes, offsets = fsx_set()
    gpu_ctx.set_sequences(codes, offsets, b"ATGC-")
    gpu_ctx.motif_sampling_multi_batch(2, 6, PC, CUTOFF, SEEDS, pcv=pcv49(b"ATGC-", 407))
    ms = gpu_ctx.multi_batch_last_ms()
    assert len(ms) == 3 and all(np.isfinite(m) and m > 0.0 for m in ms)
    assert gpu_ctx.multi_batch_last_info()["slots"] >= 1


@pytest.mark.parametrize("reps", [3, 0])
def test_mirror_get_best_pwmss_of_ppm_amount_two(reps):
    from gibbssampling_amd import MotifSampler
    N, L, W, seed = 30, 50, 6, 99
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = sources_of(codes, offsets)
    ppm = ppm49(W, 6)
    loop = MotifSampler.getBestPWMSsOfPPM(reps, 2, W, PC, CUTOFF, "ACGT", sources, ppm, seed=seed)
    batch = MotifSampler.getBestPWMSsOfPPM(reps, 2, W, PC, CUTOFF, "ACGT", sources, ppm, seed=seed,
                                           batch=True)
    assert [list(m.Positions) for m in batch] == [list(m.Positions) for m in loop]
    assert all(a.PWMS == b.PWMS or abs(a.PWMS - b.PWMS) <= RTOL * abs(b.PWMS)
               for a, b in zip(batch, loop))
    assert len(batch) == (N if reps else 1)
