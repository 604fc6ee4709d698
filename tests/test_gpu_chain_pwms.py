"""PWMS after a chain are those of its last sweep (include/gibbs_hip.h gs_run_sweeps).
gs_sweep_kernel skips the picked windows' exact folds on the sweeps of a chain whose
PWMS the next sweep overwrites unread; the state a caller can read is unchanged: a
3-sweep chain equals three 1-sweep chains bit for bit (positions and PWMS) and the
oracle's chain (positions identical, PWMS within 1e-12), an empty chain call keeps the
PWMS, and a synchronous sweep after a chain returns its own.  Ragged DNA (the
four-symbol kernel: results stored a batch at a time) and protein (more than 16
symbols: stored as each pick is made).  The fold's recheck (gs_stats rescan_recheck)
never fires.
"""
import numpy as np
import pytest

from conftest import make_dataset, uniforms
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

RTOL = 1e-12
PC, CUTOFF, SEED = 1e-4, 1.0, 97
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
DATA = {"dna": (200, 200, 12, b"ACGT", 801), "protein": (150, 200, 20, PROTEIN, 802)}


def same(gpos, gpw, opos, opw, what=""):
    bad = np.nonzero(gpos != opos)[0]
    assert bad.size == 0, f"{what}: {bad.size} positions differ, first {bad[:8]}"
    fin = np.isfinite(opw)
    assert np.array_equal(np.isfinite(gpw), fin), what
    rel = np.abs(gpw[fin] - opw[fin]) / np.maximum(np.abs(opw[fin]), 1e-300)
    assert rel.size == 0 or rel.max() <= RTOL, f"{what}: PWMS rel diff {rel.max():.3e}"


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


_REF = {}


def reference(kind):
    """The input and the oracle's chain after 1, 2 and 3 sweeps, computed once."""
    if kind not in _REF:
        N, L, W, alpha, seed = DATA[kind]
        codes, offsets = make_dataset(N, L, W, alpha, seed=seed, ragged=True)
        S = ol.Seqs(codes, offsets, alpha)
        pos = ol.random_starts(S, W, PC, seed=5, mode=1)[1].astype(np.int32)
        chain, p = [], pos
        for t in range(3):
            p, w, _ = ol.sweep(S, W, PC, CUTOFF, p, uniforms(SEED, ol.stream_sweep(t), N))
            p.setflags(write=False)
            w.setflags(write=False)
            chain.append((p, w))
        _REF[kind] = (codes, offsets, alpha, W, pos, chain)
    return _REF[kind]


@pytest.fixture(params=sorted(DATA))
def chain_ctx(request, gpu_ctx):
    codes, offsets, alpha, W, pos, chain = reference(request.param)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    assert gpu_ctx.sweep_kernel_name() == "gs_sweep_kernel"
    before = gpu_ctx.stats()["rescan_recheck"]
    yield gpu_ctx, W, pos, chain, request.param
    assert gpu_ctx.stats()["rescan_recheck"] == before == 0


def test_chain_equals_single_sweep_calls(chain_ctx):
    ctx, W, pos, chain, kind = chain_ctx
    ctx.set_positions(W, pos)
    ctx.run_sweeps(PC, CUTOFF, 3, seed=SEED, first_sweep=0)
    cpos, cpw = ctx.get_state()
    ctx.set_positions(W, pos)
    for t in range(3):
        ctx.run_sweeps(PC, CUTOFF, 1, seed=SEED, first_sweep=t)
        spos, spw = ctx.get_state()
        same(spos, spw, chain[t][0], chain[t][1], f"{kind}: single sweep {t}")
    assert np.array_equal(cpos, spos), kind
    assert np.array_equal(bits(cpw), bits(spw)), f"{kind}: PWMS bits"
    same(cpos, cpw, chain[2][0], chain[2][1], f"{kind}: 3-sweep chain")
    launch = ctx.last_sweep_launch()
    assert launch["ek"] == (4 if kind == "dna" else 0), launch


def test_empty_chain_call_keeps_pwms(chain_ctx):
    ctx, W, pos, chain, kind = chain_ctx
    ctx.set_positions(W, pos)
    ctx.run_sweeps(PC, CUTOFF, 2, seed=SEED, first_sweep=0)
    ctx.run_sweeps(PC, CUTOFF, 0, seed=SEED, first_sweep=2)
    gpos, gpw = ctx.get_state()
    same(gpos, gpw, chain[1][0], chain[1][1], f"{kind}: 2 sweeps, then none")
    # and bit for bit the PWMS of the second of two single sweeps
    ctx.set_positions(W, pos)
    ctx.run_sweeps(PC, CUTOFF, 1, seed=SEED, first_sweep=0)
    ctx.run_sweeps(PC, CUTOFF, 1, seed=SEED, first_sweep=1)
    spos, spw = ctx.get_state()
    assert np.array_equal(gpos, spos) and np.array_equal(bits(gpw), bits(spw)), kind


def test_motif_sweep_after_chain_returns_its_own_pwms(chain_ctx):
    ctx, W, pos, chain, kind = chain_ctx
    ctx.set_positions(W, pos)
    ctx.run_sweeps(PC, CUTOFF, 3, seed=SEED, first_sweep=0)
    u = uniforms(SEED, ol.stream_sweep(1), len(pos))
    gpos, gpw = ctx.motif_sweep(W, PC, CUTOFF, chain[0][0], u)
    same(gpos, gpw, chain[1][0], chain[1][1], f"{kind}: a sweep after a chain")
