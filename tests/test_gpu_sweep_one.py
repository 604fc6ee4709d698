"""The four-symbol sweep kernel's one-iteration path (gs_sweep_kernel<WM, 2, GL, 4, true>,
tuning field sweep_one) against its loop path and the oracle.

The path is taken when no wavefront of the launch has more sequences than its 64 / GL
lane groups score at a time, which is every small launch: the equality cases below run
the same 3-sweep chain with sweep_one = 0 (the loop path, which they keep covered at
small shapes) and sweep_one = 1 and require identical positions, PWMS bits, aggregates and
fallback statistics.  The all-background takeover is off (bg_mode 0) so that every sweep
of every chain, also from starts without a motif, is the sweep kernel's.
"""
import numpy as np
import pytest

from conftest import uniforms
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

ALPHA = b"ACGT"
PC, CUT = 1e-4, 1.0
RTOL = 1e-12
STATS = ("exact_rescans", "serial_picks", "desc_oob")


def dataset(N, L, W, ragged, seed, mut=0.1):
    """N sequences over ACGT with a mutated consensus W-mer planted in each; ragged:
    lengths in [W, L] with the first L (so Lmax = L decides the lane groups) and, from
    two sequences on, the last W (a single window)."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(ALPHA, np.uint8)
    lens = rng.integers(W, L + 1, N) if ragged else np.full(N, L)
    if ragged:
        lens[0] = L
        if N > 1:
            lens[-1] = W
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    codes = a[rng.integers(0, 4, int(offsets[-1]))].astype(np.uint8)
    cons = a[rng.integers(0, 4, W)]
    for n in range(N):
        m = cons.copy()
        flip = rng.random(W) < mut
        m[flip] = a[rng.integers(0, 4, int(flip.sum()))]
        s = int(offsets[n]) + int(rng.random() * (lens[n] - W + 1))
        codes[s:s + W] = m
    return codes, offsets


def starts(offsets, W, kind, seed):
    rng = np.random.default_rng(seed)
    lens = np.diff(offsets)
    pos = (rng.random(len(lens)) * (lens - W + 1)).astype(np.int32)
    if kind == "none":      # every position -1
        pos[:] = -1
    elif kind == "mixed":   # (the first two of each kind whatever the draw)
        pos[rng.random(len(lens)) < 0.4] = -1
        pos[0] = -1
        if len(pos) > 1 and pos[1] < 0:
            pos[1] = 0
    return pos


@pytest.fixture(scope="module")
def ctx_pair():
    from gibbssampling_amd import Context
    c0 = Context(0, tuning={"sweep_one": 0.0, "bg_mode": 0.0})
    c1 = Context(0, tuning={"sweep_one": 1.0, "bg_mode": 0.0})
    yield c0, c1
    c0.close()
    c1.close()


def chain(c, codes, offsets, W, pos, seed, sweeps=3):
    c.set_sequences(codes, offsets, ALPHA)
    s0 = c.stats()
    c.set_positions(W, pos)
    c.run_sweeps(PC, CUT, sweeps, seed)
    p, w = c.get_state()
    s1 = c.stats()
    return p, w, c.agg_download(), {k: s1[k] - s0[k] for k in STATS}, c.last_sweep_launch()


def oracle_chain(codes, offsets, W, pos, seed, sweeps=3):
    S = ol.Seqs(codes, offsets, ALPHA)
    p, w = pos, None
    for t in range(sweeps):
        p, w, _ = ol.sweep(S, W, PC, CUT, p, uniforms(seed, ol.stream_sweep(t), len(pos)), threads=8)
    return p, w


def same_as_oracle(gp, gw, op, ow, what):
    assert np.array_equal(gp, op), f"{what}: positions differ at {np.nonzero(gp != op)[0][:8]}"
    fin = np.isfinite(ow)
    assert np.array_equal(np.isfinite(gw), fin), what
    rel = np.abs(gw[fin] - ow[fin]) / np.maximum(np.abs(ow[fin]), 1e-300)
    assert rel.size == 0 or rel.max() <= RTOL, f"{what}: PWMS rel diff {rel.max():.3e}"


# N (short last wavefronts, inactive groups), equal / ragged lengths (the fixed-stride
# and the descriptor loads), L = W (one window), Lmax = 256 | 257 (16 -> 32 lanes a
# sequence; 900: 64), W = 4, 12, 32, starts all -1 / all placed / mixed
CASES = [
    # N, L, W, ragged, starts
    (1, 40, 12, False, "mixed"),
    (1, 60, 12, True, "placed"),
    (3, 40, 12, True, "placed"),
    (3, 900, 4, True, "mixed"),
    (5, 60, 4, True, "mixed"),
    (5, 32, 32, False, "mixed"),      # L = W at the widest motif
    (5, 256, 32, False, "placed"),
    (5, 257, 32, True, "mixed"),
    (17, 60, 12, False, "none"),
    (17, 60, 12, True, "none"),
    (17, 12, 12, False, "placed"),    # L = W: K = 1
    (17, 200, 12, True, "mixed"),
    (17, 256, 12, True, "mixed"),     # the longest sequence of 16-lane groups
    (17, 257, 12, True, "mixed"),     # the shortest of 32-lane groups
    (17, 257, 4, False, "placed"),
]


@pytest.mark.parametrize("N,L,W,ragged,kind", CASES)
def test_one_iteration_path_equals_loop_path(ctx_pair, N, L, W, ragged, kind):
    c0, c1 = ctx_pair
    seed = 1000 + 7 * N + L + W
    codes, offsets = dataset(N, L, W, ragged, seed)
    pos = starts(offsets, W, kind, seed + 1)
    p0, w0, a0, s0, l0 = chain(c0, codes, offsets, W, pos, seed + 2)
    p1, w1, a1, s1, l1 = chain(c1, codes, offsets, W, pos, seed + 2)
    assert l0["ek"] == 4 and l0["one"] == 0, l0
    assert l1["ek"] == 4 and l1["one"] == 1, l1
    assert l0["gl"] == l1["gl"] == (16 if L <= 256 else 32 if L <= 512 else 64)
    assert np.array_equal(p0, p1), np.nonzero(p0 != p1)[0][:8]
    assert w0.tobytes() == w1.tobytes()
    assert a0.tobytes() == a1.tobytes()
    assert s0 == s1 and s1["desc_oob"] == 0, (s0, s1)


def test_one_iteration_path_matches_oracle(ctx_pair):
    _, c1 = ctx_pair
    N, L, W = 17, 60, 12
    codes, offsets = dataset(N, L, W, True, 77)
    pos = starts(offsets, W, "mixed", 78)
    p, w, _, st, launch = chain(c1, codes, offsets, W, pos, 79)
    assert launch["one"] == 1, launch
    op, ow = oracle_chain(codes, offsets, W, pos, 79)
    same_as_oracle(p, w, op, ow, "one-iteration chain")
    assert st["desc_oob"] == 0


def test_dispatch_boundary():
    """One workgroup a CU (blocks_per_cu_cap 1), 4 wavefronts of 4 groups: 16 n_cu
    sequences are the most one iteration holds.  Automatic dispatch takes the path there
    and the loop path one sequence further, where requiring it is GS_E_ARG and launches
    nothing; that loop-path chain is checked against the oracle."""
    import torch
    from gibbssampling_amd import ArgumentError, Context
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    L, W = 24, 12
    N = 4 * 4 * n_cu
    codes, offsets = dataset(N + 1, L, W, False, 91)
    pos = starts(offsets, W, "mixed", 92)
    c = Context(0, tuning={"blocks_per_cu_cap": 1.0, "bg_mode": 0.0})
    try:
        assert c.get_tuning("sweep_one") == -1.0
        _, _, _, _, launch = chain(c, codes[:N * L], offsets[:N + 1], W, pos[:N], 93, sweeps=1)
        assert launch["ek"] == 4 and launch["grid"] == n_cu and launch["one"] == 1, launch
        p, w, _, st, launch = chain(c, codes, offsets, W, pos, 93)
        assert launch["ek"] == 4 and launch["grid"] == n_cu and launch["one"] == 0, launch
        op, ow = oracle_chain(codes, offsets, W, pos, 93)
        same_as_oracle(p, w, op, ow, "loop path at N + 1")
        assert st["desc_oob"] == 0
        # required where a wavefront needs a second iteration: an argument error
        c.set_tuning("sweep_one", 1.0)
        c.set_positions(W, pos)
        with pytest.raises(ArgumentError) as ei:
            c.run_sweeps(PC, CUT, 3, 93)
        assert ei.value.status == 1
        c.set_tuning("sweep_one", -1.0)
        p2, w2, _, _, launch = chain(c, codes, offsets, W, pos, 93)
        assert launch["one"] == 0
        assert np.array_equal(p2, p) and w2.tobytes() == w.tobytes()
    finally:
        c.close()


def test_sticky_error_through_one_iteration_path(ctx_pair):
    """The overrun input of test_gpu_parity.py::test_overrun_raises (u = 2 for sequence
    7: the roulette wheel runs past its last category) at 8 sequences, with W = 8 instead
    of 6 -- the four-symbol kernel takes multiples of 4 -- through both paths: the same
    status and index, which stay (the device's error word is sticky: the next call that
    reads it reports them again; the failed snapshot is void, so no call sweeps it
    further) until a new snapshot is set; the sweep after that is a clean one."""
    from gibbssampling_amd import RouletteOverrunError
    N, L, W = 8, 40, 8
    codes, offsets = dataset(N, L, W, False, 51)
    pos = starts(offsets, W, "placed", 52)
    u = np.random.default_rng(53).random(N)
    bad = u.copy()
    bad[7] = 2.0
    seen = []
    for c in ctx_pair:
        c.set_sequences(codes, offsets, ALPHA)
        with pytest.raises(RouletteOverrunError) as ei:
            c.motif_sweep(W, PC, CUT, pos, bad)
        seen.append((ei.value.status, ei.value.index))
        with pytest.raises(RouletteOverrunError) as ei:  # still there
            c.synchronize()
        seen.append((ei.value.status, ei.value.index))
    assert seen == [(2, 7)] * 4, seen
    assert ctx_pair[1].last_sweep_launch()["one"] == 1
    # a new snapshot clears it
    out = [c.motif_sweep(W, PC, CUT, pos, u) for c in ctx_pair]
    assert ctx_pair[1].last_sweep_launch()["one"] == 1
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()
    op, ow, _ = ol.sweep(ol.Seqs(codes, offsets, ALPHA), W, PC, CUT, pos, u)
    same_as_oracle(out[1][0], out[1][1], op, ow, "sweep after the cleared error")
