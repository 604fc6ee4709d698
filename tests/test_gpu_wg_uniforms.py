"""The uniforms of the four-symbol kernel's one-iteration path (gs_sweep.hip ONE, DESIGN.md
§9.16, §9.20): with no uniforms given (gs_run_sweeps) the kernel evaluates the counter RNG
itself, and what it draws for sequence n of sweep f + t must be gs_uniform(seed,
stream_sweep(f + t), global_offset + n), wherever in a workgroup the draw is done.

The chains below are compared with as many motif_sweep calls fed those values from the host
(which take the same path with the uniforms given), with the loop path (sweep_one 0, which
draws 64 a pass) and with the oracle.  The sizes are those at which a draw shared by a
workgroup's wavefronts (§9.20's lever A, measured and not shipped) could go wrong: one
workgroup holds 4 wavefronts of 64 / GL groups, 16 sequences at Lmax <= 256, 8 up to 512,
4 beyond; N = 2 leaves the third and fourth wavefront without a sequence, N = 17 and 21
fill a second workgroup partly, N = 33 a third.  The all-background takeover is off
(bg_mode 0): every sweep is gs_sweep_kernel's.
"""
import numpy as np
import pytest

from conftest import uniforms
from gibbssampling_amd import _native
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

ALPHA = b"ACGT"
PC, CUT = 1e-4, 1.0
RTOL = 1e-12
T = 3
STATS = ("exact_rescans", "serial_picks", "desc_oob")


def dataset(N, L, W, ragged, seed, mut=0.1):
    """N sequences over ACGT with a mutated consensus W-mer planted in each; ragged:
    lengths in [W, L], the first one L (Lmax = L decides the lanes a sequence)."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(ALPHA, np.uint8)
    lens = rng.integers(W, L + 1, N) if ragged else np.full(N, L)
    lens[0] = L
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


def starts(offsets, W, seed):
    """Random positions, 30 % of them -1, the first placed."""
    rng = np.random.default_rng(seed)
    lens = np.diff(offsets)
    pos = (rng.random(len(lens)) * (lens - W + 1)).astype(np.int32)
    pos[rng.random(len(lens)) < 0.3] = -1
    pos[0] = max(pos[0], 0)
    return pos


@pytest.fixture(scope="module")
def ctx_pair():
    """(loop path, one-iteration path) of the four-symbol kernel."""
    from gibbssampling_amd import Context
    c0 = Context(0, tuning={"sweep_one": 0.0, "bg_mode": 0.0})
    c1 = Context(0, tuning={"sweep_one": 1.0, "bg_mode": 0.0})
    yield c0, c1
    c0.close()
    c1.close()


def host_uniforms(seed, sweep, first, n):
    """gs_uniform(seed, stream_sweep(sweep), first + i), i < n, by the library's own
    host function, one call a value."""
    st = _native.stream_sweep(sweep)
    return np.array([_native.uniform(seed, st, first + i) for i in range(n)], np.float64)


def drawn_chain(c, W, pos, seed, f):
    """T sweeps whose uniforms the kernel draws."""
    s0 = c.stats()
    c.set_positions(W, pos)
    c.run_sweeps(PC, CUT, T, seed, first_sweep=f)
    p, w = c.get_state()
    s1 = c.stats()
    return p, w, c.agg_download(), {k: s1[k] - s0[k] for k in STATS}, c.last_sweep_launch()


def given_chain(c, W, pos, seed, f, goff):
    """The same T sweeps as single calls with the host's uniforms."""
    p, w = np.asarray(pos, np.int32), None
    for t in range(T):
        p, w = c.motif_sweep(W, PC, CUT, p, host_uniforms(seed, f + t, goff, len(p)))
    return p, w, c.agg_download(), c.last_sweep_launch()


def oracle_chain(codes, offsets, W, pos, seed, f=0):
    S = ol.Seqs(codes, offsets, ALPHA)
    p, w = pos, None
    for t in range(T):
        p, w, _ = ol.sweep(S, W, PC, CUT, p, uniforms(seed, ol.stream_sweep(f + t), len(pos)), threads=8)
    return p, w


def same_as_oracle(gp, gw, op, ow, what):
    assert np.array_equal(gp, op), f"{what}: positions differ at {np.nonzero(gp != op)[0][:8]}"
    fin = np.isfinite(ow)
    assert np.array_equal(np.isfinite(gw), fin), what
    rel = np.abs(gw[fin] - ow[fin]) / np.maximum(np.abs(ow[fin]), 1e-300)
    assert rel.size == 0 or rel.max() <= RTOL, f"{what}: PWMS rel diff {rel.max():.3e}"


def lanes(L):
    return 16 if L <= 256 else 32 if L <= 512 else 64


# N, L, W, ragged, first sweep, (n_global - n_local, global_offset)
CASES = [
    (1, 60, 12, False, 0, (0, 0)),
    (2, 60, 12, True, 7, (0, 0)),       # two wavefronts have no sequence
    (2, 60, 12, False, 0, (40, 9)),
    (3, 60, 12, True, 0, (0, 0)),
    (5, 60, 12, False, 7, (11, 3)),
    (16, 60, 12, True, 0, (0, 0)),      # one full workgroup
    (17, 60, 12, True, 7, (0, 0)),      # a second workgroup, partly filled
    (21, 200, 12, False, 0, (100, 64)),  # equal lengths: the fixed-stride descriptors
    (33, 60, 12, True, 0, (5, 1000)),   # three workgroups
    (5, 256, 12, True, 0, (0, 0)),      # 16 lanes a sequence, the longest
    (5, 257, 12, True, 7, (3, 2)),      # 32 lanes: 8 sequences a workgroup
    (9, 257, 12, False, 0, (0, 0)),     # ... two workgroups
    (3, 900, 12, True, 0, (0, 0)),      # 64 lanes: 4 sequences a workgroup
    (5, 900, 12, True, 7, (7, 5)),      # ... two workgroups
]


@pytest.mark.parametrize("N,L,W,ragged,f,shard", CASES)
def test_drawn_uniforms_are_the_hosts(ctx_pair, N, L, W, ragged, f, shard):
    """Positions, PWMS bits and aggregates of a drawn chain equal those of the same sweeps
    with the host's uniforms given, and those of the loop path, fallback counts included."""
    c0, c1 = ctx_pair
    extra, goff = shard
    seed = 500 + 11 * N + L + f
    codes, offsets = dataset(N, L, W, ragged, seed)
    pos = starts(offsets, W, seed + 1)
    out = []
    for c in (c0, c1):
        c.set_sequences(codes, offsets, ALPHA, n_global=N + extra + goff, global_offset=goff)
        out.append(drawn_chain(c, W, pos, seed + 2, f))
    (p0, w0, a0, s0, l0), (p1, w1, a1, s1, l1) = out
    assert l0["ek"] == 4 and l0["one"] == 0 and l0["gl"] == lanes(L), l0
    assert l1["ek"] == 4 and l1["one"] == 1 and l1["gl"] == lanes(L), l1
    assert l1["grid"] == -(-N // (4 * (64 // lanes(L)))), l1
    gp, gw, ga, gl = given_chain(c1, W, pos, seed + 2, f, goff)
    assert gl["one"] == 1, gl
    assert np.array_equal(p1, gp), np.nonzero(p1 != gp)[0][:8]
    assert w1.tobytes() == gw.tobytes()
    assert a1.tobytes() == ga.tobytes()
    assert np.array_equal(p0, p1), np.nonzero(p0 != p1)[0][:8]
    assert w0.tobytes() == w1.tobytes()
    assert a0.tobytes() == a1.tobytes()
    assert s0 == s1 and s1["desc_oob"] == 0, (s0, s1)


def test_ragged_chain_matches_oracle(ctx_pair):
    _, c1 = ctx_pair
    N, L, W, f = 21, 120, 12, 7
    codes, offsets = dataset(N, L, W, True, 301)
    pos = starts(offsets, W, 302)
    c1.set_sequences(codes, offsets, ALPHA)
    p, w, _, st, launch = drawn_chain(c1, W, pos, 303, f)
    assert launch["one"] == 1 and launch["grid"] == 2, launch
    op, ow = oracle_chain(codes, offsets, W, pos, 303, f)
    same_as_oracle(p, w, op, ow, "drawn ragged chain")
    assert st["desc_oob"] == 0


def test_dispatch_boundary_matches_oracle():
    """One workgroup a CU (blocks_per_cu_cap 1): 16 n_cu sequences of 16 lanes are the most
    the path takes, one more goes to the loop path; both chains are the oracle's."""
    import torch
    from gibbssampling_amd import Context
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    L, W = 24, 12
    N = 16 * n_cu
    codes, offsets = dataset(N + 1, L, W, False, 311)
    pos = starts(offsets, W, 312)
    c = Context(0, tuning={"blocks_per_cu_cap": 1.0, "bg_mode": 0.0})
    try:
        for n, one in ((N, 1), (N + 1, 0)):
            c.set_sequences(codes[:n * L], offsets[:n + 1], ALPHA)
            p, w, _, st, launch = drawn_chain(c, W, pos[:n], 313, 0)
            assert launch["ek"] == 4 and launch["grid"] == n_cu and launch["one"] == one, launch
            op, ow = oracle_chain(codes[:n * L], offsets[:n + 1], W, pos[:n], 313)
            same_as_oracle(p, w, op, ow, f"N = {n}, one = {one}")
            assert st["desc_oob"] == 0
    finally:
        c.close()


def test_given_uniforms_unchanged(ctx_pair):
    """Uniforms of the caller's (not the counter RNG's) through both paths: equal, and
    the oracle's."""
    N, L, W = 17, 90, 12
    codes, offsets = dataset(N, L, W, True, 321)
    pos = starts(offsets, W, 322)
    us = np.random.default_rng(323).random((T, N))
    out = []
    for c, one in zip(ctx_pair, (0, 1)):
        c.set_sequences(codes, offsets, ALPHA)
        p, w = pos, None
        for t in range(T):
            p, w = c.motif_sweep(W, PC, CUT, p, us[t])
        assert c.last_sweep_launch()["one"] == one
        out.append((p, w, c.agg_download()))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2].tobytes() == out[1][2].tobytes()
    S = ol.Seqs(codes, offsets, ALPHA)
    op, ow = pos, None
    for t in range(T):
        op, ow, _ = ol.sweep(S, W, PC, CUT, op, us[t], threads=8)
    same_as_oracle(out[1][0], out[1][1], op, ow, "given uniforms")
