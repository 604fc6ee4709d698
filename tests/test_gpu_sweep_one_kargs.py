"""The arguments of the four-symbol kernel's one-iteration entry (gs_sweep.hip SweepOneKargs,
DESIGN.md §9.22): what the addresses of the prologue's first loads need reaches that entry
as leading kernel parameters (aggregate replicas and their stride, pair codes, positions,
compositions, the grid and the wavefronts a workgroup, the slot ranges' quotient and
remainder, the fixed sequence stride, Lmax), built by gs_sweep_launch beside the SweepArgs
the loop path's entry takes alone.  A wrong leading argument shows as another result than
the loop path's, whose entry is unchanged: every case runs the same 3-sweep chain with
sweep_one 0 and sweep_one 1 and requires identical positions, PWMS bits, aggregates and
fallback counters.

N = 1, 3, 5, 17, 65 give a remainder of the slot ranges, short last wavefronts and
workgroups whose drawing wavefront has no sequence; equal lengths take the fixed stride,
ragged ones the descriptors, down to L = W; W = 4, 12, 32 at 16 lanes a sequence, W = 12
at Lmax = 257 and 900 (32 and 64 lanes); uniforms drawn by the kernel or given by the
caller; shards (global_offset > 0, n_global > n_local).  The all-background takeover is
off (bg_mode 0): every sweep is gs_sweep_kernel's.
"""
import numpy as np
import pytest

from conftest import uniforms
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

ALPHA = b"ACGT"
PC, CUT = 1e-4, 1.0
RTOL = 1e-12
T = 3
STATS = ("exact_rescans", "serial_picks", "desc_oob")


def dataset(N, L, W, ragged, seed, mut=0.1):
    """N sequences over ACGT with a mutated consensus W-mer planted in each; ragged:
    lengths in [W, L], the first one L (Lmax = L decides the lanes a sequence) and, from
    two sequences on, the last one W (a single window)."""
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


def starts(offsets, W, seed):
    """Random positions, 30 % of them -1, the first placed."""
    rng = np.random.default_rng(seed)
    lens = np.diff(offsets)
    pos = (rng.random(len(lens)) * (lens - W + 1)).astype(np.int32)
    pos[rng.random(len(lens)) < 0.3] = -1
    pos[0] = max(pos[0], 0)
    return pos


def lanes(L):
    return 16 if L <= 256 else 32 if L <= 512 else 64


@pytest.fixture(scope="module")
def ctx_pair():
    """(loop path, one-iteration path) of the four-symbol kernel."""
    from gibbssampling_amd import Context
    c0 = Context(0, tuning={"sweep_one": 0.0, "bg_mode": 0.0})
    c1 = Context(0, tuning={"sweep_one": 1.0, "bg_mode": 0.0})
    yield c0, c1
    c0.close()
    c1.close()


def chain(c, W, pos, seed, given, goff, sweeps=T):
    """`sweeps` sweeps from the snapshot `pos`: one gs_run_sweeps call whose uniforms the
    kernel draws, or (given) as many gs_motif_sweep calls with the same values from the
    host.  Returns positions, PWMS, aggregates, the fallback counters and the launch."""
    s0 = c.stats()
    if given:
        p, w = np.asarray(pos, np.int32), None
        for t in range(sweeps):
            p, w = c.motif_sweep(W, PC, CUT, p, uniforms(seed, ol.stream_sweep(t), len(p), first=goff))
    else:
        c.set_positions(W, pos)
        c.run_sweeps(PC, CUT, sweeps, seed)
        p, w = c.get_state()
    s1 = c.stats()
    return p, w, c.agg_download(), {k: s1[k] - s0[k] for k in STATS}, c.last_sweep_launch()


def oracle_chain(codes, offsets, W, pos, seed, goff, sweeps=T):
    """The shard's own chain: its sequences alone, sequence n's uniform the one of the
    whole sampler's sequence goff + n."""
    S = ol.Seqs(codes, offsets, ALPHA)
    p, w = pos, None
    for t in range(sweeps):
        p, w, _ = ol.sweep(S, W, PC, CUT, p, uniforms(seed, ol.stream_sweep(t), len(pos), first=goff),
                           threads=8)
    return p, w


def same_as_oracle(gp, gw, op, ow, what):
    assert np.array_equal(gp, op), f"{what}: positions differ at {np.nonzero(gp != op)[0][:8]}"
    fin = np.isfinite(ow)
    assert np.array_equal(np.isfinite(gw), fin), what
    rel = np.abs(gw[fin] - ow[fin]) / np.maximum(np.abs(ow[fin]), 1e-300)
    assert rel.size == 0 or rel.max() <= RTOL, f"{what}: PWMS rel diff {rel.max():.3e}"


def same_run(r0, r1, what=""):
    (p0, w0, a0, s0, _), (p1, w1, a1, s1, _) = r0, r1
    assert np.array_equal(p0, p1), (what, np.nonzero(p0 != p1)[0][:8])
    assert w0.tobytes() == w1.tobytes(), what
    assert a0.tobytes() == a1.tobytes(), what
    assert s0 == s1 and s1["desc_oob"] == 0, (what, s0, s1)


# N, L, W, ragged, uniforms given, (n_global - n_local, global_offset), oracle too
CASES = [
    (1, 40, 12, False, False, (0, 0), False),
    (1, 12, 12, True, True, (0, 0), False),       # L = W: one window
    (3, 60, 4, True, False, (0, 0), True),        # ragged: the descriptors
    (3, 60, 12, False, True, (0, 0), True),       # given uniforms
    (3, 900, 12, False, True, (0, 0), False),     # 64 lanes: 4 sequences a workgroup
    (5, 32, 32, False, False, (0, 0), True),      # equal lengths, L = W at the widest motif
    (5, 256, 32, True, True, (0, 0), False),      # the longest sequence of 16-lane groups
    (5, 60, 12, False, False, (11, 3), True),     # a shard
    (17, 60, 12, False, False, (0, 0), False),    # a second workgroup, partly filled
    (17, 60, 12, True, True, (40, 9), False),
    (17, 12, 12, False, False, (0, 0), False),    # L = W, equal lengths: K = 1
    (17, 257, 12, True, False, (0, 0), True),     # 32 lanes: 8 sequences a workgroup
    (17, 257, 12, False, True, (0, 0), False),
    (17, 900, 12, False, False, (5, 1000), False),
    (65, 60, 12, False, False, (0, 0), False),    # five workgroups: wq 3, wr 5
    (65, 60, 12, True, True, (3, 2), False),
    (65, 200, 4, False, True, (0, 0), False),
    (65, 257, 12, False, False, (100, 64), False),  # nine workgroups of 32 lanes
    (65, 900, 12, True, False, (0, 0), True),     # seventeen of 64 lanes
]


@pytest.mark.parametrize("N,L,W,ragged,given,shard,oracle", CASES)
def test_leading_arguments_equal_loop_path(ctx_pair, N, L, W, ragged, given, shard, oracle):
    extra, goff = shard
    seed = 2000 + 13 * N + L + W
    codes, offsets = dataset(N, L, W, ragged, seed)
    pos = starts(offsets, W, seed + 1)
    out = []
    for c in ctx_pair:
        c.set_sequences(codes, offsets, ALPHA, n_global=N + extra + goff, global_offset=goff)
        out.append(chain(c, W, pos, seed + 2, given, goff))
    l0, l1 = out[0][4], out[1][4]
    assert l0["ek"] == 4 and l0["one"] == 0 and l0["gl"] == lanes(L), l0
    assert l1["ek"] == 4 and l1["one"] == 1 and l1["gl"] == lanes(L), l1
    assert l1["grid"] == -(-N // (4 * (64 // lanes(L)))), l1
    same_run(out[0], out[1])
    if oracle:
        op, ow = oracle_chain(codes, offsets, W, pos, seed + 2, goff)
        same_as_oracle(out[1][0], out[1][1], op, ow, "one-iteration chain")


def test_shard_draws_the_whole_samplers_uniforms(ctx_pair):
    """A shard's drawn chain is the chain of single sweeps given the whole sampler's
    uniforms of its sequences (index global_offset + n), on the one-iteration path."""
    _, c1 = ctx_pair
    N, L, W, extra, goff = 21, 200, 12, 100, 64
    codes, offsets = dataset(N, L, W, False, 401)
    pos = starts(offsets, W, 402)
    c1.set_sequences(codes, offsets, ALPHA, n_global=N + extra + goff, global_offset=goff)
    drawn = chain(c1, W, pos, 403, False, goff)
    given = chain(c1, W, pos, 403, True, goff)
    assert drawn[4]["one"] == 1 and given[4]["one"] == 1
    same_run(drawn, given)


@pytest.mark.parametrize("N,L,ragged", [(5, 60, False), (17, 60, True), (65, 257, False)])
def test_first_sweep_after_set_positions(ctx_pair, N, L, ragged):
    """One sweep from a fresh snapshot: the replicas it reads are those the snapshot's
    aggregate launch wrote, their pointer and stride the leading arguments'."""
    W = 12
    codes, offsets = dataset(N, L, W, ragged, 411 + N)
    pos = starts(offsets, W, 412 + N)
    out = []
    for c in ctx_pair:
        c.set_sequences(codes, offsets, ALPHA)
        out.append(chain(c, W, pos, 413, False, 0, sweeps=1))
    assert out[0][4]["one"] == 0 and out[1][4]["one"] == 1
    same_run(out[0], out[1])
    op, ow = oracle_chain(codes, offsets, W, pos, 413, 0, sweeps=1)
    same_as_oracle(out[1][0], out[1][1], op, ow, "first sweep")


def test_timed_launch_form_equals_plain(ctx_pair):
    """With every launch timed the sweep goes through hipExtLaunchKernel with events: the
    same parameters, the same chain."""
    _, c1 = ctx_pair
    N, L, W = 17, 60, 12
    codes, offsets = dataset(N, L, W, True, 421)
    pos = starts(offsets, W, 422)
    c1.set_sequences(codes, offsets, ALPHA)
    plain = chain(c1, W, pos, 423, False, 0)
    c1.profile(True)
    try:
        timed = chain(c1, W, pos, 423, False, 0)
        c1.synchronize()
        _, nk, _, _ = c1.profile_read()
    finally:
        c1.profile(False)
    assert nk >= T and timed[4]["one"] == 1
    same_run(plain, timed)


def test_captured_chain_equals_eager(ctx_pair):
    """The chain replayed as a captured graph (graph_mode 1, captured ahead of time by
    gs_prepare_sweeps) records the plain launch form with the entry's parameters."""
    from gibbssampling_amd import Context
    _, c1 = ctx_pair
    N, L, W = 65, 60, 12
    codes, offsets = dataset(N, L, W, False, 431)
    pos = starts(offsets, W, 432)
    c1.set_sequences(codes, offsets, ALPHA)
    eager = chain(c1, W, pos, 433, False, 0)
    g = Context(0, tuning={"sweep_one": 1.0, "bg_mode": 0.0, "graph_mode": 1.0})
    try:
        g.set_sequences(codes, offsets, ALPHA)
        s0 = g.stats()
        g.set_positions(W, pos)
        g.prepare_sweeps(PC, CUT, 433)
        g.run_sweeps(PC, CUT, T, 433)
        p, w = g.get_state()
        s1 = g.stats()
        got = (p, w, g.agg_download(), {k: s1[k] - s0[k] for k in STATS}, g.last_sweep_launch())
    finally:
        g.close()
    assert got[4]["one"] == 1, got[4]
    same_run(eager, got)
