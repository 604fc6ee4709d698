"""The one-iteration path's dependent chain (gs_sweep_kernel<WM, 2, GL, 4, true>, DESIGN.md
§9.24) against the loop path, whose code that section left as it was.  Shipped: the
prologue's error vote through one barrier.  Measured with these tests and left out: the
quad scan's table reads issued half a trip ahead, and the own segment's symbols loaded from
global memory with the first loads; the shapes that those two can break stay here for
whoever takes them up again.

Every case runs the same 3-sweep chain with sweep_one = 0 and sweep_one = 1 (bg_mode 0: every
sweep is the sweep kernel's) and requires identical positions, PWMS bytes, aggregates and
fallback statistics.  The shapes are those at which the vote, the scan and the hold-one-out
block take another path:

- N = 1, 5, 17, 65: at 17 the second workgroup has three wavefronts without a sequence,
  which still vote and flush; 65 gives several workgroups.
- L = 12, 75, 76, 139, 203, 204, 256 at W = 12 (16 lanes a sequence): a lane's block is
  R = 4, 4, 8, 8, 12, 16, 16 windows, one to four trips of the scan on both sides of every
  ceil(K / 16) boundary; ragged lengths down to L = W make the wavefront's trip count exceed
  a group's own.
- W = 4 (one code dword and one), W = 32 at L = 32 and 256 (two columns a lane), W = 12 at
  Lmax = 257 and 900 (32 and 64 lanes a sequence: no quad scan).
- starts: all -1, all placed, mixed, every target at 0, every target at L - W (the own
  segment's last byte is the sequence's, and for the last sequence the array's).
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


def starts(offsets, W, kind, seed):
    rng = np.random.default_rng(seed)
    lens = np.diff(offsets)
    pos = (rng.random(len(lens)) * (lens - W + 1)).astype(np.int32)
    if kind == "none":
        pos[:] = -1
    elif kind == "mixed":   # (the first two of each kind whatever the draw)
        pos[rng.random(len(lens)) < 0.4] = -1
        pos[0] = -1
        if len(pos) > 1 and pos[1] < 0:
            pos[1] = 0
    elif kind == "zero":
        pos[:] = 0
    elif kind == "last":
        pos[:] = (lens - W).astype(np.int32)
    else:
        assert kind == "placed"
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


def both_paths(ctx_pair, N, L, W, ragged, kind, given=False, shard=(0, 0), oracle=False):
    extra, goff = shard
    seed = 3000 + 17 * N + 3 * L + W + (1 if ragged else 0)
    codes, offsets = dataset(N, L, W, ragged, seed)
    pos = starts(offsets, W, kind, seed + 1)
    out = []
    for c in ctx_pair:
        c.set_sequences(codes, offsets, ALPHA, n_global=N + extra + goff, global_offset=goff)
        out.append(chain(c, W, pos, seed + 2, given, goff))
    l0, l1 = out[0][4], out[1][4]
    assert l0["ek"] == 4 and l0["one"] == 0 and l0["gl"] == lanes(L), l0
    assert l1["ek"] == 4 and l1["one"] == 1 and l1["gl"] == lanes(L), l1
    same_run(out[0], out[1], (N, L, W, ragged, kind))
    if oracle:
        op, ow = oracle_chain(codes, offsets, W, pos, seed + 2, goff)
        same_as_oracle(out[1][0], out[1][1], op, ow, "one-iteration chain")


KINDS = ("none", "placed", "mixed", "zero", "last")
SCAN_L = (12, 75, 76, 139, 203, 204, 256)


@pytest.mark.parametrize("N", [1, 5, 17, 65])
@pytest.mark.parametrize("L", SCAN_L)
def test_scan_trips_equal_lengths(ctx_pair, N, L):
    """One to four trips of the quad scan, every group the same R; the starts rotate
    through the five kinds over the cases."""
    kind = KINDS[(SCAN_L.index(L) + N) % len(KINDS)]
    both_paths(ctx_pair, N, L, 12, False, kind)


@pytest.mark.parametrize("N", [5, 17, 65])
@pytest.mark.parametrize("L", [75, 76, 139, 204, 256])
def test_scan_trips_ragged_lengths(ctx_pair, N, L):
    """Lengths from W to L in one wavefront: the trip count is the longest group's, and
    the groups past their own R take windows that add nothing."""
    kind = KINDS[(L + N) % len(KINDS)]
    both_paths(ctx_pair, N, L, 12, True, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,L,ragged", [(17, 76, False), (65, 256, True), (17, 12, False)])
def test_starts(ctx_pair, N, L, ragged, kind):
    """Every kind of start at two to four trips, and at L = W where 0 = L - W is the only
    position: the own segment's bytes at a sequence's first and last positions."""
    both_paths(ctx_pair, N, L, 12, ragged, kind)


# N, L, W, ragged, starts, uniforms given, (n_global - n_local, global_offset), oracle too
WIDTH_CASES = [
    (5, 60, 4, False, "last", False, (0, 0), True),       # W = 4: one code dword and one
    (17, 200, 4, True, "mixed", True, (0, 0), False),
    (65, 4, 4, False, "zero", False, (0, 0), False),      # L = W = 4
    (5, 32, 32, False, "last", False, (0, 0), True),      # W = 32: two columns a lane, L = W
    (17, 32, 32, False, "mixed", True, (0, 0), False),
    (5, 256, 32, False, "last", False, (0, 0), False),
    (17, 256, 32, True, "placed", False, (0, 0), True),
    (65, 256, 32, True, "mixed", True, (7, 5), False),
    (5, 257, 12, False, "last", False, (0, 0), True),     # 32 lanes a sequence
    (17, 257, 12, True, "mixed", True, (0, 0), False),
    (65, 257, 12, True, "zero", False, (0, 0), False),
    (5, 900, 12, True, "last", False, (0, 0), False),     # 64 lanes a sequence
    (17, 900, 12, False, "mixed", False, (0, 0), True),
    (65, 900, 12, True, "placed", True, (0, 0), False),
    (17, 76, 12, True, "last", True, (0, 0), True),       # given uniforms, the array's last byte
    (17, 204, 12, False, "mixed", False, (40, 9), False),  # a shard
    (65, 139, 12, True, "last", True, (100, 64), False),
]


@pytest.mark.parametrize("N,L,W,ragged,kind,given,shard,oracle", WIDTH_CASES)
def test_widths_lanes_uniforms_shards(ctx_pair, N, L, W, ragged, kind, given, shard, oracle):
    both_paths(ctx_pair, N, L, W, ragged, kind, given, shard, oracle)


@pytest.mark.parametrize("N", [8, 65])
def test_sticky_error_vote(ctx_pair, N):
    """The overrun input of test_gpu_sweep_one.py's sticky-error test (u = 2 for sequence 7)
    in one workgroup and in five: the same status and index on both paths, which stay until
    a new snapshot is set; the sweep after that is a clean one on both."""
    from gibbssampling_amd import RouletteOverrunError
    L, W = 40, 8
    codes, offsets = dataset(N, L, W, False, 51 + N)
    pos = starts(offsets, W, "placed", 52 + N)
    u = np.random.default_rng(53 + N).random(N)
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
    out = [c.motif_sweep(W, PC, CUT, pos, u) for c in ctx_pair]
    assert ctx_pair[0].last_sweep_launch()["one"] == 0
    assert ctx_pair[1].last_sweep_launch()["one"] == 1
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()
    op, ow, _ = ol.sweep(ol.Seqs(codes, offsets, ALPHA), W, PC, CUT, pos, u)
    same_as_oracle(out[1][0], out[1][1], op, ow, "sweep after the cleared error")
