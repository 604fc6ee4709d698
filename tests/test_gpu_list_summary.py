"""GPU parity of the list chain summaries: gs_list_occupancy_summary on
hand-made bins and site counts against a numpy restatement of the definition (the modal site
count, the rounds and the ascending output by explicit loops; the cells by loops over
sequence, start and column), and gs_motif_run_multi_batch_summary against what exists: the
stats call's bins and site counts reduced the same way, ListChainStats.mode(), and the list
aggregates (gs_counts a list slot) summed over the counted states of the stepwise loop.
Everything is integers or bits: every comparison is exact."""
import numpy as np
import pytest

from conftest import init_positions, make_dataset
from gibbssampling_amd import Context, ListChainStats, ListChainSummary, MotifSampler, _native
from gibbssampling_amd.sampler import createMotifIndex
from test_gpu_run_multi_batch import PC, SEEDS, SHAPES, bits, data, one_lists
from test_gpu_run_multi_batch_stats import STATS, T_STEP, bound, counted_sweeps, steps_of
from test_gpu_run_multi_batch_stats import same as same_array
from test_gpu_summary import G_BURN, G_SEEDS, G_T, G_THIN, G_W, check_subset, group_data

pytestmark = pytest.mark.gpu

DNA = b"ACGT"
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
STAGE_BINS = 512  # kListStageBins (gs_chainstats.hip): a row of up to so many bins is staged
# bins a row: two bins is L = W; then around a wavefront's 64 lanes and the staged capacity
BINS = (2, 3, 63, 64, 65, 128, 129, 200, STAGE_BINS - 1, STAGE_BINS, STAGE_BINS + 1,
        2 * STAGE_BINS + 76)
BIG = 2**31 - 1
MODES = ("mode_sites", "mode_sites_count", "mode_cnt", "mode_pos", "mode_count")
POOL = ("pooled_sites", "pooled_sites_count", "pooled_cnt", "pooled_pos", "pooled_count",
        "pooled_counts", "n_pooled")
GROUPS = {"modes": MODES, "counts": ("counts",), "pool": POOL}


# ---- the numpy restatement ----

def reduce_row(bins, sites, W):
    """One view's row by the definition -> (c*, its count, the starts taken in ascending
    order, their bins, whether a round passed over an excluded start that came before its
    pick in the order)."""
    bins, sites = [int(x) for x in bins], [int(x) for x in sites]
    cstar = 0
    for c in range(1, len(sites)):  # the smallest c with the largest count
        if sites[c] > sites[cstar]:
            cstar = c
    K = len(bins) - 1
    excluded = [False] * K
    taken, skipped = [], False
    for _ in range(cstar):
        pick = None
        for k in range(K):  # the largest bin, the smallest k among equals
            if not excluded[k] and (pick is None or bins[1 + k] > bins[1 + pick]):
                pick = k
        if pick is None:  # every start is excluded
            break
        for k in range(K):
            if excluded[k] and (bins[1 + k] > bins[1 + pick] or
                                (bins[1 + k] == bins[1 + pick] and k < pick)):
                skipped = True
        taken.append(pick)
        for k in range(max(0, pick - W), min(K, pick + W + 1)):  # |k - pick| <= W
            excluded[k] = True
    taken.sort()
    return cstar, sites[cstar], taken, [bins[1 + k] for k in taken], skipped


def reduce_view(occ, sites, off, W, dtype):
    """One view -> (mode_sites, mode_sites_count, mode_cnt, mode_pos, mode_count, rows with a
    skip, rows with c* >= 2)."""
    N, M = len(off) - 1, sites.shape[1] - 1
    ms, mcnt = np.zeros(N, np.int32), np.zeros(N, np.int32)
    msc = np.zeros(N, dtype)
    mpos, mcount = np.full((N, M), -1, np.int32), np.zeros((N, M), dtype)
    skips = multi = 0
    for n in range(N):
        c, cc, taken, counts, skipped = reduce_row(occ[off[n]:off[n + 1]], sites[n], W)
        ms[n], msc[n], mcnt[n] = c, cc, len(taken)
        mpos[n, :len(taken)], mcount[n, :len(taken)] = taken, counts
        skips += skipped
        multi += c >= 2
    return ms, msc, mcnt, mpos, mcount, skips, multi


def count_cells(occ, off, codes, offsets, alpha, W):
    """Per chain C[a W + j] then T[a], by the definition: explicit loops over the sequence n,
    the start k (zero bins add nothing) and the column j."""
    A = len(alpha)
    index = {int(c): a for a, c in enumerate(alpha)}
    out = np.zeros((len(occ), A * W + A), np.int64)
    for r in range(len(occ)):
        for n in range(len(off) - 1):
            sym = [index.get(int(c), -1) for c in codes[offsets[n]:offsets[n + 1]]]
            comp = [sum(1 for x in sym if x == a) for a in range(A)]
            for k in range(int(off[n + 1] - off[n]) - 1):
                c = int(occ[r, off[n] + 1 + k])
                if c == 0:
                    continue
                inside = [0] * A
                for j in range(W):
                    a = sym[k + j]
                    if a >= 0:
                        out[r, a * W + j] += c
                        inside[a] += 1
                for a in range(A):
                    out[r, A * W + a] += c * (comp[a] - inside[a])
    return out


def restate(occ, sites, off, n_counted, W, cells):
    """Every output of the summary from the bins, the site counts and the chains' cells."""
    occ, sites = np.asarray(occ, np.int32), np.asarray(sites, np.int32)
    R = len(occ)
    want = {k: [] for k in MODES}
    for r in range(R):
        for k, v in zip(MODES, reduce_view(occ[r], sites[r], off, W, np.int32)):
            want[k].append(v)
    want = {k: np.array(v) for k, v in want.items()}
    want["counts"] = cells
    keep = (sites.astype(np.int64).sum(axis=2) == n_counted).all(axis=1)
    *pooled, skips, multi = reduce_view(occ[keep].astype(np.int64).sum(axis=0),
                                        sites[keep].astype(np.int64).sum(axis=0), off, W,
                                        np.int64)
    want.update(zip(POOL[:5], pooled))
    want["pooled_counts"] = cells[keep].sum(axis=0)
    want["n_pooled"] = np.array([keep.sum()], np.int32)
    return want, skips, multi


def same(got, want, keys=None):
    for k in keys or want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def summary_twice(ctx, W, M, occ, sites, n_counted, **kw):
    """Every call twice: integer adds, so the outputs are bit-equal."""
    a = ctx.list_occupancy_summary(W, M, occ, sites, n_counted, **kw)
    b = ctx.list_occupancy_summary(W, M, occ, sites, n_counted, **kw)
    assert set(a) == set(b)
    same(a, b)
    return a


# ---- hand-made slabs ----

def sequences(bins, W, alpha, seed, extra=b""):
    """One sequence a row of `bins` bins (L = bins + W - 2)."""
    rng = np.random.default_rng(seed)
    lens = np.array([b + W - 2 for b in bins], np.int64)
    offsets = np.zeros(len(bins) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    a = np.frombuffer(alpha, np.uint8)
    codes = a[rng.integers(0, len(a), int(offsets[-1]))].astype(np.uint8)
    if extra:
        hit = rng.random(codes.size) < 0.1
        codes[hit] = extra[0]
        codes[offsets[:-1]] = extra[0]  # ... and in every first window
    return codes, offsets


def ragged(N, W, alpha, seed, extra=b""):
    """N sequences whose rows have BINS bins in turn (all of them from N = 12 on)."""
    order = BINS if N >= len(BINS) else (200, 2, STAGE_BINS + 1, 129, 2 * STAGE_BINS + 76)
    return sequences([order[n % len(order)] for n in range(N)], W, alpha, seed, extra)


def random_slabs(off, R, M, n_counted, seed):
    """Site rows of n_counted counts each; up to eight non-zero bins a row, ties among them."""
    rng = np.random.default_rng(seed)
    N = len(off) - 1
    occ = np.zeros((R, int(off[-1])), np.int32)
    sites = np.zeros((R, N, M + 1), np.int32)
    for r in range(R):
        for n in range(N):
            sites[r, n] = rng.multinomial(n_counted, rng.dirichlet(np.ones(M + 1)))
            nb = int(off[n + 1] - off[n])
            at = rng.integers(0, nb, rng.integers(0, 9))
            occ[r, off[n] + at] = rng.integers(1, 6, len(at))
    return occ, sites


HAND = {
    "dna-257-w12-m2-r3": (DNA, 257, 12, 2, 3, b""),
    "dna-257-w4-m1-r1": (DNA, 257, 4, 1, 1, b""),
    "protein-257-w4-m4-r1": (PROTEIN, 257, 4, 4, 1, b""),
    "protein-5-w12-m16-r3": (PROTEIN, 5, 12, 16, 3, b""),
    "dna-1-w4-m2-r3": (DNA, 1, 4, 2, 3, b""),
    "dna-5-w12-m4-r3": (DNA, 5, 12, 4, 3, b""),
    "outside-symbol-257-w12-m2-r3": (DNA, 257, 12, 2, 3, b"N"),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_slabs(gpu_ctx, name):
    alpha, N, W, M, R, extra = HAND[name]
    codes, offsets = ragged(N, W, alpha, seed=len(name), extra=extra)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    off = gpu_ctx.occupancy_offsets(W)
    if N >= len(BINS):
        assert sorted(set(np.diff(off).tolist())) == sorted(BINS)
    nc = 40
    occ, sites = random_slabs(off, R, M, nc, seed=N + W + M)
    cells = count_cells(occ, off, codes, offsets, alpha, W)
    want, skips, multi = restate(occ, sites, off, nc, W, cells)
    got = summary_twice(gpu_ctx, W, M, occ, sites, nc)
    same(got, want)
    assert got["n_pooled"][0] == R
    if N >= len(BINS) and M >= 2:  # the random slabs do exercise the rule
        assert skips > 0 and multi > 0
    # the cells are gs_occupancy_summary's on the same bins
    plain = gpu_ctx.occupancy_summary(W, occ, nc, modes=False, pool=False)
    assert np.array_equal(got["counts"], plain["counts"])
    if extra:  # the symbol outside the alphabet is in the data, and in counted windows
        assert (codes == extra[0]).any()
        inside = sum(int(cells[0, a * W:(a + 1) * W].sum()) for a in range(len(alpha)))
        assert inside < int(occ[0].sum() - occ[0, off[:-1]].sum()) * W
    # each output group alone equals the same group of the full call
    for g, keys in GROUPS.items():
        part = summary_twice(gpu_ctx, W, M, occ, sites, nc, **{k: k == g for k in GROUPS})
        assert set(part) == set(keys)
        same(part, got, keys)


def planted(ctx, W, M, rows, R=2, nc=10):
    """rows: (bins of the row, {start: count}, site counts) a sequence, the same in R chains
    -> (the summary, the restatement's)."""
    codes, offsets = sequences([b for b, _, _ in rows], W, DNA, seed=len(rows))
    ctx.set_sequences(codes, offsets, DNA)
    off = ctx.occupancy_offsets(W)
    occ = np.zeros((R, int(off[-1])), np.int32)
    sites = np.zeros((R, len(rows), M + 1), np.int32)
    for n, (_, at, s) in enumerate(rows):
        for k, c in at.items():
            occ[:, off[n] + 1 + k] = c
        sites[:, n, :len(s)] = s
    want, _, _ = restate(occ, sites, off, nc, W, count_cells(occ, off, codes, offsets, DNA, W))
    got = summary_twice(ctx, W, M, occ, sites, nc)
    same(got, want)
    return got


def row_of(got, n, r=0):
    c = int(got["mode_cnt"][r, n])
    assert (got["mode_pos"][r, n, c:] == -1).all() and not got["mode_count"][r, n, c:].any()
    return (int(got["mode_sites"][r, n]), int(got["mode_sites_count"][r, n]),
            got["mode_pos"][r, n, :c].tolist(), got["mode_count"][r, n, :c].tolist())


def test_the_distance_rule_ties_and_short_lists(gpu_ctx):
    W, M = 4, 3
    two, one, three = [0, 0, 10], [0, 10], [0, 0, 0, 10]
    rows = [
        (100, {10: 9, 10 + W: 8, 30: 5}, two),          # 0: exactly W apart: excluded
        (100, {10: 9, 10 + W + 1: 8, 30: 5}, two),      # 1: W + 1 apart: taken
        (100, {20: 9, 22: 8, 40: 1}, two),              # 2: the excluded start is the larger
        (129, {5: 7, 5 + 64: 7, 90: 3}, one),           # 3: equal counts in one lane
        (129, {37: 7, 38: 7, 90: 3}, two),              # 4: ... at k and k + 1
        (129, {0: 7, 127: 7, 60: 3}, one),              # 5: ... at the first and last start
        (129, {0: 7, 127: 7, 60: 3}, three),            # 6: ... and all three taken in order
        (W + 3, {0: 5, 1: 4, W + 1: 2}, three),         # 7: W + 2 starts, c* = 3: a short list
        (100, {10: 6}, two),                            # 8: a zero-count pick
        (100, {10: 6, 50: 6}, [10]),                    # 9: c* = 0 with non-zero bins
        (100, {10: 6, 50: 5}, [1, 4, 4, 1]),            # 10: site counts 1 and 2 tie: 1 wins
        (2, {0: 3}, two),                               # 11: L = W, one start
        (STAGE_BINS + 1, {300: 9, 300 + W: 8, STAGE_BINS - 1: 5}, two),  # 12: the last start, unstaged
        (STAGE_BINS, {300: 9, 300 + W: 8, STAGE_BINS - 2: 5}, two),      # 13: ... and staged
    ]
    got = planted(gpu_ctx, W, M, rows)
    assert got["n_pooled"][0] == 2
    expect = {0: (2, 10, [10, 30], [9, 5]), 1: (2, 10, [10, 15], [9, 8]),
              2: (2, 10, [20, 40], [9, 1]), 3: (1, 10, [5], [7]), 4: (2, 10, [37, 90], [7, 3]),
              5: (1, 10, [0], [7]), 6: (3, 10, [0, 60, 127], [7, 3, 7]),
              7: (3, 10, [0, W + 1], [5, 2]), 8: (2, 10, [0, 10], [0, 6]), 9: (0, 10, [], []),
              10: (1, 4, [10], [6]), 11: (2, 10, [0], [3]),
              12: (2, 10, [300, STAGE_BINS - 1], [9, 5]),
              13: (2, 10, [300, STAGE_BINS - 2], [9, 5])}
    for n, e in expect.items():
        assert row_of(got, n) == e and row_of(got, n, 1) == e, n
        assert int(got["pooled_sites"][n]) == e[0] and got["pooled_sites_count"][n] == 2 * e[1]
        c = int(got["pooled_cnt"][n])
        assert got["pooled_pos"][n, :c].tolist() == e[2], n
        assert got["pooled_count"][n, :c].tolist() == [2 * x for x in e[3]], n


def test_sixteen_picks_and_an_all_zero_site_row(gpu_ctx):
    W, M = 4, 16
    full = [0] * 16 + [10]
    starts = {5 * i: 40 - i for i in range(16)}  # W + 1 apart, descending
    rows = [(100, starts, full),
            (100, {5 * i: 7 for i in range(16)}, full),  # ... all equal
            (100, starts, [0] * 17),                     # an all-zero site row: (0, 0)
            (2 * STAGE_BINS + 76, {70 * i: 1 + i for i in range(16)}, full)]
    got = planted(gpu_ctx, W, M, rows)
    assert got["n_pooled"][0] == 0  # sequence 2's site counts are short in every chain
    for n in (0, 1):
        assert row_of(got, n)[:3] == (16, 10, [5 * i for i in range(16)])
    assert row_of(got, 0)[3] == [40 - i for i in range(16)]
    assert row_of(got, 2) == (0, 0, [], [])
    assert row_of(got, 3) == (16, 10, [70 * i for i in range(16)], [1 + i for i in range(16)])
    assert not got["pooled_sites"].any() and not got["pooled_cnt"].any()
    assert (got["pooled_pos"] == -1).all() and not got["pooled_counts"].any()
    assert got["counts"].any()


def test_counts_beyond_int32_and_the_pool(gpu_ctx):
    """2^31 - 1 in one bin and one site count of each of three pooled chains: the pooled counts
    pass int32 and a cell 2^32; then one chain whose last sequence is one count short, and
    nobody pooled."""
    alpha, N, W, M, R = DNA, 5, 4, 2, 3
    codes, offsets = ragged(N, W, alpha, seed=3)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    off = gpu_ctx.occupancy_offsets(W)
    occ = np.zeros((R, int(off[-1])), np.int32)
    sites = np.zeros((R, N, M + 1), np.int32)
    occ[:, off[:-1] + 1] = BIG  # start 0 of every sequence
    sites[:, :, 1] = BIG
    cells = count_cells(occ, off, codes, offsets, alpha, W)
    want, _, _ = restate(occ, sites, off, BIG, W, cells)
    got = summary_twice(gpu_ctx, W, M, occ, sites, BIG)
    same(got, want)
    assert got["n_pooled"][0] == 3 and (got["pooled_sites_count"] == 3 * BIG).all()
    assert (got["pooled_count"][:, 0] == 3 * BIG).all() and (got["pooled_cnt"] == 1).all()
    assert got["pooled_counts"].max() > 2**32 and got["counts"].max() > 2**32
    assert (got["mode_count"][:, :, 0] == BIG).all() and (got["mode_sites_count"] == BIG).all()

    nc = 40
    occ, sites = random_slabs(off, R, M, nc, seed=8)
    c = int(np.argmax(sites[1, N - 1]))
    sites[1, N - 1, c] -= 1  # the last sequence of chain 1; its sequence 0 is complete
    cells = count_cells(occ, off, codes, offsets, alpha, W)
    want, _, _ = restate(occ, sites, off, nc, W, cells)
    got = summary_twice(gpu_ctx, W, M, occ, sites, nc)
    same(got, want)
    assert got["n_pooled"][0] == 2 and sites[1, 0].sum() == nc
    assert np.array_equal(got["pooled_counts"], got["counts"][[0, 2]].sum(axis=0))
    assert got["mode_sites_count"][1, N - 1] == sites[1, N - 1].max()  # its own rows: reduced

    got = summary_twice(gpu_ctx, W, M, occ, sites, nc + 1)
    same(got, restate(occ, sites, off, nc + 1, W, cells)[0])
    assert got["n_pooled"][0] == 0 and not got["pooled_counts"].any()
    assert not got["pooled_sites"].any() and not got["pooled_sites_count"].any()
    assert not got["pooled_cnt"].any() and (got["pooled_pos"] == -1).all()
    assert got["counts"].any() and got["mode_cnt"].any()


# ---- the run call against what exists ----

COUNTS = ((0, 1), (3, 1), (2, 3), (12, 1))
RUN_SHAPES = ["dna-m2", "dna-m3-shared", "m4", "protein-m2", "neg-cutoff"]
_aggs = {}


@pytest.fixture(scope="module")
def other_ctx():
    """The stepwise side: a second context with the shipped defaults."""
    ctx = Context(0)
    yield ctx
    ctx.close()


def list_aggregates(ctx, W, A, cnt, pos):
    """The list aggregates of one state (cnt[N], pos[N, cap]): C over every listed segment,
    T[a] over the list entries of the sequence's symbols outside the entry's segment:
    gs_counts of every list slot, summed."""
    total = np.zeros(A * W + A, np.int64)
    for i in range(pos.shape[1]):
        C, T = ctx.counts(W, np.where(cnt > i, pos[:, i], -1).astype(np.int32), A)
        total += np.concatenate([C.ravel(), T])
    return total


def aggregates_of(other_ctx, name):
    """[T_STEP, R, cells] of the stepwise states, computed once and left unchanged."""
    if name not in _aggs:
        alpha, N, L, W = SHAPES[name][:4]
        C, P = steps_of(other_ctx, name)[:2]
        ctx = bound(other_ctx, name)
        out = np.array([[list_aggregates(ctx, W, len(alpha), C[t][r], P[t][r])
                         for r in range(len(SEEDS))] for t in range(T_STEP)])
        out.setflags(write=False)
        _aggs[name] = out
    return _aggs[name]


def summary_object(s, W, A):
    return ListChainSummary(*(s[k] for k in MODES + ("counts",) + POOL[:6]),
                            int(s["n_pooled"][0]), s["n_counted"], s["ic"], s["best_sweep"], [],
                            W, A)


@pytest.mark.parametrize("burn_in,thin", COUNTS)
@pytest.mark.parametrize("name", RUN_SHAPES)
def test_run_call_against_the_stats_call(name, burn_in, thin, gpu_ctx, other_ctx):
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
    codes, offsets = data(name)
    aggs = aggregates_of(other_ctx, name)
    ctx = bound(gpu_ctx, name)
    kw = dict(init_mode=mode, burn_in=burn_in, thin=thin)
    *rows, status, st = ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, T_STEP, SEEDS, **kw)
    *srows, sstatus, s = ctx.motif_run_multi_batch_summary(M, W, PC, cutoff, T_STEP, SEEDS,
                                                           occupancy=True, sites=True, **kw)
    assert not status.any() and not sstatus.any()
    ts = counted_sweeps(T_STEP, burn_in, thin)
    R, off = len(SEEDS), st["offsets"]
    # the chains and the statistics are the stats call's, to the bit
    for a, b in zip(srows, rows):
        assert same_array(a, b)
    for k in STATS:
        assert same_array(s[k], st[k]), k
    assert s["n_counted"] == len(ts) and np.array_equal(s["offsets"], off)
    # the summary is the restatement's of those bins; the cells are the list aggregates
    # summed over the counted states of the stepwise loop
    cells = aggs[ts].sum(axis=0) if ts else np.zeros_like(aggs[0])
    want, skips, multi = restate(st["occupancy"], st["sites"], off, len(ts), W, cells)
    same(s, want)
    assert s["n_pooled"][0] == R
    assert np.array_equal(cells, count_cells(st["occupancy"], off, codes, offsets, alpha, W))
    if name in ("dna-m2", "dna-m3-shared") and burn_in in (0, 3):
        assert skips >= 1 and multi >= 1  # the pooled view exercises the distance rule
    # the bins stay on the device unless asked for
    *_, lean = ctx.motif_run_multi_batch_summary(M, W, PC, cutoff, T_STEP, SEEDS, **kw)
    assert "occupancy" not in lean and "sites" not in lean and "offsets" not in lean
    same(lean, want)
    # the mirror's mode is ListChainStats.mode() of the same chains
    mine = summary_object(lean, W, len(alpha)).mode()
    theirs = ListChainStats(st["occupancy"], off, st["ic"], st["best_sweep"], [], st["sites"],
                            W).mode()
    assert [m.Positions for m in mine] == [m.Positions for m in theirs]
    assert np.array_equal(bits([m.PWMS for m in mine]), bits([m.PWMS for m in theirs]))
    if name == "m4":  # seed 12: the all-empty absorbing state
        r = SEEDS.index(12)
        assert not s["mode_sites"][r].any() and not s["mode_cnt"][r].any()
        assert (s["mode_sites_count"][r] == len(ts)).all() and (s["mode_pos"][r] == -1).all()
    for k in MODES + ("counts",):  # the duplicate seed: identical rows
        assert np.array_equal(s[k][1], s[k][3]), k


def test_a_raising_chain_is_left_out_of_the_pool(gpu_ctx):
    """The setup of test_a_raising_chain_stops_counting: chain 1 raises in sweep 1."""
    R, T, N, W, M = 3, 4, 30, 6, 2
    codes, offsets = make_dataset(N, 40, W, seed=51)
    cnt0, pos0 = one_lists(init_positions(offsets, W, 52), M)
    u = np.random.default_rng(53).random((R, T, N))
    u[1, 1, 7] = 2.0  # beyond every category: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, DNA)
    cnts, poss = np.tile(cnt0, (R, 1)), np.tile(pos0, (R, 1, 1))
    run = gpu_ctx.motif_run_multi_batch_summary
    *_, status, s = run(M, W, PC, 1.0, T, [1, 2, 3], cnts, poss, u=u, occupancy=True, sites=True)
    assert status.tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    *_, status, st = gpu_ctx.motif_run_multi_batch_stats(M, W, PC, 1.0, T, [1, 2, 3], cnts, poss,
                                                         u=u)
    assert status.tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    for k in STATS:
        assert same_array(s[k], st[k]), k
    off = s["offsets"]
    cells = count_cells(s["occupancy"], off, codes, offsets, DNA, W)
    same(s, restate(s["occupancy"], s["sites"], off, T, W, cells)[0])
    # chain 1 is summarised from the one sweep it counted, and is no member of the pool
    assert s["n_pooled"][0] == 2 and (s["mode_sites_count"][1] == 1).all()
    assert np.array_equal(s["pooled_counts"], s["counts"][[0, 2]].sum(axis=0))
    # chains 0 and 2 and the pool: the same call without chain 1
    *_, sto, so = run(M, W, PC, 1.0, T, [1, 3], cnts[[0, 2]], poss[[0, 2]], u=u[[0, 2]])
    assert not sto.any()
    for k in MODES + ("counts",):
        assert np.array_equal(s[k][[0, 2]], so[k]), k
    same(s, so, POOL)


def test_a_resumed_chain_is_summarised_once(gpu_ctx):
    """The setup of test_chains_that_park_in_a_later_sweep: chains 0 and 1 park in sweep 1 and
    are run again with larger arenas; the reduction follows the resumed round."""
    N, L, W, M, cutoff, T = 4, 264, 2, 3, -14.0, 2
    seeds = [7, 8, 9]
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    starts = [bytes(codes[offsets[n]:offsets[n + 1]]).index(w)
              for n, w in enumerate((b"AC", b"CG", b"GT", b"TA"))]
    c0, p0 = one_lists(np.array(starts, np.int32), M)
    cnts, poss = np.tile(c0, (3, 1)), np.tile(p0, (3, 1, 1))
    cnts[2], poss[2] = 0, -1
    gpu_ctx.set_sequences(codes, offsets, DNA)
    *_, status, s = gpu_ctx.motif_run_multi_batch_summary(M, W, PC, cutoff, T, seeds, cnts, poss,
                                                          occupancy=True, sites=True)
    info = gpu_ctx.run_multi_batch_last_info()
    assert not status.any()
    assert info["parked"] == 2 and info["resume_rounds"] == 1
    # (the bins and site counts of this setup are checked against the stepwise loop by
    # test_gpu_run_multi_batch_stats.py; here: the reduction saw them complete, once)
    off = s["offsets"]
    assert (s["sites"].sum(axis=2) == T).all() and not np.isnan(s["ic"]).any()
    assert np.array_equal(s["sites"] @ np.arange(M + 1),
                          np.add.reduceat(s["occupancy"], off[:-1], axis=1) -
                          s["occupancy"][:, off[:-1]])
    cells = count_cells(s["occupancy"], off, codes, offsets, DNA, W)
    same(s, restate(s["occupancy"], s["sites"], off, T, W, cells)[0])
    assert s["n_pooled"][0] == 3


def test_a_given_up_chain_is_summarised_from_nothing():
    """The setup of test_a_given_up_chain_has_no_statistics (run_multi_arena_max 32 768): chain
    1 parks in sweep 0 and is given up there."""
    N, L, W, M, cap, cutoff, T = 4, 264, 2, 3, 8, -10.0, 2
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    cnt = np.zeros((2, N), np.int32)
    pos = np.full((2, N, cap), -1, np.int32)
    for n in range(N):
        q = codes[offsets[n]:offsets[n + 1]]
        first = [int(np.nonzero(q[:L - 1] == a)[0][0]) for a in DNA]
        second = [int(np.nonzero(q[1:] == a)[0][0]) for a in DNA]
        pos[1, n], cnt[1, n] = first + second, cap
    ctx = Context(0, tuning={"run_multi_arena_max": 32768})
    ctx.set_sequences(codes, offsets, DNA)
    *_, status, s = ctx.motif_run_multi_batch_summary(M, W, PC, cutoff, T, [7, 8], cnt, pos,
                                                      cap=cap)
    ctx.close()
    assert status.tolist() == [0, _native.GS_E_UNSUPPORTED]
    assert s["n_pooled"][0] == 1
    for k in MODES[:3] + ("mode_count", "counts"):
        assert not s[k][1].any(), k
    assert (s["mode_pos"][1] == -1).all()
    # chain 0 sits in the all-empty state: it is the pool
    assert not s["mode_sites"][0].any() and (s["mode_sites_count"][0] == T).all()
    assert not s["pooled_sites"].any() and (s["pooled_sites_count"] == T).all()
    assert not s["pooled_counts"].any()


# ---- edges ----

def test_edges(gpu_ctx, other_ctx):
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES["dna-m2"]
    codes, offsets = data("dna-m2")
    ctx = bound(gpu_ctx, "dna-m2")
    run = ctx.motif_run_multi_batch_summary
    cells = len(alpha) * W + len(alpha)
    cnt0, pos0 = one_lists(init_positions(offsets, W, 9), M)
    two_c, two_p = np.tile(cnt0, (2, 1)), np.tile(pos0, (2, 1, 1))

    # every summary output null: the stats call
    kw = dict(first_sweep=2, burn_in=1, thin=2)
    stats = ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, **kw)
    none = run(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, occupancy=True, sites=True,
               modes=False, counts=False, pool=False, **kw)
    for a, b in zip(none[:4], stats[:4]):
        assert same_array(a, b)
    assert set(none[4]) == set(stats[4]) | {"n_counted"}
    for k, v in stats[4].items():
        assert same_array(none[4][k], v), k
    # each group alone equals the full call's
    full = run(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, **kw)
    assert ctx.summary_last_ms() > 0.0
    for g, keys in GROUPS.items():
        part = run(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, ic=False, best=False,
                   **{k: k == g for k in GROUPS}, **kw)
        assert set(part[4]) == set(keys) | {"n_counted"}
        same(part[4], full[4], keys)

    # nothing counted: (0, 0), empty lists, zero cells, everybody pooled
    for T, burn_in in ((0, 0), (5, 5)):
        *_, st, s = run(M, W, PC, cutoff, T, [31, 32], two_c, two_p, burn_in=burn_in)
        assert not st.any() and s["n_counted"] == 0 and s["n_pooled"][0] == 2
        for k in MODES + POOL[:6] + ("counts",):
            if k in ("mode_pos", "pooled_pos"):
                assert (s[k] == -1).all(), k
            else:
                assert not s[k].any(), k
        assert s["best_sweep"].tolist() == [-1, -1]
    # no chains: nothing to do
    c, p, w, st, s = run(M, W, PC, cutoff, 3, [])
    assert c.shape == (0, N) and s["mode_pos"].shape == (0, N, M) and s["n_pooled"][0] == 0
    empty = ctx.list_occupancy_summary(W, M, np.zeros((0, ctx.occupancy_offsets(W)[-1]), np.int32),
                                       np.zeros((0, N, M + 1), np.int32), 4)
    assert empty["counts"].shape == (0, cells) and empty["n_pooled"][0] == 0

    # refusals before any launch: nothing written, the counters unchanged
    before = ctx.stats()
    H = int(ctx.occupancy_offsets(W)[-1])
    occ, sites = np.zeros((2, H), np.int32), np.zeros((2, N, M + 1), np.int32)
    for bad in ({"burn_in": -1}, {"burn_in": 4}, {"thin": 0}):
        with pytest.raises(_native.ArgumentError):
            run(M, W, PC, cutoff, 3, [1, 2], **bad)
    with pytest.raises(_native.ArgumentError):
        run(M, L + 1, PC, cutoff, 3, [1, 2])
    with pytest.raises(_native.ArgumentError):
        run(3, W, PC, cutoff, 3, [1, 2], cap=2)
    for w_, m_, nc_ in ((0, M, 4), (L + 1, M, 4), (W, 0, 4), (W, 17, 4), (W, M, -1)):
        with pytest.raises(_native.ArgumentError):
            ctx.list_occupancy_summary(w_, m_, occ, sites, nc_)
    P = _native._ptr
    names = _native.Context._LIST_SUMMARY_KEYS

    def raw(R, occ_, sites_, drop=(), m=M):
        outs = ctx._list_summary_outputs(W, M, 2, True, True, True)
        for a in outs.values():
            a.fill(-7)
        rc = ctx.lib.gs_list_occupancy_summary(
            ctx.h, W, m, P(occ_), P(sites_), R, 4,
            *(None if k in drop else P(outs[k]) for k in names))
        assert all((a == -7).all() for a in outs.values())
        return rc

    assert raw(-1, occ, sites) == _native.GS_E_ARG
    assert raw(2, None, sites) == _native.GS_E_ARG and raw(2, occ, None) == _native.GS_E_ARG
    for k in ("mode_cnt", "mode_count", "pooled_sites", "pooled_count", "n_pooled"):
        assert raw(2, occ, sites, drop=(k,)) == _native.GS_E_ARG, k  # half of a group
    assert raw(2**31 - 1, occ, sites) == _native.GS_E_UNSUPPORTED  # beyond 4 GiB
    seeds = np.array([1, 2], np.uint64)
    row_c, row_p = np.zeros((2, N), np.int32), np.zeros((2, N, M), np.int32)
    row_d, stw = np.zeros((2, N), np.float64), np.zeros(2, np.int32)
    outs = ctx._list_summary_outputs(W, M, 2, True, True, True)
    for k in ("mode_sites", "pooled_pos"):
        rc = ctx.lib.gs_motif_run_multi_batch_summary(
            ctx.h, M, W, PC, cutoff, 3, P(seeds), 2, 0, 1, M, None, 0, 1, P(row_c), P(row_p),
            P(row_d), P(stw), None, None, None, None, None, None, None,
            *(None if n == k else P(outs[n]) for n in names))
        assert rc == _native.GS_E_ARG, k
    assert ctx.stats() == before
    ctx.set_fixed_pcv(np.full(49, 1.0 / 49))  # the sibling's refusals
    try:
        with pytest.raises(_native.GibbsError) as e:
            run(M, W, PC, cutoff, 3, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        ctx.set_fixed_pcv(None)
    assert ctx.stats() == before
    fresh = Context(0)  # no sequences
    try:
        rc = fresh.lib.gs_list_occupancy_summary(fresh.h, W, M, P(occ), P(sites), 2, 4,
                                                 *([None] * 13))
        assert rc == _native.GS_E_STATE
    finally:
        fresh.close()

    # the reduction of caller-held slabs leaves the snapshot alone ...
    p = init_positions(offsets, W, 3)
    ctx.set_positions(W, p)
    ctx.list_occupancy_summary(W, M, occ, sites, 0)
    assert np.array_equal(ctx.get_state()[0], p)
    # ... the run call leaves none, and the next single run behaves as on a fresh context
    run(M, W, PC, cutoff, 2, [5, 6], init_mode=1)
    with pytest.raises(_native.GibbsError) as e:
        ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    bound(other_ctx, "dna-m2")
    first = other_ctx.motif_sampling(W, PC, cutoff, 31)
    again = ctx.motif_sampling(W, PC, cutoff, 31)
    assert np.array_equal(again[0], first[0]) and again[2] == first[2]
    assert same_array(again[1], first[1])


def test_mirror_returns_the_summary_of_the_list_chains():
    N, L, W, T = 40, 60, 7, 8
    codes, offsets = make_dataset(N, L, W, DNA, seed=6, mut=0.1)
    sources = [bytes(codes[offsets[i]:offsets[i + 1]]) for i in range(N)]
    seeds = [99, 100, 2**40 + 1]
    mems = [[createMotifIndex(0.0, [] if p < 0 else [p])
             for p in init_positions(offsets, W, 20 + r, 0.1)] for r in range(len(seeds))]
    mems[1][0] = createMotifIndex(0.0, [L - W, 0])
    args = (W, PC, 1.0, "ACGT", sources, T, seeds, mems)
    kw = dict(first_sweep=3, burn_in=2, motifAmount=2)
    chains, st = MotifSampler.runSweepsBatchedListStats(*args, **kw)
    mine, s = MotifSampler.runSweepsBatchedListSummary(*args, **kw)
    assert mine == chains and isinstance(s, ListChainSummary)
    assert s.occupancy is None and s.sites is None and s.offsets is None
    assert s.n_pooled == 3 and s.n_counted == T - 2 and s.best == st.best
    assert np.array_equal(s.best_sweep, st.best_sweep) and same_array(s.ic, st.ic)
    a, b = s.mode(), st.mode()
    assert [m.Positions for m in a] == [m.Positions for m in b]
    assert np.array_equal(bits([m.PWMS for m in a]), bits([m.PWMS for m in b]))
    C, Tm = s.countMatrix()
    cells = count_cells(st.occupancy, st.offsets, codes, np.asarray(offsets), DNA, W)
    assert np.array_equal(np.concatenate([C.ravel(), Tm]), cells.sum(axis=0))
    Cr, Tr = s.countMatrix(pool=False)
    assert Cr.shape == (3, 4, W) and np.array_equal(Tr, cells[:, 4 * W:])
    _, s = MotifSampler.runSweepsBatchedListSummary(*args, occupancy=True, **kw)
    assert np.array_equal(s.occupancy, st.occupancy) and np.array_equal(s.sites, st.sites)
    assert np.array_equal(s.offsets, st.offsets)


# ---- group by group: what a call returns does not depend on what else was asked for ----
# (the data, shape and comparison of test_gpu_summary.py's group tests; lists of up to
# motifAmount 3 sites at capacity 5)

G_M, G_CAP = 3, 5
G_LIST_STATS = {"occupancy": ("offsets", "occupancy"), "sites": ("sites",), "ic": ("ic",),
                "best": ("best_sweep", "best_cnt", "best_pos", "best_pwms")}
LIST_GROUPS = dict(G_LIST_STATS, **GROUPS)


@pytest.fixture(scope="module")
def group_lists(gpu_ctx):
    gpu_ctx.set_sequences(*group_data(), DNA)
    kw = dict(init_mode=1, cap=G_CAP, burn_in=G_BURN, thin=G_THIN)
    return kw, gpu_ctx.motif_run_multi_batch_summary(G_M, G_W, PC, 1.0, G_T, G_SEEDS,
                                                     occupancy=True, sites=True, **kw)


@pytest.mark.parametrize("only", list(LIST_GROUPS) + ["none", "stats"])
def test_lists_group_by_group(gpu_ctx, group_lists, only):
    kw, ref = group_lists
    gpu_ctx.set_sequences(*group_data(), DNA)
    assert ref[4]["n_counted"] == 3 and not ref[3].any() and ref[1].shape[2] == G_CAP
    if only == "stats":
        got = gpu_ctx.motif_run_multi_batch_stats(G_M, G_W, PC, 1.0, G_T, G_SEEDS, **kw)
        check_subset(ref, got, dict(G_LIST_STATS), only)
    else:
        got = gpu_ctx.motif_run_multi_batch_summary(G_M, G_W, PC, 1.0, G_T, G_SEEDS, **kw,
                                                    **{g: g == only for g in LIST_GROUPS})
        check_subset(ref, got, LIST_GROUPS, only, extra=("n_counted",))
