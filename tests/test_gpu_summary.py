"""GPU parity of the chain summaries: gs_occupancy_summary on hand-made bins
against a numpy restatement (np.argmax per row; the count matrix by explicit loops over
sequence, start and column), and gs_run_sweeps_summary / gs_motif_run_summary /
gs_motif_run_batch_summary against what exists: the stats calls' bins reduced the same way,
ChainStats.mode(), and gs_counts summed over the counted states of the stepwise loop.
Everything is integers or bits: every comparison is exact."""
import numpy as np
import pytest

from conftest import init_positions, make_dataset
from gibbssampling_amd import ChainStats, Context, MotifSampler, _native
from gibbssampling_amd.sampler import createMotifIndex
from test_gpu_run_stats import (CASES, CUTOFF, PC, SEED, T, Pair, bits, counted_sweeps, dataset,
                                ran, stepwise)

pytestmark = pytest.mark.gpu

DNA = b"ACGT"
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
BINS = (2, 3, 63, 64, 65, 128, 129, 200)  # bins a row: two bins is L = W
BIG = 2**31 - 1
GROUPS = {"modes": ("mode_pos", "mode_count"), "counts": ("counts",),
          "pool": ("pooled_pos", "pooled_count", "pooled_counts", "n_pooled")}


# ---- the numpy restatement ----

def reduce_rows(occ, off):
    """Per chain and sequence the first maximum: (bin - 1, count)."""
    R, N = len(occ), len(off) - 1
    pos, cnt = np.zeros((R, N), np.int32), np.zeros((R, N), occ.dtype)
    for r in range(R):
        for n in range(N):
            row = occ[r, off[n]:off[n + 1]]
            b = int(np.argmax(row))
            pos[r, n], cnt[r, n] = b - 1, row[b]
    return pos, cnt


def count_cells(occ, off, codes, offsets, alpha, W):
    """Per chain C[a W + j] then T[a], by the definition: explicit loops over the sequence n,
    the start k (zero bins add nothing) and the column j."""
    A = len(alpha)
    index = {int(c): a for a, c in enumerate(alpha)}
    out = np.zeros((len(occ), A * W + A), np.int64)
    for r in range(len(occ)):
        for n in range(len(off) - 1):
            s = codes[offsets[n]:offsets[n + 1]]
            sym = [index.get(int(c), -1) for c in s]
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


def restate(occ, off, n_counted, codes, offsets, alpha, W):
    occ = np.asarray(occ, np.int32)
    want = {}
    want["mode_pos"], want["mode_count"] = reduce_rows(occ, off)
    want["counts"] = count_cells(occ, off, codes, offsets, alpha, W)
    keep = occ[:, off[0]:off[1]].astype(np.int64).sum(axis=1) == n_counted
    total = occ[keep].astype(np.int64).sum(axis=0)[None, :]
    pp, pc = reduce_rows(total, off)
    want["pooled_pos"], want["pooled_count"] = pp[0], pc[0].astype(np.int64)
    want["pooled_counts"] = want["counts"][keep].sum(axis=0)
    want["n_pooled"] = np.array([keep.sum()], np.int32)
    return want


def same(got, want, keys=None):
    for k in keys or want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def summary_twice(ctx, W, occ, n_counted, **kw):
    """Every call twice: integer adds, so the outputs are bit-equal."""
    a = ctx.occupancy_summary(W, occ, n_counted, **kw)
    b = ctx.occupancy_summary(W, occ, n_counted, **kw)
    assert set(a) == set(b)
    same(a, b)
    return a


# ---- hand-made bins ----

def ragged(N, W, alpha, seed, extra=b""):
    """N sequences whose rows have BINS bins in turn (all of them from N = 8 on)."""
    rng = np.random.default_rng(seed)
    order = BINS if N >= len(BINS) else (200, 2, 65, 129, 3)
    lens = np.array([order[n % len(order)] + W - 2 for n in range(N)], np.int64)
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    a = np.frombuffer(alpha, np.uint8)
    codes = a[rng.integers(0, len(a), int(offsets[-1]))].astype(np.uint8)
    if extra:
        hit = rng.random(codes.size) < 0.1
        codes[hit] = np.frombuffer(extra, np.uint8)[0]
        codes[offsets[:-1]] = np.frombuffer(extra, np.uint8)[0]  # ... and in every first window
    return codes, offsets


def random_bins(off, R, n_counted, seed):
    """Every row's n_counted counts spread over up to four of its bins."""
    rng = np.random.default_rng(seed)
    occ = np.zeros((R, int(off[-1])), np.int32)
    for r in range(R):
        for n in range(len(off) - 1):
            nb = int(off[n + 1] - off[n])
            at = rng.integers(0, nb, 4)
            np.add.at(occ[r], off[n] + at, rng.multinomial(n_counted, [0.25] * 4))
    return occ


def plant_edges(occ, off):
    """Ties and an empty row in rows of the right lengths (never sequence 0) -> what was
    planted, by name."""
    nb = np.diff(off)
    planted = {}

    def row_with(at_least, skip):
        for n in range(1, len(nb)):
            if nb[n] >= at_least and n not in skip:
                return n
        return None

    plans = (("one_lane", 129, lambda m: (5, 5 + 64)), ("neighbours", 65, lambda m: (37, 38)),
             ("first_and_last", 128, lambda m: (0, m - 1)), ("first_two", 3, lambda m: (0, 1)),
             ("zeros", 2, lambda m: ()))
    for name, need, where in plans:
        n = row_with(need, set(planted.values()))
        if n is None:
            continue
        planted[name] = n
        occ[:, off[n]:off[n + 1]] = 0
        for b in where(int(nb[n])):
            occ[:, off[n] + b] = 9
        for b in where(int(nb[n]))[:1]:  # smaller counts around the first maximum
            if b + 2 < nb[n]:
                occ[:, off[n] + b + 2] = 8
    return planted


HAND = {
    "dna-257-w12-r3": (DNA, 257, 12, 3, b""),
    "dna-257-w4-r1": (DNA, 257, 4, 1, b""),
    "protein-257-w4-r3": (PROTEIN, 257, 4, 3, b""),
    "protein-5-w12-r1": (PROTEIN, 5, 12, 1, b""),
    "dna-1-w4-r3": (DNA, 1, 4, 3, b""),
    "dna-5-w12-r3": (DNA, 5, 12, 3, b""),
    "outside-symbol-257-w12-r3": (DNA, 257, 12, 3, b"N"),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_made_bins(gpu_ctx, name):
    alpha, N, W, R, extra = HAND[name]
    codes, offsets = ragged(N, W, alpha, seed=len(name), extra=extra)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    off = gpu_ctx.occupancy_offsets(W)
    assert sorted(set(np.diff(off).tolist())) == sorted(set(BINS if N >= 8 else
                                                            (200, 2, 65, 129, 3)[:N]))
    nc = 40
    occ = random_bins(off, R, nc, seed=N + W)
    planted = plant_edges(occ, off)
    if N >= 257:
        assert set(planted) == {"one_lane", "neighbours", "first_and_last", "first_two", "zeros"}
    want = restate(occ, off, nc, codes, offsets, alpha, W)
    got = summary_twice(gpu_ctx, W, occ, nc)
    same(got, want)
    assert got["n_pooled"][0] == R
    # the first of equal maxima, wherever the two sit in the wavefront
    for key, (pos, cnt) in {"one_lane": (4, 9), "neighbours": (36, 9), "first_and_last": (-1, 9),
                            "first_two": (-1, 9), "zeros": (-1, 0)}.items():
        if key in planted:
            n = planted[key]
            assert (got["mode_pos"][:, n] == pos).all() and (got["mode_count"][:, n] == cnt).all()
            assert got["pooled_pos"][n] == pos and got["pooled_count"][n] == cnt * R
    if extra:  # the symbol outside the alphabet is in the data, and in counted windows
        assert (codes == extra[0]).any()
        inside = sum(int(want["counts"][0, a * W:(a + 1) * W].sum()) for a in range(len(alpha)))
        assert inside < int(occ[0].sum() - occ[0, off[:-1]].sum()) * W
    # each output group alone equals the same group of the full call
    for g, keys in GROUPS.items():
        part = summary_twice(gpu_ctx, W, occ, nc, **{k: k == g for k in GROUPS})
        assert set(part) == set(keys)
        same(part, got, keys)


def test_counts_beyond_int32_and_the_pool(gpu_ctx):
    """2^31 - 1 in each of three pooled chains: the pooled count passes int32 and a cell
    2^32; then one chain a count short of n_counted, and nobody pooled."""
    alpha, N, W, R = DNA, 5, 4, 3
    codes, offsets = ragged(N, W, alpha, seed=3)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    off = gpu_ctx.occupancy_offsets(W)
    occ = np.zeros((R, int(off[-1])), np.int32)
    occ[:, off[:-1] + 1] = BIG  # start 0 of every sequence
    want = restate(occ, off, BIG, codes, offsets, alpha, W)
    got = summary_twice(gpu_ctx, W, occ, BIG)
    same(got, want)
    assert got["n_pooled"][0] == 3 and (got["pooled_count"] == 3 * BIG).all()
    assert got["pooled_counts"].max() > 2**32 and got["counts"].max() > 2**32
    assert (got["mode_count"] == BIG).all()

    nc = 40
    occ = random_bins(off, R, nc, seed=8)
    first = off[0] + int(np.argmax(occ[1, off[0]:off[1]]))
    occ[1, first] -= 1
    want = restate(occ, off, nc, codes, offsets, alpha, W)
    got = summary_twice(gpu_ctx, W, occ, nc)
    same(got, want)
    assert got["n_pooled"][0] == 2
    assert np.array_equal(got["pooled_counts"], got["counts"][[0, 2]].sum(axis=0))
    assert got["mode_count"][1, 0] == occ[1, first]  # its own row is still reduced

    got = summary_twice(gpu_ctx, W, occ, nc + 1)
    same(got, restate(occ, off, nc + 1, codes, offsets, alpha, W))
    assert got["n_pooled"][0] == 0 and not got["pooled_counts"].any()
    assert (got["pooled_pos"] == -1).all() and not got["pooled_count"].any()
    assert got["counts"].any()


# ---- the run calls against what exists ----

RUN = {"ek4_loop": "ek4_loop", "long": "long", "protein": "protein"}
COUNTS = ((0, 1), (3, 1), (2, 3), (12, 1))
_runs = {}


def run_reference(name):
    """One kernel case, computed once and left unchanged: the stepwise chain on a second
    context, gs_counts of each of its states, and the stats call of every (burn_in, thin)."""
    if name not in _runs:
        spec = CASES[name]
        N, W = spec["N"], spec["W"]
        codes, offsets, p0 = dataset(N, *spec["L"], W, spec["alpha"], seed=len(name) + N)
        pair = Pair(spec["tuning"], spec["alpha"], codes, offsets)
        try:
            p0 = pair.step.random_starts(W, PC, SEED, 1)[1]
            s0 = pair.step.stats()
            P, Q = stepwise(pair.step, W, p0, T)
            ran(pair.step, spec, N * T, s0)
            A = len(spec["alpha"])
            cells = np.array([np.concatenate([c.ravel(), t]) for c, t in
                              (pair.step.counts(W, P[t], A) for t in range(T))], np.int64)
            stats = {}
            for burn_in, thin in COUNTS:
                s0 = pair.stat.stats()
                stats[burn_in, thin] = pair.stat.motif_run_stats(W, PC, CUTOFF, T, SEED, p0,
                                                                 burn_in=burn_in, thin=thin)
                ran(pair.stat, spec, N * T, s0)
        finally:
            pair.close()
        for x in (p0, cells):
            x.setflags(write=False)
        _runs[name] = (codes, offsets, p0, P, cells, stats)
    return _runs[name]


def same_stats(a, b, keys):
    for k in keys:
        assert np.array_equal(bits(a[k]) if a[k].dtype == np.float64 else a[k],
                              bits(b[k]) if b[k].dtype == np.float64 else b[k]), k


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", list(RUN))
def test_run_summary_against_the_stats_call(name, count):
    spec = CASES[name]
    N, W, alpha = spec["N"], spec["W"], spec["alpha"]
    burn_in, thin = count
    codes, offsets, p0, P, cells, stats = run_reference(name)
    spos, spw, st = stats[count]
    ts = counted_sweeps(T, burn_in, thin)
    ctx = Context(0, tuning=spec["tuning"])
    try:
        ctx.set_sequences(codes, offsets, alpha)
        s0 = ctx.stats()
        pos, pw, s = ctx.motif_run_summary(W, PC, CUTOFF, T, SEED, p0, burn_in=burn_in, thin=thin,
                                           occupancy=True)
        ran(ctx, spec, N * T, s0)
        assert ctx.summary_last_ms() > 0.0
        # the chain and the other statistics: the stats call's, to the bit
        assert np.array_equal(pos, spos) and np.array_equal(bits(pw), bits(spw))
        same_stats(s, st, ("ic", "best_sweep", "best_pos", "best_pwms", "occupancy", "offsets"))
        # the modes: the first-maximum reduction of the stats call's bins
        mp, mc = reduce_rows(st["occupancy"][None, :], st["offsets"])
        assert np.array_equal(s["mode_pos"], mp[0]) and np.array_equal(s["mode_count"], mc[0])
        # the cells: gs_counts summed over the counted states of the stepwise loop
        want = cells[ts].sum(axis=0) if ts else np.zeros(cells.shape[1], np.int64)
        assert s["counts"].dtype == np.int64 and np.array_equal(s["counts"], want)
        if not ts:
            assert (s["mode_pos"] == -1).all() and not s["mode_count"].any()
        # without the bins: the same summary; the snapshot stays and the chain goes on
        pos2, pw2, s2 = ctx.motif_run_summary(W, PC, CUTOFF, T, SEED, p0, burn_in=burn_in, thin=thin)
        assert "occupancy" not in s2
        same_stats(s2, s, ("ic", "best_sweep", "best_pos", "best_pwms", "mode_pos", "mode_count",
                           "counts"))
        again = ctx.get_state()
        assert np.array_equal(again[0], pos) and np.array_equal(bits(again[1]), bits(pw))
        # the summary outputs null: the stats call
        pos3, pw3, s3 = ctx.motif_run_summary(W, PC, CUTOFF, T, SEED, p0, burn_in=burn_in,
                                              thin=thin, occupancy=True, modes=False, counts=False)
        assert set(s3) == set(st)
        assert np.array_equal(pos3, spos) and np.array_equal(bits(pw3), bits(spw))
        same_stats(s3, st, [k for k in st if k != "status"])
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(RUN))
def test_chain_summary_mode_is_chain_stats_mode(name):
    spec = CASES[name]
    codes, offsets, p0, P, cells, stats = run_reference(name)
    W, alpha = spec["W"], spec["alpha"]
    lens = np.diff(offsets)
    sources = [codes[offsets[n]:offsets[n + 1]].tobytes() for n in range(len(lens))]
    mem = [createMotifIndex(0.0, [] if p < 0 else [p]) for p in p0]
    burn_in, thin = 2, 3
    chain, summary = MotifSampler.runSweepsSummary(W, PC, CUTOFF, alpha, sources, mem, T, burn_in,
                                                   thin, seed=SEED)
    chain2, st = MotifSampler.runSweepsStats(W, PC, CUTOFF, alpha, sources, mem, T, burn_in, thin,
                                             seed=SEED)
    assert chain == chain2 and summary.occupancy is None
    a, b = summary.mode(), st.mode()
    assert [m.Positions for m in a] == [m.Positions for m in b]
    assert np.array_equal(bits([m.PWMS for m in a]), bits([m.PWMS for m in b]))
    ts = counted_sweeps(T, burn_in, thin)
    C, Tc = summary.countMatrix()
    A = len(alpha)
    # (the sampler's context chooses its kernels itself: the cells against its own bins)
    from gibbssampling_amd import sampler
    want = sampler.context(0).occupancy_summary(W, st.occupancy, len(ts), modes=False, pool=False)
    assert np.array_equal(np.concatenate([C.ravel(), Tc]), want["counts"][0])
    assert np.array_equal(want["counts"][0], count_cells(st.occupancy, st.offsets, codes, offsets,
                                                         alpha, W)[0])
    assert C.shape == (A, W) and summary.n_counted == len(ts) and summary.n_pooled == 1
    _, both = MotifSampler.runSweepsSummary(W, PC, CUTOFF, alpha, sources, mem, T, burn_in, thin,
                                            seed=SEED, occupancy=True)
    assert np.array_equal(both.occupancy, st.occupancy) and np.array_equal(both.offsets, st.offsets)


def test_run_sweeps_summary_goes_on_as_the_stats_call(gpu_ctx):
    N, W = 257, 9
    codes, offsets, p0 = dataset(N, 24, 64, W, DNA, seed=23)
    gpu_ctx.set_sequences(codes, offsets, DNA)
    gpu_ctx.set_positions(W, p0)
    a = gpu_ctx.run_sweeps_stats(PC, CUTOFF, 5, SEED)
    sa = gpu_ctx.get_state()
    gpu_ctx.run_sweeps(PC, CUTOFF, T - 5, SEED, first_sweep=5)
    ea = gpu_ctx.get_state()
    gpu_ctx.set_positions(W, p0)
    b = gpu_ctx.run_sweeps_summary(PC, CUTOFF, 5, SEED, occupancy=True)
    sb = gpu_ctx.get_state()
    gpu_ctx.run_sweeps(PC, CUTOFF, T - 5, SEED, first_sweep=5)
    eb = gpu_ctx.get_state()
    for x, y in ((sa, sb), (ea, eb)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1]))
    same_stats(b, a, [k for k in a if k != "status"])
    mp, mc = reduce_rows(a["occupancy"][None, :], a["offsets"])
    assert np.array_equal(b["mode_pos"], mp[0]) and np.array_equal(b["mode_count"], mc[0])
    want = gpu_ctx.occupancy_summary(W, a["occupancy"][None, :], 5)
    assert np.array_equal(b["counts"], want["counts"][0])
    # the summary call left the snapshot alone
    after = gpu_ctx.get_state()
    assert np.array_equal(after[0], eb[0]) and np.array_equal(bits(after[1]), bits(eb[1]))


def test_a_raising_chain_summarises_the_bins_as_they_stand(gpu_ctx):
    N, W, n = 65, 6, 4
    codes, offsets, p0 = dataset(N, 24, 64, W, DNA, seed=17)
    u = np.random.default_rng(53).random((n, N))
    u[1, :] = 1.0  # past every category somewhere: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, DNA)
    gpu_ctx.set_positions(W, p0)
    want = gpu_ctx.run_sweeps_stats(PC, CUTOFF, n, SEED, u=u, strict=False)
    assert want["status"] == _native.GS_E_ROULETTE_OVERRUN and want["occupancy"].any()
    gpu_ctx.set_positions(W, p0)
    s = gpu_ctx.run_sweeps_summary(PC, CUTOFF, n, SEED, u=u, strict=False)
    assert s["status"] == _native.GS_E_ROULETTE_OVERRUN and "occupancy" not in s
    mp, mc = reduce_rows(want["occupancy"][None, :], want["offsets"])
    assert np.array_equal(s["mode_pos"], mp[0]) and np.array_equal(s["mode_count"], mc[0])
    assert mc.max() == 1  # the one sweep counted before the raise
    assert np.array_equal(s["counts"],
                          count_cells(want["occupancy"][None, :], want["offsets"], codes, offsets,
                                      DNA, W)[0])
    with pytest.raises(_native.RouletteOverrunError):
        gpu_ctx.get_state()


# ---- the batch ----

B_SEEDS = [1001, 77, 5_000_000_007, 77, 12]  # rows 1 and 3: the same seed
B_N, B_L, B_W, B_T = 40, 60, 8, 12


@pytest.fixture(scope="module")
def batch(gpu_ctx):
    codes, offsets = make_dataset(B_N, B_L, B_W, PROTEIN, seed=80, mut=0.1)
    return codes, offsets


def test_batch_summary_against_stats_plus_occupancy_summary(gpu_ctx, batch):
    codes, offsets = batch
    gpu_ctx.set_sequences(codes, offsets, PROTEIN)
    kw = dict(init_mode=1, burn_in=2, thin=3)
    pos, pw, status, st = gpu_ctx.motif_run_batch_stats(B_W, PC, CUTOFF, B_T, B_SEEDS, **kw)
    nc = len(counted_sweeps(B_T, 2, 3))
    want = gpu_ctx.occupancy_summary(B_W, st["occupancy"], nc)
    same(want, restate(st["occupancy"], st["offsets"], nc, codes, offsets, PROTEIN, B_W))
    bpos, bpw, bstatus, s = gpu_ctx.motif_run_batch_summary(B_W, PC, CUTOFF, B_T, B_SEEDS,
                                                            occupancy=True, **kw)
    assert gpu_ctx.summary_last_ms() > 0.0
    assert not status.any() and not bstatus.any()
    assert np.array_equal(bpos, pos) and np.array_equal(bits(bpw), bits(pw))
    same_stats(s, st, list(st))
    same(s, want)
    assert s["n_pooled"][0] == len(B_SEEDS) and s["n_counted"] == nc
    # duplicate seeds give identical rows
    for k in ("mode_pos", "mode_count", "counts"):
        assert np.array_equal(s[k][1], s[k][3]), k
    assert (s["mode_count"] > 0).all()
    # without the bins, and group by group
    _, _, _, lean = gpu_ctx.motif_run_batch_summary(B_W, PC, CUTOFF, B_T, B_SEEDS, **kw)
    assert "occupancy" not in lean
    same(lean, want)
    for g, keys in GROUPS.items():
        _, _, _, part = gpu_ctx.motif_run_batch_summary(B_W, PC, CUTOFF, B_T, B_SEEDS, ic=False,
                                                        best=False, **kw,
                                                        **{k: k == g for k in GROUPS})
        assert set(part) == set(keys) | {"n_counted"}
        same(part, want, keys)
    # all summary outputs null: the stats call
    p4, w4, _, s4 = gpu_ctx.motif_run_batch_summary(B_W, PC, CUTOFF, B_T, B_SEEDS, occupancy=True,
                                                    modes=False, counts=False, pool=False, **kw)
    assert np.array_equal(p4, pos) and np.array_equal(bits(w4), bits(pw))
    assert set(s4) == set(st) | {"n_counted"}
    same_stats(s4, st, list(st))
    # the sampler's entry point: ChainStats.mode() of the same chains
    sources = [codes[offsets[n]:offsets[n + 1]].tobytes() for n in range(B_N)]
    chains, summary = MotifSampler.runSweepsBatchedSummary(B_W, PC, CUTOFF, PROTEIN, sources, B_T,
                                                           B_SEEDS, init_mode=1, burn_in=2, thin=3)
    chains2, cs = MotifSampler.runSweepsBatchedStats(B_W, PC, CUTOFF, PROTEIN, sources, B_T,
                                                     B_SEEDS, init_mode=1, burn_in=2, thin=3)
    assert chains == chains2 and isinstance(cs, ChainStats)
    a, b = summary.mode(), cs.mode()
    assert [m.Positions for m in a] == [m.Positions for m in b]
    assert np.array_equal(bits([m.PWMS for m in a]), bits([m.PWMS for m in b]))
    C, Tc = summary.countMatrix()
    assert np.array_equal(np.concatenate([C.ravel(), Tc]), want["pooled_counts"])


def test_batch_a_raising_chain_is_left_out_of_the_pool(gpu_ctx):
    """The recipe of test_gpu_run_batch_stats.py: chain 1 raises in sweep 1."""
    R, n, N, W = 3, 4, 30, 6
    codes, offsets = make_dataset(N, 40, W, seed=51)
    p0 = init_positions(offsets, W, 52)
    u = np.random.default_rng(53).random((R, n, N))
    u[1, 1, 7] = 2.0  # beyond every category: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    starts = np.tile(p0, (R, 1))
    _, _, status, s = gpu_ctx.motif_run_batch_summary(W, PC, CUTOFF, n, [1, 2, 3], pos=starts, u=u,
                                                      occupancy=True)
    assert status.tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    assert s["n_pooled"][0] == 2
    same(s, restate(s["occupancy"], s["offsets"], n, codes, offsets, b"ACGT", W),
         [k for g in GROUPS.values() for k in g])
    assert s["mode_count"][1].max() == 1  # its own row: the sweep before the raise
    # the others are as without it
    _, _, sto, so = gpu_ctx.motif_run_batch_summary(W, PC, CUTOFF, n, [1, 3], pos=starts[[0, 2]],
                                                    u=u[[0, 2]])
    assert not sto.any() and so["n_pooled"][0] == 2
    for k in ("mode_pos", "mode_count", "counts"):
        assert np.array_equal(s[k][[0, 2]], so[k]), k
    same(s, so, GROUPS["pool"])


# ---- edges ----

def test_edges(gpu_ctx, batch):
    codes, offsets = batch
    ctx = gpu_ctx
    ctx.set_sequences(codes, offsets, PROTEIN)
    W, N, R = B_W, B_N, 2
    cells = len(PROTEIN) * W + len(PROTEIN)
    p0 = np.tile(init_positions(offsets, W, 9, 0.2), (R, 1))
    off = ctx.occupancy_offsets(W)
    H = int(off[-1])

    # no sweeps, and no counted sweep: modes (-1, 0), zero cells, every chain pooled
    for n_sweeps, burn_in in ((0, 0), (5, 5)):
        _, _, st, s = ctx.motif_run_batch_summary(W, PC, CUTOFF, n_sweeps, [31, 32], pos=p0,
                                                  burn_in=burn_in)
        assert not st.any() and s["n_pooled"][0] == R and s["n_counted"] == 0
        assert (s["mode_pos"] == -1).all() and not s["mode_count"].any()
        assert (s["pooled_pos"] == -1).all() and not s["pooled_count"].any()
        assert not s["counts"].any() and not s["pooled_counts"].any()
        _, _, s = ctx.motif_run_summary(W, PC, CUTOFF, n_sweeps, SEED, p0[0], burn_in=burn_in)
        assert (s["mode_pos"] == -1).all() and not s["mode_count"].any()
        assert not s["counts"].any()

    # no chains: nothing to do, nothing written
    P = _native._ptr
    lib = ctx.lib
    mp, mc = np.full((R, N), 7, np.int32), np.full((R, N), 7, np.int32)
    cnt = np.full((R, cells), 7, np.int64)
    pp, pc_, pcs, npool = (np.full(N, 7, np.int32), np.full(N, 7, np.int64),
                           np.full(cells, 7, np.int64), np.full(1, 7, np.int32))
    occ = random_bins(off, R, 10, seed=4)

    def call(W_=W, occ_=occ, R_=R, nc=10, mp_=mp, mc_=mc, cnt_=cnt, pp_=pp, pc2=pc_, pcs_=pcs,
             np_=npool, c=ctx):
        return lib.gs_occupancy_summary(c.h, W_, P(occ_), R_, nc, P(mp_), P(mc_), P(cnt_), P(pp_),
                                        P(pc2), P(pcs_), P(np_))

    ctx.set_positions(W, p0[0])
    ctx.synchronize()
    before, state = ctx.stats(), ctx.get_state()
    assert call(R_=0) == _native.GS_OK and call(R_=0, occ_=None) == _native.GS_OK
    out = ctx.occupancy_summary(W, np.zeros((0, H), np.int32), 3)
    assert out["mode_pos"].shape == (0, N) and out["n_pooled"][0] == 0
    # GS_E_ARG: a bad W, no bins, negative counts, half of a group
    for kw in ({"W_": 0}, {"W_": 65}, {"W_": B_L + 1}, {"occ_": None}, {"R_": -1}, {"nc": -1},
               {"mp_": None}, {"mc_": None}, {"pp_": None}, {"pc2": None}, {"pcs_": None},
               {"np_": None}, {"pp_": None, "pc2": None, "pcs_": None}):
        assert call(**kw) == _native.GS_E_ARG, kw
    for a in (mp, mc, cnt, pp, pc_, pcs, npool):
        assert (a == 7).all()
    with pytest.raises(_native.ArgumentError):
        ctx.occupancy_summary(W, occ, -1)
    # half of a group on the run calls
    seeds = np.array([1, 2], np.uint64)
    rows_i, rows_d, stw = p0.copy(), np.zeros((R, N)), np.zeros(R, np.int32)
    for m1, m2, q1, q2, q3, q4 in ((mp, None, None, None, None, None),
                                   (None, mc, None, None, None, None),
                                   (None, None, pp, pc_, pcs, None),
                                   (None, None, None, None, None, npool)):
        rc = lib.gs_motif_run_batch_summary(
            ctx.h, W, PC, CUTOFF, 3, P(seeds), R, 0, -1, None, 0, 1, P(rows_i), P(rows_d), P(stw),
            None, None, None, None, None, P(m1), P(m2), None, P(q1), P(q2), P(q3), P(q4))
        assert rc == _native.GS_E_ARG
    one_i, one_d = p0[0].copy(), np.zeros(N)
    for m1, m2 in ((mp[0], None), (None, mc[0])):
        assert lib.gs_run_sweeps_summary(ctx.h, PC, CUTOFF, 3, SEED, 0, None, 0, 1, None, None,
                                         None, None, None, P(m1), P(m2), None) == _native.GS_E_ARG
        assert lib.gs_motif_run_summary(ctx.h, W, PC, CUTOFF, 3, SEED, 0, None, 0, 1, P(one_i),
                                        P(one_d), None, None, None, None, None, P(m1), P(m2),
                                        None) == _native.GS_E_ARG
    for kw in ({"burn_in": -1}, {"burn_in": 4}, {"thin": 0}):
        with pytest.raises(_native.ArgumentError):
            ctx.run_sweeps_summary(PC, CUTOFF, 3, SEED, **kw)
        with pytest.raises(_native.ArgumentError):
            ctx.motif_run_summary(W, PC, CUTOFF, 3, SEED, p0[0], **kw)
        with pytest.raises(_native.ArgumentError):
            ctx.motif_run_batch_summary(W, PC, CUTOFF, 3, [1, 2], **kw)
    # nothing ran, and gs_occupancy_summary leaves the snapshot alone
    assert ctx.stats() == before
    good = ctx.occupancy_summary(W, occ, 10)
    assert ctx.stats() == before
    got = ctx.get_state()
    assert np.array_equal(got[0], state[0]) and np.array_equal(bits(got[1]), bits(state[1]))
    same(good, restate(occ, off, 10, codes, offsets, PROTEIN, W))

    fresh = Context(0)
    try:
        # GS_E_STATE: no sequences; no snapshot for the run call
        assert call(c=fresh) == _native.GS_E_STATE
        fresh.set_sequences(codes, offsets, PROTEIN)
        with pytest.raises(_native.GibbsError) as e:
            fresh.run_sweeps_summary(PC, CUTOFF, 3, SEED)
        assert e.value.status == _native.GS_E_STATE
        assert call(c=fresh) == _native.GS_OK  # ... which gs_occupancy_summary does not need
        # sharded sequences
        fresh.set_sequences(codes, offsets, PROTEIN, n_global=N + 5)
        assert call(c=fresh) == _native.GS_E_UNSUPPORTED
        with pytest.raises(_native.GibbsError) as e:
            fresh.motif_run_summary(W, PC, CUTOFF, 3, SEED, p0[0])
        assert e.value.status == _native.GS_E_UNSUPPORTED
        # a following motif_sampling behaves as on a fresh context
        fresh.set_sequences(codes, offsets, PROTEIN)
        want = fresh.motif_sampling(W, PC, CUTOFF, 31)
    finally:
        fresh.close()
    ctx.motif_run_batch_summary(W, PC, CUTOFF, 2, [5, 6], init_mode=1)
    ctx.occupancy_summary(W, occ, 10)
    again = ctx.motif_sampling(W, PC, CUTOFF, 31)
    assert np.array_equal(again[0], want[0]) and again[2] == want[2]
    assert np.array_equal(bits(again[1]), bits(want[1]))


# ---- group by group: what a call returns does not depend on what else was asked for ----
# The statistics' device slab and the summary's are carved from the parts a call asks for
# (DESIGN.md §9.30): a part left out must move nothing else.  Odd sizes everywhere (ragged
# lengths, W = 3, three chains, three counted sweeps), so that every part boundary is one a
# wrong alignment would show at.

G_LENS, G_W, G_T, G_BURN, G_THIN = (9, 10, 12, 13, 17), 3, 7, 2, 2
G_SEEDS = [11, 5_000_000_011, 23]
G_STATS = {"occupancy": ("offsets", "occupancy"), "ic": ("ic",),
           "best": ("best_sweep", "best_pos", "best_pwms")}


def group_data():
    offsets = np.concatenate([[0], np.cumsum(G_LENS)]).astype(np.int64)
    codes = np.frombuffer(DNA, np.uint8)[np.random.default_rng(90).integers(0, 4, offsets[-1])]
    return np.ascontiguousarray(codes), offsets


def same_bits(got, want, key):
    """Bit for bit: integers as they are, doubles as uint64; scalars by value."""
    if not isinstance(want, np.ndarray):
        assert got == want, key
        return
    assert got.dtype == want.dtype and got.shape == want.shape, key
    if want.dtype == np.float64:
        got, want = got.view(np.uint64), want.view(np.uint64)
    assert np.array_equal(got, want), key


def check_subset(ref, got, groups, only, extra=()):
    """`got` (chain outputs..., stats) of a call that asked for `only` (a group's name, "none",
    or "stats": every statistic through the _stats method) against the all-groups call."""
    for k, (a, b) in enumerate(zip(got[:-1], ref[:-1])):
        same_bits(a, b, f"chain output {k}")
    want_keys = set(extra)
    for g in (groups if only == "stats" else [only] if only != "none" else []):
        want_keys |= set(groups[g])
    assert set(got[-1]) == want_keys
    for key in want_keys:
        same_bits(got[-1][key], ref[-1][key], key)


@pytest.fixture(scope="module")
def group_single(gpu_ctx):
    codes, offsets = group_data()
    gpu_ctx.set_sequences(codes, offsets, DNA)
    p0 = init_positions(offsets, G_W, 91)
    kw = dict(burn_in=G_BURN, thin=G_THIN)
    return p0, kw, [gpu_ctx.motif_run_summary(G_W, PC, 1.0, G_T, s, p0, occupancy=True, **kw)
                    for s in G_SEEDS]


SINGLE_GROUPS = dict(G_STATS, modes=GROUPS["modes"], counts=GROUPS["counts"])


@pytest.mark.parametrize("only", list(SINGLE_GROUPS) + ["none", "stats"])
def test_single_chain_group_by_group(gpu_ctx, group_single, only):
    p0, kw, refs = group_single
    gpu_ctx.set_sequences(*group_data(), DNA)
    assert refs[0][2]["ic"].shape == (3,)
    for seed, ref in zip(G_SEEDS, refs):
        if only == "stats":
            got = gpu_ctx.motif_run_stats(G_W, PC, 1.0, G_T, seed, p0, **kw)
        else:
            got = gpu_ctx.motif_run_summary(G_W, PC, 1.0, G_T, seed, p0, **kw,
                                            **{g: g == only for g in SINGLE_GROUPS})
        check_subset(ref, got, dict(G_STATS) if only == "stats" else SINGLE_GROUPS, only,
                     extra=("status",))


@pytest.fixture(scope="module")
def group_batch(gpu_ctx):
    codes, offsets = group_data()
    gpu_ctx.set_sequences(codes, offsets, DNA)
    kw = dict(init_mode=1, burn_in=G_BURN, thin=G_THIN)
    return kw, gpu_ctx.motif_run_batch_summary(G_W, PC, 1.0, G_T, G_SEEDS, occupancy=True, **kw)


BATCH_GROUPS = dict(G_STATS, **GROUPS)


@pytest.mark.parametrize("only", list(BATCH_GROUPS) + ["none", "stats"])
def test_batch_group_by_group(gpu_ctx, group_batch, only):
    kw, ref = group_batch
    gpu_ctx.set_sequences(*group_data(), DNA)
    assert ref[3]["n_counted"] == 3 and not ref[2].any()
    if only == "stats":
        got = gpu_ctx.motif_run_batch_stats(G_W, PC, 1.0, G_T, G_SEEDS, **kw)
        check_subset(ref, got, dict(G_STATS), only)
    else:
        got = gpu_ctx.motif_run_batch_summary(G_W, PC, 1.0, G_T, G_SEEDS, **kw,
                                              **{g: g == only for g in BATCH_GROUPS})
        check_subset(ref, got, BATCH_GROUPS, only, extra=("n_counted",))
