"""GPU parity of gs_motif_run_multi_batch_stats: the chains of gs_motif_run_multi_batch with,
per chain, the occupancy of every motif start and the number of sites of every sequence over
the counted sweeps, the trace of the summed PWMS in its fixed order, and the best state
visited, all gathered on the device.  The reference is what a caller had to do before: T
one-sweep motif_run_multi_batch calls (init_mode -1, first_sweep advancing) on a second
context with a numpy tally.  Counts, lists and the chosen sweeps are compared exactly,
binary64 values bit for bit; against the oracle the trace within the PWMS tolerance plus the
summation's rounding."""
import numpy as np
import pytest

from conftest import init_positions, make_dataset, uniforms
from gibbssampling_amd import _native
from gibbssampling_amd.sampler import informationContent
from oracle import oracle_lib as ol
from test_gpu_run_multi_batch import PC, SEEDS, SHAPES, bits, data, fsx_set, one_lists

pytestmark = pytest.mark.gpu

T_STEP, T_ORACLE = 12, 4
STEP_SHAPES = ["dna-m2", "dna-m3-shared", "neg-cutoff", "m4", "protein-m2"]
STATS = ("occupancy", "sites", "ic", "best_sweep", "best_cnt", "best_pos", "best_pwms")


def counted_sweeps(T, burn_in, thin):
    return [t for t in range(T) if t >= burn_in and (t - burn_in) % thin == 0]


def tally(off, M, states):
    """(bins, site counts) of one chain over `states`, (cnt[N], pos[N, cap]) pairs."""
    N = len(off) - 1
    occ, sites = np.zeros(int(off[-1]), np.int32), np.zeros((N, M + 1), np.int32)
    for cnt, pos in states:
        for n in range(N):
            sites[n, cnt[n]] += 1
            if cnt[n] == 0:
                occ[off[n]] += 1
            for k in pos[n, :cnt[n]]:
                occ[off[n] + 1 + k] += 1
    return occ, sites


def first_best(ics):
    """The index of the first maximum as .fs:989 takes it: the first entry, replaced only by
    a strictly larger one (a NaN replaces nothing); -1 for no entry."""
    best = -1
    for i, x in enumerate(ics):
        if best < 0 or x > ics[best]:
            best = i
    return best


def same(a, b):
    """Equal arrays; binary64 ones bit for bit."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float64:
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


def identities(s, r, n_counted):
    """The three identities of sites_out (gibbs_hip.h) for the finished chain r."""
    off, occ, sites = s["offsets"], s["occupancy"][r], s["sites"][r]
    M = sites.shape[1] - 1
    assert np.array_equal(sites.sum(axis=1), np.full(len(sites), n_counted)), r
    assert np.array_equal(sites[:, 0], occ[off[:-1]]), r
    others = np.add.reduceat(occ, off[:-1]) - occ[off[:-1]]
    assert np.array_equal(sites @ np.arange(M + 1), others), r


def stepwise(ctx, M, W, cutoff, T, seeds, cnt, pos, cap=None, u=None, first=0):
    """T one-sweep calls from the lists -> (C[T, R, N], P[T, R, N, cap], Q[T, R, N], status of
    the last call)."""
    C, P, Q, st = [], [], [], None
    for t in range(T):
        cnt, pos, pw, st = ctx.motif_run_multi_batch(
            M, W, PC, cutoff, 1, seeds, cnt, pos, first_sweep=first + t, cap=cap,
            u=None if u is None else u[:, t:t + 1])
        C.append(cnt)
        P.append(pos)
        Q.append(pw)
    return np.array(C), np.array(P), np.array(Q), st


def check_chain(s, r, off, M, C, P, Q, ts, first=0):
    """Chain r's statistics against the tally of the stepwise states of the sweeps ts."""
    occ, sites = tally(off, M, [(C[t][r], P[t][r]) for t in ts])
    assert np.array_equal(s["occupancy"][r], occ), r
    assert np.array_equal(s["sites"][r], sites), r
    ics = [informationContent(Q[t][r]) for t in ts]
    assert np.array_equal(bits(s["ic"][r]), bits(ics)), r
    b = first_best(ics)
    if b < 0:
        assert s["best_sweep"][r] == -1, r
        return
    assert s["best_sweep"][r] == first + ts[b], r
    assert np.array_equal(s["best_cnt"][r], C[ts[b]][r]), r
    assert np.array_equal(s["best_pos"][r], P[ts[b]][r]), r  # entries past cnt are -1
    assert np.array_equal(bits(s["best_pwms"][r]), bits(Q[ts[b]][r])), r
    identities(s, r, len(ts))


@pytest.fixture(scope="module")
def other_ctx():
    """The stepwise side: a second context with the shipped defaults."""
    from gibbssampling_amd import Context
    ctx = Context(0)
    yield ctx
    ctx.close()


_steps = {}


def bound(ctx, name):
    codes, offsets = data(name)
    ctx.set_sequences(codes, offsets, SHAPES[name][0])
    return ctx


def steps_of(other_ctx, name):
    """The reference of one shape, computed once and left unchanged: the starts as lists,
    T_STEP one-sweep calls, the plain call of T_STEP sweeps, and the bins' offsets."""
    if name not in _steps:
        alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
        ctx = bound(other_ctx, name)
        c0, p0, _, st = ctx.motif_run_multi_batch(M, W, PC, cutoff, 0, SEEDS, init_mode=mode)
        assert not st.any()
        C, P, Q, st = stepwise(ctx, M, W, cutoff, T_STEP, SEEDS, c0, p0)
        assert not st.any()
        plain = ctx.motif_run_multi_batch(M, W, PC, cutoff, T_STEP, SEEDS, init_mode=mode)
        out = (C, P, Q, plain[0], plain[1], plain[2], ctx.occupancy_offsets(W))
        for a in out:
            a.setflags(write=False)
        _steps[name] = out
    return _steps[name]


@pytest.mark.parametrize("burn_in,thin", [(0, 1), (3, 1), (2, 3), (12, 1)])
@pytest.mark.parametrize("name", STEP_SHAPES)
def test_against_the_stepwise_loop(name, burn_in, thin, gpu_ctx, other_ctx):
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
    C, P, Q, plain_cnt, plain_pos, plain_pw, off = steps_of(other_ctx, name)
    ctx = bound(gpu_ctx, name)
    cnt, pos, pw, status, s = ctx.motif_run_multi_batch_stats(
        M, W, PC, cutoff, T_STEP, SEEDS, init_mode=mode, burn_in=burn_in, thin=thin)
    assert not status.any()
    ts = counted_sweeps(T_STEP, burn_in, thin)
    R = len(SEEDS)
    assert np.array_equal(s["offsets"], off)
    assert s["occupancy"].shape == (R, off[-1]) and s["sites"].shape == (R, N, M + 1)
    assert s["ic"].shape == (R, len(ts)) and s["best_pos"].shape == (R, N, M)
    # the chains are those of the plain call, and of the loop, to the bit
    assert np.array_equal(cnt, plain_cnt) and np.array_equal(pos, plain_pos)
    assert np.array_equal(bits(pw), bits(plain_pw))
    assert np.array_equal(cnt, C[-1]) and np.array_equal(pos, P[-1])
    assert np.array_equal(bits(pw), bits(Q[-1]))
    for r in range(R):
        check_chain(s, r, off, M, C, P, Q, ts)
    if name == "m4" and ts:  # seed 12: the all-empty absorbing state, the [] bins alone
        r = SEEDS.index(12)
        assert np.array_equal(s["sites"][r, :, 0], np.full(N, len(ts)))
        assert s["occupancy"][r].sum() == N * len(ts)
    if ts:  # lists of more than one position occur among the counted states
        assert C[ts].max() >= 2
    # the duplicate seed: identical rows
    for k in STATS:
        assert same(s[k][1], s[k][3]), k


@pytest.mark.parametrize("name", STEP_SHAPES)
def test_against_the_oracle(name, gpu_ctx):
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES[name]
    codes, offsets = data(name)
    ctx = bound(gpu_ctx, name)
    _, _, _, status, s = ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, T_ORACLE, SEEDS,
                                                         init_mode=mode)
    assert not status.any()
    off = s["offsets"]
    S = ol.Seqs(codes, offsets, alpha)
    decided = 0
    for seed in sorted(set(SEEDS)):
        _, p0 = ol.random_starts(S, W, PC, seed=seed, mode=mode)
        c, p = one_lists(p0, M)
        states, sums, tols = [], [], []
        for t in range(T_ORACLE):
            c, p, w = ol.sweep_lists(S, M, W, PC, cutoff, c, p, M,
                                     uniforms(seed, ol.stream_sweep(t), N))
            states.append((c, p))
            sums.append(float(np.sum(w)))
            # the project's PWMS tolerance plus the rounding of a sum of N terms
            tols.append((1e-12 + N * 2.0**-52) * float(np.sum(np.abs(w))))
        occ, sites = tally(off, M, states)
        ob = first_best(sums)
        # the oracle's best is decided when it leads every other sweep by more than both
        # sides' error: each trace entry is within its tol of the oracle's sum
        clear = all(abs(sums[ob] - sums[t]) > tols[ob] + tols[t]
                    for t in range(T_ORACLE) if t != ob)
        for r in [i for i, x in enumerate(SEEDS) if x == seed]:
            assert np.array_equal(s["occupancy"][r], occ), (seed, r)
            assert np.array_equal(s["sites"][r], sites), (seed, r)
            for t in range(T_ORACLE):
                assert abs(s["ic"][r, t] - sums[t]) <= tols[t], (seed, r, t)
            if clear:
                decided += 1
                assert s["best_sweep"][r] == ob, (seed, r)
                assert np.array_equal(s["best_cnt"][r], states[ob][0]), (seed, r)
                for n in range(N):
                    assert list(s["best_pos"][r, n, :states[ob][0][n]]) == \
                        list(states[ob][1][n, :states[ob][0][n]]), (seed, r, n)
    assert decided > 0  # the comparison of the best sweep took place


def test_amount_one_through_the_list_statistics(gpu_ctx):
    """motifAmount = 1, capacity 1: the statistics are gs_motif_run_batch_stats' (the `dna`
    shape of test_gpu_run_batch_stats.py)."""
    N, L, W, T = 150, 90, 9, 8
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=77, ragged=True, mut=0.1)
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    cnt, pos, pw, status, s = gpu_ctx.motif_run_multi_batch_stats(
        1, W, PC, 1.0, T, SEEDS, init_mode=1, cap=1, burn_in=1, thin=2)
    spos, spw, sstatus, so = gpu_ctx.motif_run_batch_stats(W, PC, 1.0, T, SEEDS, init_mode=1,
                                                           burn_in=1, thin=2)
    assert not status.any() and not sstatus.any()
    assert np.array_equal(pos[:, :, 0], spos) and np.array_equal(bits(pw), bits(spw))
    assert np.array_equal(s["occupancy"], so["occupancy"]) and s["occupancy"].any()
    assert np.array_equal(bits(s["ic"]), bits(so["ic"]))
    assert np.array_equal(s["best_sweep"], so["best_sweep"])
    assert np.array_equal(bits(s["best_pwms"]), bits(so["best_pwms"]))
    assert np.array_equal(s["best_pos"][:, :, 0], so["best_pos"])
    assert np.array_equal(s["best_cnt"], (so["best_pos"] >= 0).astype(np.int32))
    assert np.array_equal(s["sites"][:, :, 0], s["occupancy"][:, s["offsets"][:-1]])
    for r in range(len(SEEDS)):
        identities(s, r, 4)


def overflow_case(gpu_ctx, other_ctx, N, L, T, seeds):
    """Every window and every pair passes (cut-off -1000, W = 2, motifAmount 3): the batch
    with statistics against the stepwise loop."""
    W, M, cutoff = 2, 3, -1000.0
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    for ctx in (gpu_ctx, other_ctx):
        ctx.set_sequences(codes, offsets, b"ACGT")
    c0, p0, _, st = other_ctx.motif_run_multi_batch(M, W, PC, cutoff, 0, seeds)
    assert not st.any()
    C, P, Q, st = stepwise(other_ctx, M, W, cutoff, T, seeds, c0, p0)
    assert not st.any()
    cnt, pos, pw, status, s = gpu_ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, T, seeds)
    info = gpu_ctx.run_multi_batch_last_info()
    assert not status.any()
    assert np.array_equal(cnt, C[-1]) and np.array_equal(pos, P[-1])
    assert np.array_equal(bits(pw), bits(Q[-1]))
    for r in range(len(seeds)):
        check_chain(s, r, s["offsets"], M, C, P, Q, list(range(T)))
    return info


def test_overflow_on_the_device(gpu_ctx, other_ctx):
    """6 905 arena entries a target, above the first arena and below the overflow launch's:
    every pair is rescored on the device, no chain parks."""
    info = overflow_case(gpu_ctx, other_ctx, 12, 120, 3, [7, 8, 9, 10])
    assert info["rescored"] > 0 and info["parked"] == 0


def test_parking_and_resuming(gpu_ctx, other_ctx):
    """34 193 arena entries a target, above the overflow launch's 32 768: both chains park in
    sweep 0 and are run again with larger arenas.  Every counted sweep is there exactly once:
    the first round counted nothing for them, the resumed one all three sweeps."""
    info = overflow_case(gpu_ctx, other_ctx, 4, 264, 3, [7, 8])
    assert info["parked"] == 2 and info["resume_rounds"] >= 1


def test_chains_that_park_in_a_later_sweep(gpu_ctx, other_ctx):
    """Chains 0 and 1 park in sweep 1, not 0: the first round counts their sweep 0, the resumed
    one their sweep 1; chain 2 beside them never parks and is no member of the resumed round.
    N = 4, L = 264, W = 2, motifAmount 3, cut-off -14 (found with the CPU oracle).  Chains 0 and
    1 start from one window a sequence, reading AC, CG, GT, TA: a target's profile, built from
    the other three sequences' lists, then holds three symbols a column, and a window with
    both symbols outside them has two cells of (pc / 3.0004) / PCV, log2 about -26, and
    fails: the levels fit the overflow launch's arena (32 768 entries) and no chain parks.
    Sweep 0 writes three-position lists, nine segments a profile that hold more symbols a
    column; sweep 1 then needs more than 32 768 entries for some target of either chain (all
    263 + 260 * 261 / 2 = 34 193 when every window and pair passes).  Which sweep parks is
    read from the stepwise side's counts.  Chain 2 starts from empty lists: every cell is
    (pc / 3.0004) / PCV, no window passes, and it stays there."""
    N, L, W, M, cutoff, T = 4, 264, 2, 3, -14.0, 2
    seeds = [7, 8, 9]
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    starts = [bytes(codes[offsets[n]:offsets[n + 1]]).index(w)
              for n, w in enumerate((b"AC", b"CG", b"GT", b"TA"))]
    c0, p0 = one_lists(np.array(starts, np.int32), M)
    cnts, poss = np.tile(c0, (3, 1)), np.tile(p0, (3, 1, 1))
    cnts[2], poss[2] = 0, -1
    for ctx in (gpu_ctx, other_ctx):
        ctx.set_sequences(codes, offsets, b"ACGT")
    C, P, Q, parked = [], [], [], []
    c, p = cnts, poss
    for t in range(T):
        c, p, w, st = other_ctx.motif_run_multi_batch(M, W, PC, cutoff, 1, seeds, c, p,
                                                      first_sweep=t)
        assert not st.any()
        parked.append(other_ctx.run_multi_batch_last_info()["parked"])
        C.append(c), P.append(p), Q.append(w)
    assert parked == [0, 2]  # no chain parks in sweep 0, two in sweep 1
    cnt, pos, pw, status, s = gpu_ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, T, seeds,
                                                                  cnts, poss)
    info = gpu_ctx.run_multi_batch_last_info()
    assert not status.any()
    assert info["parked"] == 2 and info["resume_rounds"] == 1 and info["rescored"] > 0
    assert np.array_equal(cnt, C[-1]) and np.array_equal(pos, P[-1])
    assert np.array_equal(bits(pw), bits(Q[-1]))
    assert not np.isnan(s["ic"]).any() and not cnt[2].any()
    for r in range(3):
        check_chain(s, r, s["offsets"], M, C, P, Q, list(range(T)))


def test_a_given_up_chain_has_no_statistics():
    """The setup of test_a_chain_beyond_the_last_arena_is_given_up_alone: chain 1 parks in
    sweep 0 and is given up there, chain 0 sits in the all-empty state."""
    from gibbssampling_amd import Context
    N, L, W, M, cap, cutoff, T = 4, 264, 2, 3, 8, -10.0, 2
    codes, offsets = make_dataset(N, L, W, seed=41, mut=0.0)
    cnt = np.zeros((2, N), np.int32)
    pos = np.full((2, N, cap), -1, np.int32)
    for n in range(N):
        q = codes[offsets[n]:offsets[n + 1]]
        first = [int(np.nonzero(q[:L - 1] == a)[0][0]) for a in b"ACGT"]
        second = [int(np.nonzero(q[1:] == a)[0][0]) for a in b"ACGT"]
        pos[1, n], cnt[1, n] = first + second, cap
    ctx = Context(0, tuning={"run_multi_arena_max": 32768})
    ctx.set_sequences(codes, offsets, b"ACGT")
    c, p, w, status, s = ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, T, [7, 8], cnt, pos,
                                                         cap=cap)
    info = ctx.run_multi_batch_last_info()
    alone = ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, T, [7], cnt[:1], pos[:1], cap=cap)
    ctx.close()
    assert status.tolist() == [0, _native.GS_E_UNSUPPORTED]
    assert info["parked"] == 1 and info["resume_rounds"] == 0
    assert not s["occupancy"][1].any() and not s["sites"][1].any()
    assert np.isnan(s["ic"][1]).all() and s["ic"].shape == (2, T)
    assert s["best_sweep"][1] == -1
    # the empty-list chain beside it: as without the given-up chain
    assert not alone[3].any()
    for k in STATS:
        assert same(s[k][0], alone[4][k][0]), k
    assert np.array_equal(s["sites"][0, :, 0], np.full(N, T)) and s["best_sweep"][0] >= 0
    assert not np.isnan(s["ic"][0]).any() and not s["best_cnt"][0].any()
    identities(s, 0, T)


def test_a_raising_chain_stops_counting(gpu_ctx):
    """The explicit uniforms of test_explicit_uniforms_and_error_isolation: chain 1 raises in
    sweep 1."""
    R, T, N, W, M = 3, 4, 30, 6, 2
    codes, offsets = make_dataset(N, 40, W, seed=51)
    cnt0, pos0 = one_lists(init_positions(offsets, W, 52), M)
    u = np.random.default_rng(53).random((R, T, N))
    u[1, 1, 7] = 2.0  # beyond every category: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    cnts, poss = np.tile(cnt0, (R, 1)), np.tile(pos0, (R, 1, 1))
    *_, status, s = gpu_ctx.motif_run_multi_batch_stats(M, W, PC, 1.0, T, [1, 2, 3], cnts, poss,
                                                        u=u)
    assert status.tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    # chain 1: exactly the state of sweep 0
    c1, p1, w1, st1 = gpu_ctx.motif_run_multi_batch(M, W, PC, 1.0, 1, [2], cnts[1:2], poss[1:2],
                                                    u=u[1:2, :1])
    assert not st1.any()
    off = s["offsets"]
    occ, sites = tally(off, M, [(c1[0], p1[0])])
    assert np.array_equal(s["occupancy"][1], occ) and np.array_equal(s["sites"][1], sites)
    assert bits(s["ic"][1, :1])[0] == bits([informationContent(w1[0])])[0]
    assert np.isnan(s["ic"][1, 1:]).all() and not np.isnan(s["ic"][1, 0])
    assert s["best_sweep"][1] == 0
    assert np.array_equal(s["best_cnt"][1], c1[0]) and np.array_equal(s["best_pos"][1], p1[0])
    assert np.array_equal(bits(s["best_pwms"][1]), bits(w1[0]))
    # chains 0 and 2: the same call without chain 1
    *_, sto, so = gpu_ctx.motif_run_multi_batch_stats(M, W, PC, 1.0, T, [1, 3], cnts[[0, 2]],
                                                      poss[[0, 2]], u=u[[0, 2]])
    assert not sto.any() and not np.isnan(so["ic"]).any()
    for k in STATS:
        assert same(s[k][[0, 2]], so[k]), k
    for r in (0, 1):
        identities(so, r, T)


def test_more_chains_than_cus_fewer_targets_than_a_wavefront(gpu_ctx, other_ctx):
    """The .fsx:407 data set (N = 5, L = 27, W = 6, motifAmount 2), 300 chains of 6 sweeps."""
    seqs, codes, offsets = fsx_set()
    alpha, W, M, R, T = b"ATGC-", 6, 2, 300, 6
    gpu_ctx.set_sequences(codes, offsets, alpha)
    other_ctx.set_sequences(codes, offsets, alpha)
    seeds = [7000 + 3 * r for r in range(R)]
    c0, p0, _, st = other_ctx.motif_run_multi_batch(M, W, PC, 1.0, 0, seeds)
    C, P, Q, st = stepwise(other_ctx, M, W, 1.0, T, seeds, c0, p0)
    assert not st.any()
    cnt, pos, pw, status, s = gpu_ctx.motif_run_multi_batch_stats(M, W, PC, 1.0, T, seeds,
                                                                  burn_in=1)
    assert not status.any()
    assert np.array_equal(cnt, C[-1]) and np.array_equal(bits(pw), bits(Q[-1]))
    for r in range(R):
        check_chain(s, r, s["offsets"], M, C, P, Q, list(range(1, T)))
    assert len({o.tobytes() for o in s["occupancy"]}) > 1


@pytest.mark.parametrize("N,cap", [(65, 4), (257, 2)])
def test_a_workgroup_boundary_inside_a_chain(N, cap, other_ctx):
    """N * cap = 260 and 514 list slots a chain: with several statistics workgroups a chain
    (run_stats_blocks 4, and the automatic choice) the 256-slot boundary falls inside it."""
    from gibbssampling_amd import Context
    W, M, T, seeds = 6, 2, 4, [3, 4, 5]
    codes, offsets = make_dataset(N, 50, W, b"ACGT", seed=90 + N, ragged=True, mut=0.1)
    other_ctx.set_sequences(codes, offsets, b"ACGT")
    c0, p0, _, st = other_ctx.motif_run_multi_batch(M, W, PC, 1.0, 0, seeds, cap=cap)
    C, P, Q, st = stepwise(other_ctx, M, W, 1.0, T, seeds, c0, p0, cap=cap)
    assert not st.any()
    for tuning in ({"run_stats_blocks": 4}, {}):
        ctx = Context(0, tuning=tuning)
        ctx.set_sequences(codes, offsets, b"ACGT")
        *_, status, s = ctx.motif_run_multi_batch_stats(M, W, PC, 1.0, T, seeds, cap=cap)
        ctx.close()
        assert not status.any() and s["best_pos"].shape == (3, N, cap)
        for r in range(len(seeds)):
            check_chain(s, r, s["offsets"], M, C, P, Q, list(range(T)))


def test_edges(gpu_ctx, other_ctx):
    from gibbssampling_amd import Context
    alpha, N, L, W, _, M, cutoff, mode, _ = SHAPES["dna-m2"]
    codes, offsets = data("dna-m2")
    ctx = bound(gpu_ctx, "dna-m2")
    cnt0, pos0 = one_lists(init_positions(offsets, W, 9), M)
    cnt0[5] = 0  # one Positions []
    pos0[5] = -1
    two_c, two_p = np.tile(cnt0, (2, 1)), np.tile(pos0, (2, 1, 1))
    kw = dict(first_sweep=2, burn_in=1, thin=2)
    run = ctx.motif_run_multi_batch_stats

    # all statistics null: the bits of gs_motif_run_multi_batch
    plain = ctx.motif_run_multi_batch(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, first_sweep=2)
    c, p, w, st, s = run(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, occupancy=False,
                         sites=False, ic=False, best=False, **kw)
    assert s == {} and not st.any()
    assert same(c, plain[0]) and same(p, plain[1]) and same(w, plain[2])
    ms = ctx.run_multi_batch_last_ms()
    assert len(ms) == 2 and all(np.isfinite(m) and m >= 0.0 for m in ms)
    # ... and so with each of them alone
    full = run(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, **kw)
    for only in ("occupancy", "sites", "ic", "best"):
        flags = {k: k == only for k in ("occupancy", "sites", "ic", "best")}
        part = run(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, **flags, **kw)
        assert same(part[0], plain[0]) and same(part[1], plain[1]) and same(part[2], plain[2])
        assert part[4] and set(part[4]) < set(full[4])
        for k, v in part[4].items():
            assert same(v, full[4][k]), k
    assert full[4]["best_sweep"].min() >= 2 + 1  # absolute sweep numbers
    assert ctx.run_multi_batch_last_info()["arena"] == 2048

    # no sweeps: zero bins, no best, the lists as given
    c, p, _, st, s = run(M, W, PC, cutoff, 0, [31, 32], two_c, two_p)
    assert same(c, two_c) and same(p, two_p) and not st.any()
    assert not s["occupancy"].any() and not s["sites"].any() and s["ic"].shape == (2, 0)
    assert s["best_sweep"].tolist() == [-1, -1]
    # burn_in == n_sweeps: nothing is counted
    c, p, w, st, s = run(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, first_sweep=2, burn_in=5)
    assert same(c, plain[0]) and same(w, plain[2]) and not st.any()
    assert not s["occupancy"].any() and not s["sites"].any() and s["ic"].shape == (2, 0)
    assert s["best_sweep"].tolist() == [-1, -1]
    # no chains: nothing to do
    c, p, w, st, s = run(M, W, PC, cutoff, 3, [])
    assert c.shape == (0, N) and p.shape == (0, N, M) and st.shape == (0,)
    assert s["occupancy"].shape == (0, ctx.occupancy_offsets(W)[-1])
    assert s["sites"].shape == (0, N, M + 1)

    # argument errors before any launch
    before = ctx.stats()
    for bad in ({"burn_in": -1}, {"burn_in": 4}, {"thin": 0}, {"thin": -2}):
        with pytest.raises(_native.ArgumentError):
            run(M, W, PC, cutoff, 3, [1, 2], **bad)
    with pytest.raises(_native.ArgumentError):
        run(M, L + 1, PC, cutoff, 3, [1, 2])
    with pytest.raises(_native.ArgumentError):
        run(M, W, PC, cutoff, -1, [1, 2])
    with pytest.raises(_native.ArgumentError):
        run(3, W, PC, cutoff, 3, [1, 2], cap=2)
    # the best sweep without all three rows, and rows without it
    seeds = np.array([1, 2], np.uint64)
    row_c, row_p = np.zeros((2, N), np.int32), np.zeros((2, N, M), np.int32)
    row_d = np.zeros((2, N), np.float64)
    bs, stw = np.zeros(2, np.int64), np.zeros(2, np.int32)
    P = _native._ptr
    for b, bc, bp, bw in ((bs, row_c, row_p, None), (bs, row_c, None, row_d),
                          (bs, None, row_p, row_d), (bs, None, None, None),
                          (None, row_c, row_p, row_d), (None, None, row_p, None)):
        rc = ctx.lib.gs_motif_run_multi_batch_stats(
            ctx.h, M, W, PC, cutoff, 3, P(seeds), 2, 0, 1, M, None, 0, 1, P(row_c.copy()),
            P(row_p.copy()), P(row_d.copy()), P(stw), None, None, None, P(b), P(bc), P(bp), P(bw))
        assert rc == _native.GS_E_ARG
    assert ctx.stats() == before

    # the sibling's refusals: a fixed PCV on the context
    ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
    try:
        with pytest.raises(_native.GibbsError) as e:
            run(M, W, PC, cutoff, 3, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        ctx.set_fixed_pcv(None)
    assert ctx.stats() == before

    # the launch choices change no bit: one, the automatic number of, or four statistics
    # workgroups a chain, atomic or plain bins
    for tuning in ({"run_stats_blocks": 1, "run_stats_atomic": 0}, {"run_stats_blocks": 0},
                   {"run_stats_blocks": 4, "run_stats_atomic": 1},
                   {"run_stats_blocks": 4, "run_stats_atomic": 0}):
        c2 = Context(0, tuning=tuning)
        c2.set_sequences(codes, offsets, alpha)
        o = c2.motif_run_multi_batch_stats(M, W, PC, cutoff, 5, [31, 32], two_c, two_p, **kw)
        c2.close()
        assert same(o[0], full[0]) and same(o[1], full[1]) and same(o[2], full[2])
        for k, v in full[4].items():
            assert same(o[4][k], v), (tuning, k)

    # a continued call: its bins added to the first call's are one call's of 25 sweeps
    whole = run(M, W, PC, cutoff, 25, SEEDS, init_mode=mode, burn_in=2, thin=3)
    a = run(M, W, PC, cutoff, 10, SEEDS, init_mode=mode, burn_in=2, thin=3)
    # sweeps 2, 5, 8 counted; the next one is 11: burn-in 1 of the continuation
    b = run(M, W, PC, cutoff, 15, SEEDS, a[0], a[1], first_sweep=10, burn_in=1, thin=3)
    assert not whole[3].any() and not a[3].any() and not b[3].any()
    assert same(b[0], whole[0]) and same(b[1], whole[1]) and same(b[2], whole[2])
    for k in ("occupancy", "sites"):
        assert np.array_equal(a[4][k] + b[4][k], whole[4][k]), k
    assert same(np.concatenate([a[4]["ic"], b[4]["ic"]], axis=1), whole[4]["ic"])

    # no snapshot is left behind, and the next single run behaves as on a fresh context
    with pytest.raises(_native.GibbsError) as e:
        ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    bound(other_ctx, "dna-m2")
    fresh = other_ctx.motif_sampling(W, PC, cutoff, 31)
    run(M, W, PC, cutoff, 2, [5, 6], init_mode=1)
    again = ctx.motif_sampling(W, PC, cutoff, 31)
    assert np.array_equal(again[0], fresh[0]) and again[2] == fresh[2]
    assert same(again[1], fresh[1])


def test_mirror_gathers_the_statistics_of_the_list_chains():
    from gibbssampling_amd import ListChainStats, MotifSampler
    from gibbssampling_amd.sampler import createMotifIndex
    N, L, W, T = 40, 60, 7, 8
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=6, mut=0.1)
    sources = [bytes(codes[offsets[i]:offsets[i + 1]]) for i in range(N)]
    seeds = [99, 100, 2**40 + 1]
    mems = [[createMotifIndex(0.0, [] if p < 0 else [p])
             for p in init_positions(offsets, W, 20 + r, 0.1)] for r in range(len(seeds))]
    mems[1][0] = createMotifIndex(0.0, [L - W, 0])
    chains, st = MotifSampler.runSweepsBatchedListStats(W, PC, 1.0, "ACGT", sources, T, seeds,
                                                        mems, first_sweep=3, burn_in=2,
                                                        motifAmount=2)
    plain = MotifSampler.runSweepsBatched(W, PC, 1.0, "ACGT", sources, T, seeds, mems,
                                          first_sweep=3, motifAmount=2)
    assert chains == plain and isinstance(st, ListChainStats)
    assert st.finished().all() and st.sites.shape == (3, N, 3) and st.ic.shape == (3, T - 2)
    for r in range(3):
        b = first_best(st.ic[r].tolist())
        assert st.best_sweep[r] == 3 + 2 + b
        assert informationContent([m.PWMS for m in st.best[r]]) == st.ic[r, b]
    means = [float(m[1:].sum()) for m in st.marginals()]
    want = [float(s @ np.arange(3)) for s in st.siteCounts()]
    assert np.allclose(means, want, rtol=1e-12, atol=0)
    mode = st.mode()
    assert len(mode) == N
    for m, s in zip(mode, st.siteCounts()):
        assert len(m.Positions) <= int(np.argmax(s))
        assert all(abs(a - b) > W for i, a in enumerate(m.Positions) for b in m.Positions[:i])
