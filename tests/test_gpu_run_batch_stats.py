"""GPU parity of gs_motif_run_batch_stats: the chains of gs_motif_run_batch with, per chain,
the occupancy of every motif start over the counted sweeps, the trace of the summed PWMS in
its fixed order, and the best state visited, all gathered on the device.  The reference is
what a caller had to do before: T one-sweep motif_run_batch calls with a numpy tally.
Counts, positions and the chosen sweeps are compared exactly, binary64 values bit for bit;
against the oracle the trace within the PWMS tolerance plus the summation's rounding."""
import numpy as np
import pytest

from conftest import init_positions, make_dataset, uniforms
from gibbssampling_amd import _native
from gibbssampling_amd.sampler import informationContent
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

PC, CUTOFF = 1e-4, 1.0
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
# those of test_gpu_run_batch.py: non-contiguous, one duplicate (rows 1 and 3), one beyond 2^32
SEEDS = [1001, 77, 5_000_000_007, 77, 12]
T_STEP, T_ORACLE = 12, 4

# name: (alphabet, N, L, W, ragged, dataset seed)
SHAPES = {
    "dna": (b"ACGT", 150, 90, 9, True, 77),
    "gap-symbol": (b"ATGC-", 150, 90, 9, True, 79),
    "protein": (PROTEIN, 40, 60, 8, False, 80),
}


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def counted_sweeps(T, burn_in, thin):
    return [t for t in range(T) if t >= burn_in and (t - burn_in) % thin == 0]


def tally(off, states):
    """The histogram of one chain over `states` (position rows, -1 = Positions [])."""
    occ = np.zeros(int(off[-1]), np.int32)
    for p in states:
        np.add.at(occ, off[:-1] + 1 + p, 1)
    return occ


def first_best(ics):
    """(index, value) of the first maximum as .fs:989 takes it: the first entry, replaced
    only by a strictly larger one; -1 for no entry."""
    best = -1
    for i, x in enumerate(ics):
        if best < 0 or x > ics[best]:
            best = i
    return best


_data, _ctx, _steps = {}, {}, {}


def data(name):
    if name not in _data:
        alpha, N, L, W, ragged, dseed = SHAPES[name]
        _data[name] = make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1)
    return _data[name]


def bound(gpu_ctx, name):
    alpha = SHAPES[name][0]
    codes, offsets = data(name)
    gpu_ctx.set_sequences(codes, offsets, alpha)
    return gpu_ctx


def stepwise(gpu_ctx, name):
    """The reference of one shape, computed once and left unchanged: the starts of mode 1,
    T_STEP one-sweep calls (pos = the previous rows, first_sweep = t), and the plain call."""
    if name not in _steps:
        W = SHAPES[name][3]
        ctx = bound(gpu_ctx, name)
        pos, _, st = ctx.motif_run_batch(W, PC, CUTOFF, 0, SEEDS, init_mode=1)
        assert not st.any()
        P, Q = [], []
        for t in range(T_STEP):
            pos, pw, st = ctx.motif_run_batch(W, PC, CUTOFF, 1, SEEDS, pos=pos, first_sweep=t)
            assert not st.any()
            P.append(pos)
            Q.append(pw)
        plain = ctx.motif_run_batch(W, PC, CUTOFF, T_STEP, SEEDS, init_mode=1)
        out = (np.array(P), np.array(Q), plain[0], plain[1], ctx.occupancy_offsets(W))
        for a in out:
            a.setflags(write=False)
        _steps[name] = out
    return _steps[name]


@pytest.mark.parametrize("burn_in,thin", [(0, 1), (3, 1), (3, 2), (12, 1)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_stepwise_loop(name, burn_in, thin, gpu_ctx):
    alpha, N, L, W, _, _ = SHAPES[name]
    P, Q, plain_pos, plain_pw, off = stepwise(gpu_ctx, name)
    ctx = bound(gpu_ctx, name)
    pos, pw, status, s = ctx.motif_run_batch_stats(W, PC, CUTOFF, T_STEP, SEEDS, init_mode=1,
                                                   burn_in=burn_in, thin=thin)
    assert not status.any()
    ts = counted_sweeps(T_STEP, burn_in, thin)
    R = len(SEEDS)
    assert np.array_equal(s["offsets"], off)
    assert s["occupancy"].shape == (R, off[-1]) and s["ic"].shape == (R, len(ts))
    # the chains are those of the plain call, to the bit
    assert np.array_equal(pos, plain_pos) and np.array_equal(bits(pw), bits(plain_pw))
    assert np.array_equal(pos, P[-1]) and np.array_equal(bits(pw), bits(Q[-1]))
    if ts:  # kept motifs and [] entries both occur among the counted states
        kinds = {bool(x) for x in (P[ts] >= 0).ravel()}
        assert kinds == {True, False}
    for r in range(R):
        want = tally(off, [P[t][r] for t in ts])
        assert np.array_equal(s["occupancy"][r], want), r
        # every sequence's bins sum to n_counted
        per_seq = np.add.reduceat(s["occupancy"][r], off[:-1])
        assert np.array_equal(per_seq, np.full(N, len(ts))), r
        ics = [informationContent(Q[t][r]) for t in ts]
        assert np.array_equal(bits(s["ic"][r]), bits(ics)), r
        b = first_best(ics)
        if b < 0:
            assert s["best_sweep"][r] == -1
            continue
        assert s["best_sweep"][r] == ts[b], r
        assert np.array_equal(s["best_pos"][r], P[ts[b]][r]), r
        assert np.array_equal(bits(s["best_pwms"][r]), bits(Q[ts[b]][r])), r
    # the duplicate seed: identical rows
    for k in ("occupancy", "ic", "best_sweep", "best_pos"):
        assert np.array_equal(s[k][1], s[k][3], equal_nan=k == "ic"), k
    assert np.array_equal(bits(s["best_pwms"][1]), bits(s["best_pwms"][3]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_against_the_oracle(name, gpu_ctx):
    alpha, N, L, W, _, _ = SHAPES[name]
    codes, offsets = data(name)
    ctx = bound(gpu_ctx, name)
    _, _, status, s = ctx.motif_run_batch_stats(W, PC, CUTOFF, T_ORACLE, SEEDS, init_mode=1)
    assert not status.any()
    off = s["offsets"]
    S = ol.Seqs(codes, offsets, alpha)
    decided = 0
    for seed in sorted(set(SEEDS)):
        _, p = ol.random_starts(S, W, PC, seed=seed, mode=1)
        states, sums, tols = [], [], []
        for t in range(T_ORACLE):
            p, w, _ = ol.sweep(S, W, PC, CUTOFF, p, uniforms(seed, ol.stream_sweep(t), N))
            states.append(p)
            sums.append(float(np.sum(w)))
            # the project's PWMS tolerance plus the rounding of a sum of N terms
            tols.append((1e-12 + N * 2.0**-52) * float(np.sum(np.abs(w))))
        ob = first_best(sums)
        # the oracle's best is decided when it leads every other sweep by more than both
        # sides' error: each trace entry is within its tol of the oracle's sum
        clear = all(abs(sums[ob] - sums[t]) > tols[ob] + tols[t]
                    for t in range(T_ORACLE) if t != ob)
        for r in [i for i, x in enumerate(SEEDS) if x == seed]:
            assert np.array_equal(s["occupancy"][r], tally(off, states)), (seed, r)
            for t in range(T_ORACLE):
                assert abs(s["ic"][r, t] - sums[t]) <= tols[t], (seed, r, t)
            if clear:
                decided += 1
                assert s["best_sweep"][r] == ob, (seed, r)
                assert np.array_equal(s["best_pos"][r], states[ob]), (seed, r)
    assert decided > 0  # the comparison of the best sweep took place


def test_the_first_maximum_wins_a_tie(gpu_ctx):
    """With a cut-off nothing passes, every chain sits in the all-[] state from sweep 1 on;
    the same uniforms every sweep then give the same PWMS row, and the trace ties."""
    alpha, N, L, W, _, _ = SHAPES["dna"]
    ctx = bound(gpu_ctx, "dna")
    R, T, first = len(SEEDS), 6, 40
    u = np.repeat(np.random.default_rng(3).random((R, 1, N)), T, axis=1)
    pos, _, status, s = ctx.motif_run_batch_stats(W, PC, 1e300, T, SEEDS, init_mode=1,
                                                  first_sweep=first, u=u, burn_in=1)
    assert not status.any() and (pos == -1).all()
    for r in range(R):
        assert len(set(bits(s["ic"][r]).tolist())) == 1, r  # ties really occurred
        assert s["best_sweep"][r] == first + 1, r
        assert (s["best_pos"][r] == -1).all()
    assert np.array_equal(s["occupancy"][:, s["offsets"][:-1]], np.full((R, N), T - 1))


def test_a_raising_chain_stops_counting(gpu_ctx):
    R, T, N, W = 3, 4, 30, 6
    codes, offsets = make_dataset(N, 40, W, seed=51)
    p0 = init_positions(offsets, W, 52)
    u = np.random.default_rng(53).random((R, T, N))
    u[1, 1, 7] = 2.0  # beyond every category: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, b"ACGT")
    starts = np.tile(p0, (R, 1))
    _, _, status, s = gpu_ctx.motif_run_batch_stats(W, PC, CUTOFF, T, [1, 2, 3], pos=starts, u=u)
    assert status.tolist() == [0, _native.GS_E_ROULETTE_OVERRUN, 0]
    # chain 1: exactly the state of sweep 0
    p1, w1, st1 = gpu_ctx.motif_run_batch(W, PC, CUTOFF, 1, [2], pos=starts[1:2], u=u[1:2, :1])
    assert not st1.any()
    off = s["offsets"]
    assert np.array_equal(s["occupancy"][1], tally(off, [p1[0]]))
    assert bits(s["ic"][1, :1])[0] == bits([informationContent(w1[0])])[0]
    assert np.isnan(s["ic"][1, 1:]).all() and not np.isnan(s["ic"][1, 0])
    assert s["best_sweep"][1] == 0
    assert np.array_equal(s["best_pos"][1], p1[0])
    assert np.array_equal(bits(s["best_pwms"][1]), bits(w1[0]))
    # chains 0 and 2: the same call without chain 1
    po, wo, sto, so = gpu_ctx.motif_run_batch_stats(W, PC, CUTOFF, T, [1, 3], pos=starts[[0, 2]],
                                                    u=u[[0, 2]])
    assert not sto.any()
    for k in ("occupancy", "best_sweep", "best_pos"):
        assert np.array_equal(s[k][[0, 2]], so[k]), k
    for k in ("ic", "best_pwms"):
        assert np.array_equal(bits(s[k][[0, 2]]), bits(so[k])), k
    assert not np.isnan(so["ic"]).any()


def test_edges(gpu_ctx):
    from gibbssampling_amd import Context
    alpha, N, L, W, _, _ = SHAPES["dna"]
    codes, offsets = data("dna")
    ctx = bound(gpu_ctx, "dna")
    p0 = np.tile(init_positions(offsets, W, 9, 0.2), (2, 1))

    # the bins follow the formula on ragged lengths
    lens = np.diff(offsets)
    want = np.concatenate([[0], np.cumsum(1 + (lens - W + 1))])
    assert len(set(lens.tolist())) > 1
    assert np.array_equal(ctx.occupancy_offsets(W), want)
    assert ctx.lib.gs_occupancy_size(ctx.h, W) == want[-1]
    assert ctx.lib.gs_occupancy_size(ctx.h, int(lens.min()) + 1) == -1
    assert ctx.lib.gs_occupancy_size(ctx.h, 0) == -1
    with pytest.raises(_native.ArgumentError):
        ctx.occupancy_offsets(int(lens.min()) + 1)

    # all statistics null: the bits of gs_motif_run_batch
    plain = ctx.motif_run_batch(W, PC, CUTOFF, 5, [31, 32], pos=p0, first_sweep=2)
    pos, pw, st, s = ctx.motif_run_batch_stats(W, PC, CUTOFF, 5, [31, 32], pos=p0, first_sweep=2,
                                               burn_in=1, thin=2, occupancy=False, ic=False,
                                               best=False)
    assert s == {} and not st.any()
    assert np.array_equal(pos, plain[0]) and np.array_equal(bits(pw), bits(plain[1]))
    # ... and so with only some of them
    full = ctx.motif_run_batch_stats(W, PC, CUTOFF, 5, [31, 32], pos=p0, first_sweep=2,
                                     burn_in=1, thin=2)
    for kw in ({"ic": False, "best": False}, {"occupancy": False, "best": False},
               {"occupancy": False, "ic": False}):
        part = ctx.motif_run_batch_stats(W, PC, CUTOFF, 5, [31, 32], pos=p0, first_sweep=2,
                                         burn_in=1, thin=2, **kw)
        assert np.array_equal(part[0], plain[0]) and np.array_equal(bits(part[1]), bits(plain[1]))
        assert part[3] and set(part[3]) < set(full[3])
        for k, v in part[3].items():
            assert np.array_equal(bits(v) if v.dtype == np.float64 else v,
                                  bits(full[3][k]) if v.dtype == np.float64 else full[3][k]), k
    assert full[3]["best_sweep"].min() >= 2 + 1  # absolute sweep numbers

    # no sweeps: zero bins, no best, the positions as given
    pos, _, st, s = ctx.motif_run_batch_stats(W, PC, CUTOFF, 0, [31, 32], pos=p0)
    assert np.array_equal(pos, p0) and not st.any()
    assert not s["occupancy"].any() and s["ic"].shape == (2, 0)
    assert s["best_sweep"].tolist() == [-1, -1]
    # no chains: nothing to do
    pos, pw, st, s = ctx.motif_run_batch_stats(W, PC, CUTOFF, 3, [])
    assert pos.shape == (0, N) and st.shape == (0,) and s["occupancy"].shape == (0, want[-1])

    # argument errors before any launch
    before = ctx.stats()
    for kw in ({"burn_in": -1}, {"burn_in": 4}, {"thin": 0}, {"thin": -2}):
        with pytest.raises(_native.ArgumentError):
            ctx.motif_run_batch_stats(W, PC, CUTOFF, 3, [1, 2], **kw)
    with pytest.raises(_native.ArgumentError):
        ctx.motif_run_batch_stats(L + 1, PC, CUTOFF, 3, [1, 2])
    with pytest.raises(_native.ArgumentError):
        ctx.motif_run_batch_stats(W, PC, CUTOFF, -1, [1, 2])
    # the best sweep without both rows, and rows without it
    seeds = np.array([1, 2], np.uint64)
    row_i, row_d = np.zeros((2, N), np.int32), np.zeros((2, N), np.float64)
    bs, stw = np.zeros(2, np.int64), np.zeros(2, np.int32)
    P = _native._ptr
    for b, bp, bw in ((bs, row_i, None), (bs, None, row_d), (bs, None, None), (None, row_i, row_d),
                      (None, row_i, None)):
        rc = ctx.lib.gs_motif_run_batch_stats(
            ctx.h, W, PC, CUTOFF, 3, P(seeds), 2, 0, 1, None, 0, 1, P(row_i.copy()), P(row_d.copy()),
            P(stw), None, None, P(b), P(bp), P(bw))
        assert rc == _native.GS_E_ARG
    assert ctx.stats() == before

    # the sibling's refusals: a fixed PCV on the context
    ctx.set_fixed_pcv(np.full(49, 1.0 / 49))
    try:
        with pytest.raises(_native.GibbsError) as e:
            ctx.motif_run_batch_stats(W, PC, CUTOFF, 3, [1, 2])
        assert e.value.status == _native.GS_E_UNSUPPORTED
    finally:
        ctx.set_fixed_pcv(None)

    # the launch choices change no bit: aggregate rows cleared by a memset or in-kernel,
    # one or many statistics workgroups a chain, atomic or plain bins
    for tuning in ({"run_batch_clear": 0}, {"run_batch_clear": 1, "run_stats_blocks": 1},
                   {"run_stats_blocks": 7, "run_stats_atomic": 0}):
        c2 = Context(0, tuning=tuning)
        c2.set_sequences(codes, offsets, alpha)
        other = c2.motif_run_batch_stats(W, PC, CUTOFF, 5, [31, 32], pos=p0, first_sweep=2,
                                         burn_in=1, thin=2)
        c2.close()
        assert np.array_equal(other[0], full[0]) and np.array_equal(bits(other[1]), bits(full[1]))
        for k, v in full[3].items():
            assert np.array_equal(bits(v) if v.dtype == np.float64 else v,
                                  bits(other[3][k]) if v.dtype == np.float64 else other[3][k]), k

    # no snapshot is left behind, and the next single run behaves as on a fresh context
    with pytest.raises(_native.GibbsError) as e:
        ctx.get_state()
    assert e.value.status == _native.GS_E_STATE
    fresh_ctx = Context(0)
    fresh_ctx.set_sequences(codes, offsets, alpha)
    fresh = fresh_ctx.motif_sampling(W, PC, CUTOFF, 31)
    fresh_ctx.close()
    ctx.motif_run_batch_stats(W, PC, CUTOFF, 2, [5, 6], init_mode=1)
    again = ctx.motif_sampling(W, PC, CUTOFF, 31)
    assert np.array_equal(again[0], fresh[0]) and again[2] == fresh[2]
    assert np.array_equal(bits(again[1]), bits(fresh[1]))
