"""GPU parity of gs_run_sweeps_stats / gs_motif_run_stats: the single chain of gs_run_sweeps
with the occupancy of every motif start over the counted sweeps, the trace of the summed
PWMS in its fixed order and the best state visited, gathered on the device behind the sweeps
of every sweep kernel.  The reference is what a caller had to do before: one-sweep
run_sweeps calls with get_state and a numpy tally, on a second context with the same tuning.
Counts, positions and the chosen sweeps are compared exactly, binary64 values bit for bit;
where the two sides may run different kernels (automatic choice, the oracle, the chain
batch) the trace within the PWMS tolerance plus the summation's rounding."""
import numpy as np
import pytest

from conftest import uniforms
from gibbssampling_amd import Context, _native
from gibbssampling_amd.sampler import informationContent
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

PC, CUTOFF, SEED, T = 1e-4, 1.0, 4242, 12
DNA = b"ACGT"
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
NO_BG = {"bg_mode": 0}

# name: tuning (both sides), alphabet, N, lengths (lo, hi), W, (burn_in, thin), what must have
# run: the kernel's name, fields of the last gs_sweep_kernel launch, all-background targets;
# keeps: the counted states hold kept motifs (the chains start from getPWMOfRandomStarts)
CASES = {
    "ek4_one": dict(tuning={"dna_mode": 0, "sweep_one": 1, **NO_BG}, alpha=DNA, N=2049, L=(64, 64),
                    W=12, count=(0, 1), kernel="gs_sweep_kernel", launch={"ek": 4, "one": 1}, keeps=True),
    "ek4_loop": dict(tuning={"dna_mode": 0, "sweep_one": 0, **NO_BG}, alpha=DNA, N=257, L=(24, 64),
                     W=4, count=(3, 1), kernel="gs_sweep_kernel", launch={"ek": 4, "one": 0}),
    "dna": dict(tuning={"dna_mode": 1, "live_mode": 0, "long_mode": 0, **NO_BG}, alpha=DNA, N=65,
                L=(24, 64), W=12, count=(2, 3), kernel="gs_sweep_dna_kernel", keeps=True),
    "live": dict(tuning={"live_mode": 1, "long_mode": 0, **NO_BG}, alpha=DNA, N=2049, L=(24, 64),
                 W=4, count=(2, 3), kernel="gs_sweep_live_kernel"),
    "long": dict(tuning={"dna_mode": 1, "long_mode": 1, **NO_BG}, alpha=DNA, N=257, L=(64, 64),
                 W=12, count=(0, 1), kernel="gs_sweep_long_kernel", keeps=True),
    "protein": dict(tuning=dict(NO_BG), alpha=PROTEIN, N=65, L=(40, 40), W=4, count=(3, 1),
                    kernel="gs_sweep_kernel", launch={"ek": 0}),
    "bg": dict(tuning={"bg_mode": 1}, alpha=DNA, N=257, L=(24, 64), W=12, count=(3, 1), bg=True),
    "one_sequence": dict(tuning={"dna_mode": 0, **NO_BG}, alpha=DNA, N=1, L=(30, 30), W=4,
                         count=(0, 1), kernel="gs_sweep_kernel"),
    # from 32 768 targets on the best rows are copied by a launch of their own
    "two_launches": dict(tuning=dict(NO_BG), alpha=DNA, N=32768, L=(24, 40), W=12, count=(3, 1)),
    "five": dict(tuning={"dna_mode": 0, **NO_BG}, alpha=DNA, N=5, L=(24, 64), W=12, count=(12, 1),
                 kernel="gs_sweep_kernel"),
}


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def counted_sweeps(n, burn_in, thin):
    return [t for t in range(n) if t >= burn_in and (t - burn_in) % thin == 0]


def tally(off, states):
    """The histogram of a chain over `states` (position rows, -1 = Positions [])."""
    occ = np.zeros(int(off[-1]), np.int32)
    for p in states:
        np.add.at(occ, off[:-1] + 1 + p, 1)
    return occ


def first_best(ics):
    """The index of the first maximum as .fs:989 takes it: the first entry, replaced only
    by a strictly larger one; -1 for no entry."""
    best = -1
    for i, x in enumerate(ics):
        if best < 0 or x > ics[best]:
            best = i
    return best


def trace_bound(pw):
    """The project's PWMS tolerance plus the rounding of a sum of N terms."""
    return (1e-12 + len(pw) * 2.0 ** -52) * float(np.sum(np.abs(pw)))


def dataset(N, lo, hi, W, alpha, seed, planted=True):
    """i.i.d. symbols with one 10 % mutated copy of a consensus W-mer a sequence, lengths
    uniform in [lo, hi]; starts with a fifth of the sequences at Positions []."""
    rng = np.random.default_rng(seed)
    a = np.frombuffer(alpha, np.uint8)
    lens = rng.integers(lo, hi + 1, N)
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    codes = a[rng.integers(0, len(a), int(offsets[-1]))].astype(np.uint8)
    if planted:
        cons = a[rng.integers(0, len(a), W)]
        at = offsets[:-1] + (rng.random(N) * (lens - W + 1)).astype(np.int64)
        motif = np.tile(cons, (N, 1))
        flip = rng.random((N, W)) < 0.1
        motif[flip] = a[rng.integers(0, len(a), int(flip.sum()))]
        codes[at[:, None] + np.arange(W)[None, :]] = motif
    pos = (rng.random(N) * (lens - W + 1)).astype(np.int32)
    if N > 1:
        pos[rng.random(N) < 0.2] = -1
    return codes, offsets, pos


class Pair:
    """The two sides of one case: the context of the statistics call and the stepwise one,
    with the same tuning and sequences."""

    def __init__(self, tuning, alpha, codes, offsets):
        self.stat = Context(0, tuning=tuning)
        self.step = Context(0, tuning=tuning)
        for c in (self.stat, self.step):
            c.set_sequences(codes, offsets, alpha)

    def close(self):
        self.stat.close()
        self.step.close()


def stepwise(ctx, W, p0, n, first=0, pc=PC, cutoff=CUTOFF, seed=SEED):
    """n one-sweep run_sweeps calls, each followed by get_state -> (P[n, N], Q[n, N])."""
    ctx.set_positions(W, p0)
    P, Q = [], []
    for t in range(n):
        ctx.run_sweeps(pc, cutoff, 1, seed, first_sweep=first + t)
        pos, pw = ctx.get_state()
        P.append(pos)
        Q.append(pw)
    P, Q = np.array(P).reshape(n, len(p0)), np.array(Q).reshape(n, len(p0))
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q


def check_exact(s, P, Q, off, burn_in, thin, first=0):
    """The statistics against the stepwise states, everything exact."""
    n = len(P)
    ts = counted_sweeps(n, burn_in, thin)
    assert np.array_equal(s["offsets"], off)
    assert s["occupancy"].shape == (off[-1],) and s["ic"].shape == (len(ts),)
    assert np.array_equal(s["occupancy"], tally(off, [P[t] for t in ts]))
    assert np.array_equal(np.add.reduceat(s["occupancy"], off[:-1]), np.full(P.shape[1], len(ts)))
    ics = [informationContent(Q[t]) for t in ts]
    assert np.array_equal(bits(s["ic"]), bits(ics))
    b = first_best(ics)
    if b < 0:
        assert s["best_sweep"][0] == -1
        return
    assert s["best_sweep"][0] == first + ts[b]
    assert np.array_equal(s["best_pos"], P[ts[b]])
    assert np.array_equal(bits(s["best_pwms"]), bits(Q[ts[b]]))
    assert bits([informationContent(s["best_pwms"])])[0] == bits(s["ic"][b:b + 1])[0]


def ran(ctx, spec, n_targets, before):
    """The intended kernel ran (since `before`, the context's earlier gs_stats)."""
    if spec.get("bg"):
        assert ctx.stats()["bg_path"] - before["bg_path"] == n_targets
        return
    if "kernel" not in spec:
        return
    assert ctx.sweep_kernel_name() == spec["kernel"]
    if spec["kernel"] == "gs_sweep_kernel":
        launch = ctx.last_sweep_launch()
        for k, v in spec.get("launch", {}).items():
            assert launch[k] == v, launch


@pytest.mark.parametrize("name", list(CASES))
def test_every_kernel_against_the_stepwise_loop(name):
    spec = CASES[name]
    N, W, (burn_in, thin) = spec["N"], spec["W"], spec["count"]
    codes, offsets, p0 = dataset(N, *spec["L"], W, spec["alpha"], seed=len(name) + N)
    if spec.get("bg"):
        p0 = np.full(N, -1, np.int32)  # the all-background state from the start
    pair = Pair(spec["tuning"], spec["alpha"], codes, offsets)
    try:
        if N >= 65 and not spec.get("bg"):  # starts that hold a motif, as doMotifSampling's
            p0 = pair.step.random_starts(W, PC, SEED, 1)[1]
        s0 = pair.step.stats()
        P, Q = stepwise(pair.step, W, p0, T)
        ran(pair.step, spec, N * T, s0)
        off = pair.step.occupancy_offsets(W)
        s0 = pair.stat.stats()
        pos, pw, s = pair.stat.motif_run_stats(W, PC, CUTOFF, T, SEED, p0, burn_in=burn_in, thin=thin)
        ran(pair.stat, spec, N * T, s0)
        # the chain is the stepwise one, to the bit
        assert np.array_equal(pos, P[-1]) and np.array_equal(bits(pw), bits(Q[-1]))
        check_exact(s, P, Q, off, burn_in, thin)
        ts = counted_sweeps(T, burn_in, thin)
        if ts and ts[-1] == T - 1:
            assert bits([informationContent(pw)])[0] == bits(s["ic"][-1:])[0]
        if spec.get("bg"):  # the [] bins fill
            assert np.array_equal(s["occupancy"][off[:-1]], np.full(N, len(ts)))
        elif spec.get("keeps"):
            assert (P[ts] >= 0).any()
        # the snapshot stays: the state is there again, and the chain goes on from it
        again = pair.stat.get_state()
        assert np.array_equal(again[0], pos) and np.array_equal(bits(again[1]), bits(pw))
    finally:
        pair.close()


def test_automatic_kernel_choice():
    """bg_mode -1: a chain without motifs falls into the all-background state, and the two
    sides may hand over to the all-background kernel at different sweeps."""
    N, W = 2049, 12
    codes, offsets, p0 = dataset(N, 24, 64, W, DNA, seed=7, planted=False)
    pair = Pair({}, DNA, codes, offsets)
    try:
        P, Q = stepwise(pair.step, W, p0, T)
        pos, pw, s = pair.stat.motif_run_stats(W, PC, CUTOFF, T, SEED, p0, burn_in=2, thin=1)
        ts = counted_sweeps(T, 2, 1)
        off = s["offsets"]
        assert np.array_equal(pos, P[-1])
        assert np.array_equal(s["occupancy"], tally(off, [P[t] for t in ts]))
        for i, t in enumerate(ts):
            assert abs(s["ic"][i] - informationContent(Q[t])) <= trace_bound(Q[t]), t
    finally:
        pair.close()


def test_against_the_oracle(gpu_ctx):
    N, W, n = 257, 12, 4
    codes, offsets, p0 = dataset(N, 24, 64, W, DNA, seed=11)
    S = ol.Seqs(codes, offsets, DNA)
    p0 = ol.random_starts(S, W, PC, seed=SEED, mode=1)[1].astype(np.int32)
    states, rows, p = [], [], p0
    for t in range(n):
        p, w, _ = ol.sweep(S, W, PC, CUTOFF, p, uniforms(SEED, ol.stream_sweep(t), N))
        states.append(p)
        rows.append(w)
    gpu_ctx.set_sequences(codes, offsets, DNA)
    pos, pw, s = gpu_ctx.motif_run_stats(W, PC, CUTOFF, n, SEED, p0)
    assert np.array_equal(pos, states[-1])
    assert np.array_equal(s["occupancy"], tally(s["offsets"], states))
    for t in range(n):
        assert abs(s["ic"][t] - float(np.sum(rows[t]))) <= trace_bound(rows[t]), t
    sums = [float(np.sum(w)) for w in rows]
    ob = first_best(sums)
    if all(abs(sums[ob] - sums[t]) > trace_bound(rows[ob]) + trace_bound(rows[t])
           for t in range(n) if t != ob):  # the oracle's best leads by more than both errors
        assert s["best_sweep"][0] == ob and np.array_equal(s["best_pos"], states[ob])


def test_the_first_maximum_wins_a_tie(gpu_ctx):
    """With a cut-off nothing passes the chain sits in the all-[] state from sweep 1 on; the
    same uniforms every sweep then give the same PWMS row, and the trace ties."""
    N, W, n, first = 65, 9, 6, 40
    codes, offsets, p0 = dataset(N, 24, 64, W, DNA, seed=13)
    u = np.repeat(np.random.default_rng(3).random((1, N)), n, axis=0)
    gpu_ctx.set_sequences(codes, offsets, DNA)
    pos, _, s = gpu_ctx.motif_run_stats(W, PC, 1e300, n, SEED, p0, first_sweep=first, u=u, burn_in=1)
    assert (pos == -1).all()
    assert len(set(bits(s["ic"]).tolist())) == 1  # ties really occurred
    assert s["best_sweep"][0] == first + 1 and (s["best_pos"] == -1).all()
    assert np.array_equal(s["occupancy"][s["offsets"][:-1]], np.full(N, n - 1))


def test_a_raising_chain_stops_counting(gpu_ctx):
    N, W, n = 65, 6, 4
    codes, offsets, p0 = dataset(N, 24, 64, W, DNA, seed=17)
    u = np.random.default_rng(53).random((n, N))
    u[1, :] = 1.0  # past every category somewhere: the reference's list index overruns
    gpu_ctx.set_sequences(codes, offsets, DNA)
    p1, w1 = gpu_ctx.motif_sweep(W, PC, CUTOFF, p0, u[0])
    with pytest.raises(_native.RouletteOverrunError):
        gpu_ctx.motif_sweep(W, PC, CUTOFF, p1, u[1])
    gpu_ctx.set_positions(W, p0)
    s = gpu_ctx.run_sweeps_stats(PC, CUTOFF, n, SEED, u=u, strict=False)
    assert s["status"] == _native.GS_E_ROULETTE_OVERRUN
    assert np.array_equal(s["occupancy"], tally(s["offsets"], [p1]))
    assert bits(s["ic"][:1])[0] == bits([informationContent(w1)])[0]
    assert np.isnan(s["ic"][1:]).all()
    assert s["best_sweep"][0] == 0 and np.array_equal(s["best_pos"], p1)
    assert np.array_equal(bits(s["best_pwms"]), bits(w1))
    # the context is left as run_sweeps + synchronize leave it after the error: the error
    # sticks until the next snapshot, and there is no snapshot
    with pytest.raises(_native.RouletteOverrunError):
        gpu_ctx.get_state()
    assert gpu_ctx.lib.gs_state_motif_length(gpu_ctx.h) == 0
    # ... and the strict call raises the mapped exception
    gpu_ctx.set_positions(W, p0)
    with pytest.raises(_native.RouletteOverrunError):
        gpu_ctx.run_sweeps_stats(PC, CUTOFF, n, SEED, u=u)


def test_under_a_fixed_pcv():
    N, W = 257, 9
    codes, offsets, p0 = dataset(N, 24, 64, W, DNA, seed=19)
    pcv = np.zeros(49)
    pcv[[c - 42 for c in DNA]] = [0.1, 0.2, 0.3, 0.4]
    pair = Pair(dict(NO_BG), DNA, codes, offsets)
    try:
        for c in (pair.stat, pair.step):
            c.set_fixed_pcv(pcv)
        p0 = pair.step.random_starts(W, PC, SEED, 1)[1]
        P, Q = stepwise(pair.step, W, p0, T)
        off = pair.step.occupancy_offsets(W)
        pos, pw, s = pair.stat.motif_run_stats(W, PC, CUTOFF, T, SEED, p0, burn_in=3, thin=2)
        assert np.array_equal(pos, P[-1]) and np.array_equal(bits(pw), bits(Q[-1]))
        check_exact(s, P, Q, off, 3, 2)
    finally:
        pair.close()


def same_stats(a, b, keys=None):
    for k in keys or [k for k in a if k != "status"]:
        assert np.array_equal(bits(a[k]) if a[k].dtype == np.float64 else a[k],
                              bits(b[k]) if b[k].dtype == np.float64 else b[k]), k


N_E, W_E = 257, 9


@pytest.fixture(scope="module")
def edge():
    """The edges' data, their context, and the full statistics of one 7-sweep call."""
    codes, offsets, p0 = dataset(N_E, 24, 64, W_E, DNA, seed=23)
    ctx = Context(0, tuning=dict(NO_BG))
    ctx.set_sequences(codes, offsets, DNA)
    p0 = ctx.random_starts(W_E, PC, SEED, 1)[1]  # starts that hold a motif
    pos, pw, full = ctx.motif_run_stats(W_E, PC, CUTOFF, 7, SEED, p0, first_sweep=2, burn_in=1, thin=2)
    yield codes, offsets, p0, ctx, (pos, pw, full)
    ctx.close()


def test_all_statistics_null_is_run_sweeps(edge):
    codes, offsets, p0, ctx, (pos, pw, full) = edge
    ctx.set_positions(W_E, p0)
    ctx.run_sweeps(PC, CUTOFF, 7, SEED, first_sweep=2)
    plain = ctx.get_state()
    ctx.set_positions(W_E, p0)
    s = ctx.run_sweeps_stats(PC, CUTOFF, 7, SEED, first_sweep=2, burn_in=1, thin=2,
                             occupancy=False, ic=False, best=False)
    assert s == {"status": 0}
    got = ctx.get_state()
    assert np.array_equal(got[0], plain[0]) and np.array_equal(bits(got[1]), bits(plain[1]))
    assert np.array_equal(pos, plain[0]) and np.array_equal(bits(pw), bits(plain[1]))
    assert full["best_sweep"][0] >= 2 + 1  # absolute sweep numbers
    # each statistic alone: the chain and that statistic as in the full call
    for kw in ({"ic": False, "best": False}, {"occupancy": False, "best": False},
               {"occupancy": False, "ic": False}):
        p, w, part = ctx.motif_run_stats(W_E, PC, CUTOFF, 7, SEED, p0, first_sweep=2, burn_in=1,
                                         thin=2, **kw)
        assert np.array_equal(p, pos) and np.array_equal(bits(w), bits(pw))
        assert set(part) < set(full)
        same_stats(part, full)


def test_no_sweeps_and_no_counted_sweep(edge):
    codes, offsets, p0, ctx, _ = edge
    pos, _, s = ctx.motif_run_stats(W_E, PC, CUTOFF, 0, SEED, p0)
    assert np.array_equal(pos, p0)
    assert not s["occupancy"].any() and s["ic"].shape == (0,) and s["best_sweep"][0] == -1
    plain = ctx.motif_run(W_E, PC, CUTOFF, 5, SEED, p0)
    pos, pw, s = ctx.motif_run_stats(W_E, PC, CUTOFF, 5, SEED, p0, burn_in=5)
    assert np.array_equal(pos, plain[0]) and np.array_equal(bits(pw), bits(plain[1]))
    assert not s["occupancy"].any() and s["ic"].shape == (0,) and s["best_sweep"][0] == -1


def test_refusals_come_before_any_launch(edge):
    codes, offsets, p0, ctx, _ = edge
    ctx.set_positions(W_E, p0)
    ctx.synchronize()
    before, state = ctx.stats(), ctx.get_state()
    P = _native._ptr
    H = int(ctx.occupancy_offsets(W_E)[-1])
    occ, ic = np.zeros(H, np.int32), np.zeros(16, np.float64)
    bs, bp, bw = np.zeros(1, np.int64), np.zeros(N_E, np.int32), np.zeros(N_E, np.float64)

    def call(c, n=3, first=0, burn_in=0, thin=1, occ_=None, ic_=None, b=None, bp_=None, bw_=None):
        return c.lib.gs_run_sweeps_stats(c.h, PC, CUTOFF, n, SEED, first, None, burn_in, thin,
                                         P(occ_), P(ic_), P(b), P(bp_), P(bw_))

    for kw in ({"n": -1}, {"first": -1}, {"burn_in": -1}, {"burn_in": 4}, {"thin": 0}, {"thin": -2},
               {"b": bs, "bp_": bp}, {"b": bs, "bw_": bw}, {"b": bs}, {"bp_": bp, "bw_": bw},
               {"bp_": bp}):
        assert call(ctx, occ_=occ, ic_=ic, **kw) == _native.GS_E_ARG, kw
    for kw in ({"burn_in": -1}, {"burn_in": 4}, {"thin": 0}):
        with pytest.raises(_native.ArgumentError):
            ctx.run_sweeps_stats(PC, CUTOFF, 3, SEED, **kw)
        with pytest.raises(_native.ArgumentError):
            ctx.motif_run_stats(W_E, PC, CUTOFF, 3, SEED, p0, **kw)
    # a trace beyond what a call may hold (refused: nothing is written to ic)
    assert call(ctx, n=2**31 - 1, ic_=ic) == _native.GS_E_UNSUPPORTED
    assert ctx.stats() == before
    got = ctx.get_state()  # the snapshot is untouched
    assert np.array_equal(got[0], state[0]) and np.array_equal(bits(got[1]), bits(state[1]))
    # no snapshot
    fresh = Context(0)
    try:
        fresh.set_sequences(codes, offsets, DNA)
        assert call(fresh, occ_=occ) == _native.GS_E_STATE
        with pytest.raises(_native.GibbsError) as e:
            fresh.run_sweeps_stats(PC, CUTOFF, 3, SEED)
        assert e.value.status == _native.GS_E_STATE
        # sharded sequences: the trace needs every sequence
        fresh.set_sequences(codes, offsets, DNA, n_global=N_E + 5)
        fresh.set_positions(W_E, p0)
        fresh.synchronize()
        before = fresh.stats()
        assert call(fresh, occ_=occ, ic_=ic) == _native.GS_E_UNSUPPORTED
        with pytest.raises(_native.GibbsError) as e:
            fresh.motif_run_stats(W_E, PC, CUTOFF, 3, SEED, p0)
        assert e.value.status == _native.GS_E_UNSUPPORTED
        assert fresh.stats() == before
    finally:
        fresh.close()


@pytest.mark.parametrize("tuning", [{"run_stats_blocks": 1}, {"run_stats_blocks": 4},
                                    {"run_stats_atomic": 0}, {"run_stats_blocks": 1, "run_stats_atomic": 0},
                                    {"graph_mode": 1}])
def test_the_launch_choices_change_no_bit(edge, tuning):
    codes, offsets, p0, ctx, (pos, pw, full) = edge
    assert ctx.get_tuning("run_stats_blocks") == 0 and ctx.get_tuning("run_stats_atomic") == 1
    c2 = Context(0, tuning={**NO_BG, **tuning})
    try:
        c2.set_sequences(codes, offsets, DNA)
        p, w, other = c2.motif_run_stats(W_E, PC, CUTOFF, 7, SEED, p0, first_sweep=2, burn_in=1, thin=2)
    finally:
        c2.close()
    assert np.array_equal(p, pos) and np.array_equal(bits(w), bits(pw))
    same_stats(other, full)


def test_a_continued_call_adds_up(edge):
    codes, offsets, p0, ctx, _ = edge
    _, _, whole = ctx.motif_run_stats(W_E, PC, CUTOFF, T, SEED, p0)
    ctx.set_positions(W_E, p0)
    a = ctx.run_sweeps_stats(PC, CUTOFF, 5, SEED)
    b = ctx.run_sweeps_stats(PC, CUTOFF, T - 5, SEED, first_sweep=5)
    assert np.array_equal(a["occupancy"] + b["occupancy"], whole["occupancy"])
    assert np.array_equal(bits(np.concatenate([a["ic"], b["ic"]])), bits(whole["ic"]))
    assert whole["best_sweep"][0] in (a["best_sweep"][0], b["best_sweep"][0])
    # a plain run_sweeps goes on from the statistics call's snapshot as well
    ctx.set_positions(W_E, p0)
    ctx.run_sweeps_stats(PC, CUTOFF, 5, SEED)
    ctx.run_sweeps(PC, CUTOFF, T - 5, SEED, first_sweep=5)
    plain = ctx.motif_run(W_E, PC, CUTOFF, T, SEED, p0)
    ctx.set_positions(W_E, p0)
    ctx.run_sweeps_stats(PC, CUTOFF, 5, SEED)
    ctx.run_sweeps(PC, CUTOFF, T - 5, SEED, first_sweep=5)
    got = ctx.get_state()
    assert np.array_equal(got[0], plain[0]) and np.array_equal(bits(got[1]), bits(plain[1]))


def test_greedy_and_sampling_afterwards_as_on_a_fresh_context(edge):
    codes, offsets, p0, ctx, _ = edge
    fresh = Context(0, tuning=dict(NO_BG))
    try:
        fresh.set_sequences(codes, offsets, DNA)
        fresh.set_positions(W_E, p0)
        fresh.run_sweeps(PC, CUTOFF, 3, SEED)
        want_passes = fresh.run_greedy(PC, CUTOFF)[0]
        want = fresh.get_state()
        want_sampling = fresh.motif_sampling(W_E, PC, CUTOFF, 31)
    finally:
        fresh.close()
    ctx.set_positions(W_E, p0)
    ctx.run_sweeps_stats(PC, CUTOFF, 3, SEED)
    assert ctx.run_greedy(PC, CUTOFF)[0] == want_passes
    got = ctx.get_state()
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    again = ctx.motif_sampling(W_E, PC, CUTOFF, 31)
    assert np.array_equal(again[0], want_sampling[0]) and again[2] == want_sampling[2]
    assert np.array_equal(bits(again[1]), bits(want_sampling[1]))


def test_equals_the_chain_batch_of_one_chain(edge):
    codes, offsets, p0, ctx, _ = edge
    pos, pw, s = ctx.motif_run_stats(W_E, PC, CUTOFF, T, SEED, p0, burn_in=2, thin=2)
    bpos, bpw, status, b = ctx.motif_run_batch_stats(W_E, PC, CUTOFF, T, [SEED], pos=p0[None, :],
                                                    burn_in=2, thin=2)
    assert not status.any()
    assert np.array_equal(pos, bpos[0])
    assert np.array_equal(s["occupancy"], b["occupancy"][0])
    # the batch's sweep kernel rounds its PWMS on its own: its states' rows give the bound
    for i, t in enumerate(counted_sweeps(T, 2, 2)):
        ctx.set_positions(W_E, p0)
        ctx.run_sweeps(PC, CUTOFF, t + 1, SEED)
        row = ctx.get_state()[1]
        assert abs(s["ic"][i] - b["ic"][0, i]) <= trace_bound(row), t
