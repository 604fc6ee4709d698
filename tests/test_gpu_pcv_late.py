"""The four-symbol kernel's hold-one-out PCV with its division taken where the quotient is
read (gs_sweep.hip kPcvLate): the group's slice holds the numerators
T[a] + s + pc, and the picked window's PWMS factors, the exact rescan's table and the
log of a target without a motif divide by the same denominator.  Through the outputs:
3-sweep chains on the loop path and the one-iteration path, bit for bit against each
other (positions, PWMS, aggregates, counters) and against the oracle, at W = 4, 12, 32 on
16 lanes a sequence and W = 12 on 32 and 64 (Lmax = 257, 900); starts without a motif
(the log of the quotient at once), all placed (the table's log, no quotient before the
PWMS) and mixed; PWMS on every sweep and on the last only; every target through the
exact rescan; pseudo-count 0 with a zero numerator; ragged lengths down to one window.
The all-background takeover is off (bg_mode 0).
"""
import numpy as np
import pytest

import decision_edges as de
import test_gpu_ek4_cells as ec
import test_gpu_scan_bgsum as sb
from oracle import oracle_lib as ol

pytestmark = pytest.mark.gpu

ALPHA = ec.ALPHA
PC, CUT = ec.PC, ec.CUT


@pytest.fixture(scope="module")
def ctx_pair():
    """(loop path, one-iteration path) of gs_sweep_kernel's four-symbol instantiation."""
    from gibbssampling_amd import Context
    c0 = Context(0, tuning={"dna_mode": 0.0, "sweep_one": 0.0, "bg_mode": 0.0})
    c1 = Context(0, tuning={"dna_mode": 0.0, "sweep_one": 1.0, "bg_mode": 0.0})
    yield c0, c1
    for c in (c0, c1):
        st = c.stats()
        c.close()
        assert st["rescan_recheck"] == 0 and st["desc_oob"] == 0, st


# W, Lmax, lanes a sequence (16 Lmax / 16 < lanes: 257 is the first length of 32 lanes)
SHAPES = [(4, 70, 16), (12, 90, 16), (32, 120, 16), (12, 257, 32), (12, 900, 64)]


@pytest.mark.parametrize("N", [1, 5, 17])
@pytest.mark.parametrize("kind", ["none", "placed", "mixed"])
@pytest.mark.parametrize("W,L,gl", SHAPES)
def test_chains(ctx_pair, W, L, gl, kind, N):
    codes, offsets = de.dataset(N, L, W, ALPHA, 500 + W + N)
    pos = ec.starts(np.diff(offsets), W, kind, 501 + W + N)
    ec.both_paths(ctx_pair, codes, offsets, W, pos, 502 + W, gl, f"W = {W}, L = {L}, N = {N}, starts {kind}")


@pytest.mark.parametrize("W,L,gl", SHAPES)
def test_ragged_down_to_one_window(ctx_pair, W, L, gl):
    """Lengths from W (K = 1) to Lmax, mixed starts."""
    N = 17
    codes, offsets = de.dataset(N, L, W, ALPHA, 510 + W, lmin=W)
    lens = np.diff(offsets)
    assert lens.min() < L // 2 and lens.max() == L
    pos = ec.starts(lens, W, "mixed", 511 + W)
    ec.both_paths(ctx_pair, codes, offsets, W, pos, 512 + W, gl, f"ragged, W = {W}, L = {L}")


@pytest.mark.parametrize("one", [0, 1])
@pytest.mark.parametrize("W,L,gl", SHAPES)
def test_pwms_on_every_sweep(ctx_pair, W, L, gl, one):
    """Three 1-sweep calls (the picked window's factors PPM' / (numerator / denominator)
    on each) against the 3-sweep chain (on its last sweep only): bit for bit; each
    sweep's positions and PWMS are the oracle's."""
    c = ctx_pair[one]
    N = 17
    codes, offsets = de.dataset(N, L, W, ALPHA, 520 + W)
    pos = ec.starts(np.diff(offsets), W, "mixed", 521 + W)
    seed = 522 + W
    p3, w3, a3, _ = ec.chain(c, codes, offsets, W, pos, seed)
    ec.launch_is(c, one, gl)
    S = ol.Seqs(codes, offsets, ALPHA)
    c.set_positions(W, pos)
    op = pos
    for t in range(3):
        c.run_sweeps(PC, CUT, 1, seed, first_sweep=t)
        p1, w1 = c.get_state()
        op, ow, _ = ol.sweep(S, W, PC, CUT, op, ec.uniforms(seed, ol.stream_sweep(t), N), threads=8)
        ec.same_as_oracle(p1, w1, op, ow, f"sweep {t} of three calls, W = {W}, L = {L}")
    assert np.array_equal(p3, p1) and w3.tobytes() == w1.tobytes()
    assert a3.tobytes() == c.agg_download().tobytes()


def test_every_target_rescanned(ctx_pair):
    """test_gpu_scan_bgsum.py's all-rescan set (every sequence A but for one run of
    W = 32 symbols cycling C, G, T: a window of the run lies more than 96 below the
    scan's reference in every target, asserted), two targets without a motif: every exact
    table divides the numerators.  A 3-sweep chain whose first sweep rescans every
    target, both paths bit for bit and the oracle's."""
    N, L, W = 9, 256, 32
    a = np.frombuffer(ALPHA, np.uint8)
    codes = np.full(N * L, a[0], np.uint8)
    offsets = np.arange(0, N * L + 1, L, dtype=np.int64)
    for n in range(N):
        codes[n * L + 11 * n: n * L + 11 * n + W] = a[1 + (np.arange(W) + n) % 3]
    S = ol.Seqs(codes, offsets, ALPHA)
    pos = ol.random_starts(S, W, PC, seed=92, mode=1)[1].astype(np.int32)
    pos[[1, 6]] = -1
    lo, _ = sb.window_offsets(S, W, pos)
    assert (lo < -(sb.RANGE + 1.0)).all(), lo
    u = np.random.default_rng(531).random(N)
    op, ow, _ = ol.sweep(S, W, PC, CUT, pos, u)
    out = []
    for c, one in zip(ctx_pair, (0, 1)):
        c.set_sequences(codes, offsets, ALPHA)
        s0 = c.stats()
        gp, gw = c.motif_sweep(W, PC, CUT, pos, u)
        dl = sb.delta(c, s0)
        ec.launch_is(c, one, 16)
        assert dl["exact_rescans"] == N, dl
        ec.same_as_oracle(gp, gw, op, ow, f"every target through the exact rescan, one = {one}")
        out.append((gp, gw, c.agg_download()))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2].tobytes() == out[1][2].tobytes()
    _, _, s1 = ec.both_paths(ctx_pair, codes, offsets, W, pos, 532, 16, "all-rescan set, 3-sweep chain")
    assert s1["exact_rescans"] >= N, s1


@pytest.mark.parametrize("W,gl,L", [(4, 16, 70), (12, 16, 90), (32, 16, 120), (12, 32, 257), (12, 64, 900)])
def test_zero_numerator(ctx_pair, W, gl, L):
    """Pseudo-count 0 and no T anywhere but in one sequence's motif segment: that
    sequence's hold-one-out background counts no T, the numerator and so the PCV are 0
    (the exact rescan, whose table then holds PPM' / 0), and two targets have no motif.
    One sweep, both paths bit for bit (aggregates and counters too), against the oracle."""
    N = 9
    rng = np.random.default_rng(540 + W + gl)
    a = np.frombuffer(ALPHA, np.uint8)
    lens = np.full(N, L)
    offsets = np.arange(0, N * L + 1, L, dtype=np.int64)
    codes = a[rng.integers(0, 3, N * L)].astype(np.uint8)
    pos = (rng.random(N) * (lens - W + 1)).astype(np.int32)
    pos[[2, 7]] = -1
    codes[4 * L + pos[4]: 4 * L + pos[4] + W] = a[3]  # every T of the data is in this segment
    S = ol.Seqs(codes, offsets, ALPHA)
    u = rng.random(N)
    out = []
    for c, one in zip(ctx_pair, (0, 1)):
        c.set_sequences(codes, offsets, ALPHA)
        s0 = c.stats()
        gp, gw = c.motif_sweep(W, 0.0, CUT, pos, u)
        dl = sb.delta(c, s0)
        ec.launch_is(c, one, gl)
        assert dl["exact_rescans"] >= 1, dl
        out.append((gp, gw, c.agg_download(), dl))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2].tobytes() == out[1][2].tobytes() and out[0][3] == out[1][3]
    op, ow, _ = ol.sweep(S, W, 0.0, CUT, pos, u)
    ec.same_as_oracle(out[1][0], out[1][1], op, ow, f"zero numerator, W = {W}, {gl} lanes")
