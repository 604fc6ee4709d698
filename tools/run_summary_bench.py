"""One chain of T sweeps reduced to what a caller keeps of it (each sequence's most frequent
start with its count, and the count matrix over the counted states): one gs_motif_run_summary
call against the statistics call with the host reduction it needed before.

    python tools/run_summary_bench.py --loop-lib PATH                  # the three shapes
    python tools/run_summary_bench.py --loop-lib PATH --shapes dna10k

Three sides from the same uploaded starts (the positions of random_starts mode 1, computed
outside the timed region):
  (a) gs_motif_run_stats with the bins through the parent commit's build (--loop-lib,
      required), then on the host ChainStats.mode() and the count matrix by numpy (the
      non-zero bins, a bincount a column); the call and the host reduction timed separately;
  (b) one gs_motif_run_summary call without the bins through this tree's library;
  (c) plain gs_motif_run through the parent's build.
Per shape a warm-up of every side, then `--reps` timed repetitions, the sides interleaved, wall
clock around the call(s) that return host results; the median counts, the spread (min, max) is
recorded.  Every repetition asserts that (b)'s modes and cells equal (a)'s exactly.  The
reduction's own device time (gs_summary_last_ms) is recorded next to the time of a
device-to-device copy of a slab of the bins' size in the same process: the traffic of reading
the bins once and writing them once, i.e. twice the floor of one read.
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from conftest import make_dataset  # noqa: E402
from run_batch_stats_bench import spread  # noqa: E402

# name: (N, L, W, T, burn_in); thin = 1: the shapes of tools/run_stats_bench.py
SHAPES = {"dna2000": (2_000, 200, 12, 200, 50), "dna10k": (10_000, 200, 12, 200, 50),
          "dna100k": (100_000, 500, 15, 50, 10)}
PC, CUTOFF, SEED, THIN = 1e-4, 1.0, 7, 1
ALPHA = b"ACGT"


def host_static(codes, offsets):
    """What the host reduction needs of the data, computed once outside the timed region:
    the symbols as alphabet indices (A: outside) and the sequences' compositions [N, A]."""
    A = len(ALPHA)
    index = np.full(256, A, np.uint8)
    index[np.frombuffer(ALPHA, np.uint8)] = np.arange(A)
    sym = index[codes]
    seq_of = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    comp = np.stack([np.bincount(seq_of[sym == a], minlength=len(offsets) - 1) for a in range(A)],
                    axis=1)
    return sym, comp


def host_count_matrix(occ, off, sym, comp, offsets, W):
    """C[A W] then T[A] of one chain's bins by numpy: the non-zero start bins, one bincount a
    column (binary64 weights: exact below 2^53), T from the sequences' compositions."""
    A = len(ALPHA)
    b = np.nonzero(occ)[0]
    n = np.searchsorted(off, b, side="right") - 1
    k = b - off[n] - 1
    keep = k >= 0
    b, n, k = b[keep], n[keep], k[keep]
    c = occ[b].astype(np.float64)
    cells = np.zeros(A * W + A, np.int64)
    for j in range(W):
        col = np.bincount(sym[offsets[n] + k + j], weights=c, minlength=A + 1)
        cells[np.arange(A) * W + j] = col[:A].astype(np.int64)
    per_seq = np.bincount(n, weights=c, minlength=len(off) - 1)  # S_n
    for a in range(A):
        cells[A * W + a] = int((per_seq * comp[:, a]).sum()) - int(cells[a * W:(a + 1) * W].sum())
    return cells


def copy_ms(n_bytes, reps=5):
    """Device-to-device copy of n_bytes, ms (the median of `reps` after a warm-up)."""
    import torch
    src = torch.zeros(n_bytes // 4, dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library: sides (a) and (c)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "chain" / "run_summary_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import ChainStats, Context

    rec = {"tool": "tools/run_summary_bench.py", "pc": PC, "cutoff": CUTOFF, "reps": args.reps,
           "thin": THIN, "loop_lib": "parent commit's build",
           "starts": "random_starts mode 1, uploaded", "shapes": {}}
    for name in args.shapes:
        N, L, W, T, burn_in = SHAPES[name]
        n_counted = len(range(burn_in, T, THIN))
        codes, offsets = make_dataset(N, L, W, ALPHA, seed=5)
        parent_stats, parent_plain = (Context(0, lib_path=args.loop_lib) for _ in range(2))
        mine = Context(0)
        ctxs = (parent_stats, parent_plain, mine)
        for c in ctxs:
            c.set_sequences(codes, offsets, ALPHA)
        off = mine.occupancy_offsets(W)
        starts = parent_plain.random_starts(W, PC, SEED, 1)[1]
        sym, comp = host_static(codes, offsets)

        def side_a():
            t0 = time.perf_counter()
            pos, pw, st = parent_stats.motif_run_stats(W, PC, CUTOFF, T, SEED, starts,
                                                       burn_in=burn_in, thin=THIN)
            t1 = time.perf_counter()
            cs = ChainStats(st["occupancy"][None, :], st["offsets"], st["ic"][None, :],
                            st["best_sweep"], [[]])
            mode = cs.mode()
            cells = host_count_matrix(st["occupancy"], st["offsets"], sym, comp, offsets, W)
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, pos, mode, cells

        def side_b():
            t0 = time.perf_counter()
            pos, pw, s = mine.motif_run_summary(W, PC, CUTOFF, T, SEED, starts, burn_in=burn_in,
                                                thin=THIN)
            return (time.perf_counter() - t0) * 1e3, pos, s

        def side_c():
            t0 = time.perf_counter()
            pos, pw = parent_plain.motif_run(W, PC, CUTOFF, T, SEED, starts)
            return (time.perf_counter() - t0) * 1e3, pos

        side_a(), side_b(), side_c()  # warm-up: code objects, allocations
        ms = {k: [] for k in ("a_call", "a_host", "a", "b", "c")}
        dev = []
        for rep in range(args.reps):
            call, host, pos_a, mode_a, cells_a = side_a()
            ms["a_call"].append(call)
            ms["a_host"].append(host)
            ms["a"].append(call + host)
            t, pos_b, s = side_b()
            ms["b"].append(t)
            dev.append(mine.summary_last_ms())
            t, pos_c = side_c()
            ms["c"].append(t)
            assert np.array_equal(pos_a, pos_b) and np.array_equal(pos_b, pos_c), name
            a_pos = np.array([m.Positions[0] if m.Positions else -1 for m in mode_a], np.int32)
            a_freq = np.array([m.PWMS for m in mode_a])
            assert np.array_equal(a_pos, s["mode_pos"]), f"{name}: modes differ"
            assert np.array_equal(a_freq, s["mode_count"] / float(n_counted)), f"{name}: counts differ"
            assert np.array_equal(cells_a, s["counts"]), f"{name}: cells differ"
        H = int(off[-1])
        cp = copy_ms(H * 4)
        med = {k: statistics.median(v) for k, v in ms.items()}
        entry = {"N": N, "L": L, "W": W, "sweeps": T, "burn_in": burn_in, "counted": n_counted,
                 "bins": H, "bin_bytes": H * 4,
                 "a_stats_call_parent": spread(ms["a_call"]), "a_host_reduction": spread(ms["a_host"]),
                 "a_total": spread(ms["a"]), "b_summary_call": spread(ms["b"]),
                 "c_plain_parent": spread(ms["c"]),
                 "a_over_b": med["a"] / med["b"], "a_call_alone_over_b": med["a_call"] / med["b"],
                 "summary_cost_ms_b_minus_c": med["b"] - med["c"],
                 "b_slowest_below_a_fastest": max(ms["b"]) < min(ms["a"]),
                 "b_slowest_below_a_call_alone_fastest": max(ms["b"]) < min(ms["a_call"]),
                 "reduction_device_ms": spread(dev), "d2d_copy_of_the_bins_ms": cp,
                 "reduction_over_copy": statistics.median(dev) / cp if cp > 0 else None,
                 "modes_and_cells_equal": True}
        rec["shapes"][name] = entry
        print(f"{name}: (a) {med['a']:.2f} = call {med['a_call']:.2f} + host {med['a_host']:.2f}, "
              f"(b) {med['b']:.2f} ({min(ms['b']):.2f} - {max(ms['b']):.2f}), (c) {med['c']:.2f} ms; "
              f"a / b x{entry['a_over_b']:.2f}, b - c {entry['summary_cost_ms_b_minus_c']:.2f} ms; "
              f"reduction {statistics.median(dev):.3f} ms on the device, copy of {H * 4} B "
              f"{cp:.3f} ms", file=sys.stderr, flush=True)
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"a_ms": v["a_total"]["median_ms"], "b_ms": v["b_summary_call"]["median_ms"],
                          "c_ms": v["c_plain_parent"]["median_ms"]}
                      for k, v in rec["shapes"].items()}))


if __name__ == "__main__":
    main()
