"""One chain of T sweeps with its statistics (occupancy, trace of the summed PWMS, best state)
on the single-chain sweep kernels: one gs_motif_run_stats call against what a caller had to
do before it.

    python tools/run_stats_bench.py --loop-lib PATH                  # the three shapes
    python tools/run_stats_bench.py --loop-lib PATH --shapes dna10k

Five sides from the same uploaded starts (the positions of random_starts mode 1, computed
outside the timed region):
  (a)  plain gs_motif_run through the parent commit's build (--loop-lib, required);
  (a') the same through this tree's library;
  (b)  one gs_motif_run_stats call through this tree's library;
  (c)  T one-sweep gs_run_sweeps + gs_state_get calls through the parent's build, with the tally
       in numpy: bins, the ordered sum of every PWMS row, the first-maximum best state;
  (d)  gs_motif_run_batch_stats with one chain through the parent's build.
Per shape a warm-up of every side, then `--reps` timed repetitions, the sides interleaved (the
two plain calls swapping places every repetition), wall clock around the call(s) that return
host results; the median counts, the spread (min, max) is recorded.  Every repetition asserts
that (b)'s bins and final positions equal (c)'s exactly (the two may hand over to the
all-background kernel at different sweeps, so the trace is compared within the PWMS tolerance).
A further context with the profile on gives the device time of the statistics launches
(gs_run_stats_last_ms), per counted sweep.
"""
import argparse
import hashlib
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
from pmc_traffic import _code_only  # noqa: E402
from run_batch_stats_bench import bits, ic_rows, spread  # noqa: E402

# name: (N, L, W, T, burn_in); thin = 1.  The burn-in of the last shape is this tool's choice:
# a fifth of its sweeps, as at the other two a quarter
SHAPES = {"dna2000": (2_000, 200, 12, 200, 50), "dna10k": (10_000, 200, 12, 200, 50),
          "dna100k": (100_000, 500, 15, 50, 10)}
PC, CUTOFF, SEED, THIN = 1e-4, 1.0, 7, 1
SOURCES = ["gibbssampling_amd/csrc/gs_chainstats.hip", "gibbssampling_amd/csrc/gs_api.cpp",
           "gibbssampling_amd/csrc/gs_engine.cpp", "gibbssampling_amd/csrc/gs_common.h",
           "gibbssampling_amd/csrc/gs_ctx.h", "gibbssampling_amd/csrc/Makefile"]


def source_hash(root: Path = ROOT) -> str:
    h = hashlib.sha256()
    for s in SOURCES:
        h.update(s.encode())
        h.update(_code_only((root / s).read_text()).encode())
    return h.hexdigest()


def stepwise(ctx, W, T, burn_in, starts, off):
    """Side (c): T one-sweep calls, two downloads each, and the host tally."""
    occ = np.zeros(int(off[-1]), np.int32)
    base = off[:-1] + 1
    ic = np.zeros(len(range(burn_in, T, THIN)), np.float64)
    best_sweep, best_ic, best = -1, 0.0, None
    ctx.set_positions(W, starts)
    pos = pwms = None
    for t in range(T):
        ctx.run_sweeps(PC, CUTOFF, 1, SEED, first_sweep=t)
        pos, pwms = ctx.get_state()
        if t < burn_in or (t - burn_in) % THIN:
            continue
        occ[base + pos] += 1  # the bins of one sweep are distinct
        v = float(ic_rows(pwms[None, :])[0])
        ic[(t - burn_in) // THIN] = v
        if best_sweep < 0 or v > best_ic:
            best_sweep, best_ic, best = t, v, (pos, pwms)
    return pos, pwms, {"occupancy": occ, "ic": ic, "best_sweep": best_sweep, "best": best}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library: sides (a), (c) and (d)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "chain" / "run_stats_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    rec = {"tool": "tools/run_stats_bench.py", "source_sha256": source_hash(), "pc": PC,
           "cutoff": CUTOFF, "reps": args.reps, "thin": THIN, "loop_lib": "parent commit's build",
           "starts": "random_starts mode 1, uploaded", "shapes": {}}
    for name in args.shapes:
        N, L, W, T, burn_in = SHAPES[name]
        n_counted = len(range(burn_in, T, THIN))
        codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5)
        # one context a side, so that each plain call's context has seen plain calls only
        parent, parent_step, parent_batch = (Context(0, lib_path=args.loop_lib) for _ in range(3))
        mine, mine_stats, mine_prof = Context(0), Context(0), Context(0)
        ctxs = (parent, parent_step, parent_batch, mine, mine_stats, mine_prof)
        for c in ctxs:
            c.set_sequences(codes, offsets, b"ACGT")
        off = mine.occupancy_offsets(W)
        starts = parent.random_starts(W, PC, SEED, 1)[1]

        def plain(ctx):
            return ctx.motif_run(W, PC, CUTOFF, T, SEED, starts)

        def stats(ctx, **parts):
            return ctx.motif_run_stats(W, PC, CUTOFF, T, SEED, starts, burn_in=burn_in, thin=THIN,
                                       **parts)

        def batch(ctx):
            return ctx.motif_run_batch_stats(W, PC, CUTOFF, T, [SEED], pos=starts[None, :],
                                             burn_in=burn_in, thin=THIN)

        # warm-up: code objects, allocations
        plain(parent), plain(mine), stats(mine_stats), batch(parent_batch)
        parent_step.set_positions(W, starts)
        parent_step.run_sweeps(PC, CUTOFF, 1, SEED)
        parent_step.get_state()
        ms = {k: [] for k in ("a", "a_tree", "b", "c", "d")}
        kernel = mine_stats.sweep_kernel_name()
        for rep in range(args.reps):
            res = {}
            for k in (("a", "a_tree"), ("a_tree", "a"))[rep % 2]:
                ctx = parent if k == "a" else mine
                t0 = time.perf_counter()
                res[k] = plain(ctx)
                ms[k].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            pos_b, pw_b, b = stats(mine_stats)
            ms["b"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            pos_c, pw_c, c = stepwise(parent_step, W, T, burn_in, starts, off)
            ms["c"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            pos_d, _, st_d, d = batch(parent_batch)
            ms["d"].append((time.perf_counter() - t0) * 1e3)
            assert not st_d.any(), st_d
            assert np.array_equal(b["occupancy"], c["occupancy"]), f"{name}: bins differ from (c)"
            assert np.array_equal(b["occupancy"], d["occupancy"][0]), f"{name}: bins differ from (d)"
            for p in (pos_c, pos_d[0], res["a"][0], res["a_tree"][0]):
                assert np.array_equal(pos_b, p), name
            # the plain calls run the statistics call's kernels sweep for sweep: to the bit
            assert np.array_equal(bits(pw_b), bits(res["a_tree"][1])), name
            assert np.array_equal(bits(pw_b), bits(res["a"][1])), name
            tol = (1e-12 + N * 2.0 ** -52) * float(np.abs(pw_c).sum()) * 2  # each side within the bound of the exact sum
            assert np.all(np.abs(b["ic"] - c["ic"]) <= tol), name
        # the statistics launches' own device time
        mine_prof.profile(True)
        stats(mine_prof)
        stats(mine_prof)
        chain_ms, stat_ms = mine_prof.run_stats_last_ms()
        alone = {}  # ... and with one statistic asked for at a time
        for part in ("occupancy", "ic", "best"):
            parts = {k: k == part for k in ("occupancy", "ic", "best")}
            stats(mine_prof, **parts)
            stats(mine_prof, **parts)
            alone[part] = 1e3 * mine_prof.run_stats_last_ms()[1] / max(n_counted, 1)
        med = {k: statistics.median(v) for k, v in ms.items()}
        entry = {"N": N, "L": L, "W": W, "sweeps": T, "burn_in": burn_in, "counted": n_counted,
                 "bins": int(off[-1]), "sweep_kernel_at_the_end": kernel,
                 "a_plain_parent": spread(ms["a"]), "a_plain_this_tree": spread(ms["a_tree"]),
                 "b_stats_call": spread(ms["b"]), "c_stepwise_numpy": spread(ms["c"]),
                 "d_batch_stats_one_chain_parent": spread(ms["d"]),
                 "stats_cost_ms_b_minus_a": med["b"] - med["a"],
                 "c_over_b": med["c"] / med["b"], "d_over_b": med["d"] / med["b"],
                 "b_slowest_below_c_fastest": max(ms["b"]) < min(ms["c"]),
                 "b_slowest_below_d_fastest": max(ms["b"]) < min(ms["d"]),
                 "plain_this_tree_within_parent_spread": min(ms["a"]) <= med["a_tree"] <= max(ms["a"]),
                 "profiled_chain_device_ms": chain_ms, "profiled_stats_launches_device_ms": stat_ms,
                 "stats_launch_us_per_counted_sweep": 1e3 * stat_ms / max(n_counted, 1),
                 "stats_launch_us_per_counted_sweep_one_statistic_alone": alone,
                 "best_sweeps_won": int(len(set(np.maximum.accumulate(b["ic"]).tolist()))),
                 "b_bins_equal_c_and_d": True}
        rec["shapes"][name] = entry
        print(f"{name}: " + ", ".join(
            f"({k}) {med[k]:.2f} ({min(ms[k]):.2f} - {max(ms[k]):.2f})" for k in ms) +
              f" ms; b - a {med['b'] - med['a']:.2f} ms, c / b x{med['c'] / med['b']:.2f}, d / b "
              f"x{med['d'] / med['b']:.2f}; statistics launch "
              f"{entry['stats_launch_us_per_counted_sweep']:.2f} us a counted sweep, alone "
              f"{ {k: round(v, 2) for k, v in alone.items()} }, {entry['best_sweeps_won']} wins ({kernel})",
              file=sys.stderr, flush=True)
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"a_ms": v["a_plain_parent"]["median_ms"],
                          "b_ms": v["b_stats_call"]["median_ms"],
                          "c_ms": v["c_stepwise_numpy"]["median_ms"],
                          "d_ms": v["d_batch_stats_one_chain_parent"]["median_ms"]}
                      for k, v in rec["shapes"].items()}))


if __name__ == "__main__":
    main()
