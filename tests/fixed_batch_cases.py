"""What the three GPU test files of the batched ByPCV / WithBPV / OfPPM drivers share
(test_gpu_fixed_batch.py, test_gpu_fixed_site_batch.py, test_gpu_fixed_multi_batch.py):
the seeds, the shapes, the caller's values and the comparisons."""
import numpy as np

from conftest import make_dataset

RTOL = 1e-12
PC, CUTOFF = 1e-4, 1.0
PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"
# non-contiguous, one duplicate (rows 1 and 3), one beyond 2^32
SEEDS = [1001, 77, 5_000_000_007, 77, 12]

# name: (alphabet, symbols outside it in the data, N, L, W, ragged, dataset seed)
SHAPES = {
    "dna": (b"ACGT", b"", 150, 90, 9, True, 77),
    "dna-extra": (b"ATGC-", b"*", 150, 90, 9, True, 79),
    "protein": (PROTEIN, b"", 40, 60, 8, False, 80),
}


def dataset(name):
    alpha, extra, N, L, W, ragged, dseed = SHAPES[name]
    return make_dataset(N, L, W, alpha, seed=dseed, ragged=ragged, mut=0.1, extra=extra,
                        extra_rate=0.03 if extra else 0.0)


def pcv49(alpha, seed):
    """pcv49 of test_gpu_variants.py: non-uniform, strictly positive, not summing to 1, a
    value of its own at every slot outside the alphabet (a wrong slot mapping shows)."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.05, 0.6, 49)
    slots = [c - 42 for c in alpha]
    v[slots] = rng.dirichlet(np.ones(len(alpha)))
    return v


def ppm49(W, seed):
    return np.random.default_rng(seed).uniform(0.01, 1.0, (49, W))


def values(name, kind, W=None):
    """(pcv, ppm) of a shape for kind 'pcv', 'ppm' or 'both'."""
    alpha, _, _, _, w, _, dseed = SHAPES[name]
    W = w if W is None else W
    return (pcv49(alpha, dseed + W) if kind in ("pcv", "both") else None,
            ppm49(W, dseed + 100) if kind in ("ppm", "both") else None)


def set_fixed(ctx, pcv, ppm, W):
    ctx.set_fixed_pcv(pcv)
    ctx.set_fixed_ppm(ppm, W if ppm is not None else None)


def close(g, o):
    g, o = np.asarray(g, np.float64), np.asarray(o, np.float64)
    same = g == o  # also equal infinities (log2 of a zero best score)
    with np.errstate(invalid="ignore"):
        rel = np.abs(g - o) / np.maximum(np.abs(o), 1e-300)
    return bool(np.all(same | (rel <= RTOL)))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def sources_of(codes, offsets):
    return [bytes(codes[offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]
