"""Host side of the batched repetition drivers under a caller's PCV / PPM: the header
declares gs_motif_sampling_batch_fixed, gs_site_sampling_batch_fixed and
gs_motif_sampling_multi_batch_fixed, _native binds them with the declared argument counts,
a wrong-shaped pcv / ppm raises before any native call, and the four mirrors keep their
loop unless batch=True, which makes one batch call with the values as keywords.  The
context is a stand-in: no device is touched."""
import re

import numpy as np
import pytest

from gibbssampling_amd import MotifSampler, SiteSampler, _native, sampler

NEW = ("gs_motif_sampling_batch_fixed", "gs_site_sampling_batch_fixed",
       "gs_motif_sampling_multi_batch_fixed")
SIBLING = {n: n[:-len("_fixed")] for n in NEW}
SOURCES = [b"ACGTACGTACGTACGT"] * 3
W, PC, CUTOFF = 5, 1e-4, 1.0
PCV = np.linspace(0.1, 0.9, 49)
PPM = np.linspace(0.01, 1.0, 49 * W).reshape(49, W)


def header_params(name):
    """The parameter declarations of one function of the header."""
    text = re.sub(r"/\*.*?\*/", "", _native.HEADER_PATH.read_text(), flags=re.S)
    m = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return [p.strip() for p in m.group(1).split(",")]


def test_the_header_declares_the_new_entry_points():
    names = _native.header_symbols()
    assert all(n in names for n in NEW)
    for n in NEW:
        params, plain = header_params(n), header_params(SIBLING[n])
        added = [p for p in params if p not in plain]
        assert added == ["const double *pcv49", "const double *ppm49"], (n, added)
        assert [p for p in params if p not in added] == plain, n
        # after the sampler parameters, before the seeds
        i = params.index("const double *pcv49")
        assert params[i + 1] == "const double *ppm49"
        assert params[i + 2] == "const uint64_t *seeds", n


def test_native_binds_them_with_the_declared_argument_counts():
    lib = _native.load_library()
    for n in NEW:
        f = getattr(lib, n)
        assert len(f.argtypes) == len(header_params(n)), n
        assert len(f.argtypes) == len(getattr(lib, SIBLING[n]).argtypes) + 2, n


@pytest.mark.parametrize("bad", [
    dict(pcv=np.ones(48)), dict(pcv=np.ones((49, 1))), dict(pcv=np.ones(50)),
    dict(ppm=np.ones((49, W + 1))), dict(ppm=np.ones((48, W))), dict(ppm=np.ones(49 * W)),
    dict(pcv=PCV, ppm=np.ones((W, 49))),
])
def test_a_wrong_shape_raises_with_no_library_loaded(bad):
    ctx = _native.Context.__new__(_native.Context)  # no library, no handle
    ctx.h, ctx.n_local = None, 3
    with pytest.raises(_native.ArgumentError):
        ctx.motif_sampling_batch(W, PC, CUTOFF, [1, 2], **bad)
    with pytest.raises(_native.ArgumentError):
        ctx.site_sampling_batch(W, PC, [1, 2], **bad)
    with pytest.raises(_native.ArgumentError):
        ctx.motif_sampling_multi_batch(2, W, PC, CUTOFF, [1, 2], **bad)


def test_fixed_args_passes_right_shapes_through():
    pcv, ppm = _native.fixed_args(list(PCV), PPM.tolist(), W)
    assert pcv.dtype == np.float64 and pcv.shape == (49,) and pcv.flags.c_contiguous
    assert ppm.dtype == np.float64 and ppm.shape == (49, W) and ppm.flags.c_contiguous
    assert _native.fixed_args(None, None, W) == (None, None)


class FakeCtx:
    """The single-chain and the batch entry points over a table: run `seed` leaves sequence
    n the start seed + n with score (seed + n) / 4; what is fixed on the context is noted
    with every call."""

    def __init__(self):
        self.calls = []
        self.pcv = self.ppm = None

    def set_fixed_pcv(self, pcv49):
        self.pcv = None if pcv49 is None else np.array(pcv49)

    def set_fixed_ppm(self, ppm49, W=None):
        self.ppm = None if ppm49 is None else np.array(ppm49)

    def _fixed(self):
        return self.pcv is not None, self.ppm is not None

    def _row(self, seed):
        k = seed + np.arange(len(SOURCES))
        return k.astype(np.int32), k / 4.0

    def motif_sampling(self, W, pc, cutoff, seed, init_mode=0, max_passes=1000):
        self.calls.append(("motif_sampling", seed, init_mode) + self._fixed())
        return self._row(seed) + (1,)

    def motif_sampling_multi(self, motif_amount, W, pc, cutoff, seed, init_mode=0,
                             max_passes=1000, cap=None):
        self.calls.append(("motif_sampling_multi", motif_amount, seed, init_mode) + self._fixed())
        p, w = self._row(seed)
        return np.ones(len(p), np.int32), p[:, None], w, 1

    def site_sampling(self, W, pc, seed, init_mode=0, max_passes=1000):
        self.calls.append(("site_sampling", seed, init_mode) + self._fixed())
        p, s = self._row(seed)
        return p, s, np.ones(3, np.int32)

    def _rows(self, seeds):
        rows = [self._row(s) for s in seeds]
        return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])

    def motif_sampling_batch(self, W, pc, cutoff, seeds, init_mode=0, max_passes=1000, *,
                             pcv=None, ppm=None):
        self.calls.append(("motif_sampling_batch", list(seeds), init_mode, pcv, ppm)
                          + self._fixed())
        p, w = self._rows(seeds)
        return p, w, np.ones(len(seeds), np.int32), np.zeros(len(seeds), np.int32)

    def motif_sampling_multi_batch(self, motif_amount, W, pc, cutoff, seeds, init_mode=0,
                                   max_passes=1000, cap=None, *, pcv=None, ppm=None):
        self.calls.append(("motif_sampling_multi_batch", motif_amount, list(seeds), init_mode,
                           pcv, ppm) + self._fixed())
        p, w = self._rows(seeds)
        return (np.ones(p.shape, np.int32), p[:, :, None], w, np.ones(len(seeds), np.int32),
                np.zeros(len(seeds), np.int32))

    def site_sampling_batch(self, W, pc, seeds, init_mode=0, max_passes=1000, *, pcv=None,
                            ppm=None):
        self.calls.append(("site_sampling_batch", list(seeds), init_mode, pcv, ppm)
                          + self._fixed())
        p, s = self._rows(seeds)
        return p, s, np.ones((len(seeds), 3), np.int32), np.zeros(len(seeds), np.int32)


def bind(monkeypatch, ctx):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return ctx


def drivers(batch):
    """The four mirrors (name, single-chain method, batch method, which value, call)."""
    kw = {} if batch is None else {"batch": batch}
    return [
        ("WithPCV", "motif_sampling", "motif_sampling_batch", "pcv",
         lambda reps, M=1: MotifSampler.findBestInormationContentContainingMotifsWithPCV(
             reps, M, W, PC, CUTOFF, "ACGT", SOURCES, PCV, seed=10, **kw)),
        ("OfPPM", "motif_sampling", "motif_sampling_batch", "ppm",
         lambda reps, M=1: MotifSampler.getBestPWMSsOfPPM(
             reps, M, W, PC, CUTOFF, "ACGT", SOURCES, PPM, seed=10, **kw)),
        ("WithBPV", "site_sampling", "site_sampling_batch", "pcv",
         lambda reps, M=1: SiteSampler.getMotifsWithBestInformationContentWithBPV(
             reps, W, PC, "ACGT", SOURCES, PCV, seed=10, **kw)),
        ("siteOfPPM", "site_sampling", "site_sampling_batch", "ppm",
         lambda reps, M=1: SiteSampler.getBestInformationContentOfPPM(
             reps, W, PC, "ACGT", SOURCES, PPM, seed=10, **kw)),
    ]


@pytest.mark.parametrize("batch", [None, False])
def test_the_loop_never_reaches_a_batch_method(monkeypatch, batch):
    for name, single, _, which, call in drivers(batch):
        ctx = bind(monkeypatch, FakeCtx())
        out = call(3)
        assert len(out) == len(SOURCES), name
        assert ctx.calls and all(c[0] == single for c in ctx.calls), (name, ctx.calls)
        # the values are set on the context around every run, and cleared after it
        assert all(c[-2:] == (which == "pcv", which == "ppm") for c in ctx.calls), name
        assert ctx.pcv is None and ctx.ppm is None, name
    # motifAmount 2: the list path's single-chain entry point
    for name, _, _, which, call in drivers(batch)[:2]:
        ctx = bind(monkeypatch, FakeCtx())
        call(3, 2)
        assert ctx.calls and all(c[0] == "motif_sampling_multi" and c[1] == 2
                                 for c in ctx.calls), (name, ctx.calls)


@pytest.mark.parametrize("reps", [3, 0])
def test_batch_true_makes_one_batch_call_with_the_values_as_keywords(monkeypatch, reps):
    seeds = [10 + r for r in range(reps + 1)]
    for (name, _, batched, which, call), (_, _, _, _, loop) in zip(drivers(True), drivers(False)):
        ctx = bind(monkeypatch, FakeCtx())
        out = call(reps)
        assert len(ctx.calls) == 1, (name, ctx.calls)
        got = ctx.calls[0]
        assert got[0] == batched and got[1] == seeds and got[2] == 0, (name, got)
        pcv, ppm = got[3], got[4]
        if which == "pcv":
            assert np.array_equal(pcv, PCV) and ppm is None, name
        else:
            assert np.array_equal(ppm, PPM) and pcv is None, name
        assert got[-2:] == (False, False), name  # nothing is set on the context itself
        # the same loop over the same runs
        assert out == loop(reps), name
    # motifAmount 2 goes to the list batch
    for (name, _, _, which, call), (_, _, _, _, loop) in zip(drivers(True)[:2],
                                                            drivers(False)[:2]):
        ctx = bind(monkeypatch, FakeCtx())
        out = call(reps, 2)
        assert len(ctx.calls) == 1, (name, ctx.calls)
        got = ctx.calls[0]
        assert got[0] == "motif_sampling_multi_batch" and got[1] == 2 and got[2] == seeds, name
        assert (got[4] is not None) == (which == "pcv") and (got[5] is not None) == (which == "ppm")
        assert out == loop(reps, 2), name
