"""Host side of the mirror's chains of sweeps with Positions lists: runSweeps and
runSweepsBatched keep today's calls (Context.motif_run / motif_run_batch) for the default
motifAmount and single positions, and route to Context.motif_run_multi /
motif_run_multi_batch for motifAmount >= 2 or a MotifIndex of more than one position; a chain
whose status is set raises the mapped exception.  The context is a stand-in: no device is
touched."""
import numpy as np
import pytest

from gibbssampling_amd import ChecksumOverflowError, MotifSampler, _native, sampler
from gibbssampling_amd.sampler import createMotifIndex

SOURCES = [b"ACGTACGTACGTACGT"] * 3
NEW = ("gs_motif_run_multi_batch", "gs_motif_run_multi", "gs_run_multi_batch_last_ms",
       "gs_run_multi_batch_last_info")


class FakeCtx:
    """Every chain entry point over a table: chain r leaves sequence n the list
    [r + n, 0][:(r + n) % 3] with PWMS (r + n) / 4."""

    def __init__(self, status=None):
        self.status = status
        self.calls = []

    def _rows(self, R):
        n = len(SOURCES)
        k = np.arange(R)[:, None] + np.arange(n)[None, :]
        return k, k / 4.0

    def motif_run(self, W, pc, cutoff, n_sweeps, seed, pos, first_sweep=0):
        self.calls.append(("motif_run", W, pc, cutoff, n_sweeps, seed, np.array(pos).tolist(),
                           first_sweep))
        k, pw = self._rows(1)
        return k[0].astype(np.int32), pw[0]

    def motif_run_batch(self, W, pc, cutoff, n_sweeps, seeds, pos=None, init_mode=0,
                        first_sweep=0, u=None):
        self.calls.append(("motif_run_batch", W, pc, cutoff, n_sweeps, list(seeds),
                           None if pos is None else np.array(pos).tolist(), init_mode,
                           first_sweep))
        k, pw = self._rows(len(seeds))
        return k.astype(np.int32), pw, np.zeros(len(seeds), np.int32)

    def _lists(self, R, cap):
        k, pw = self._rows(R)
        pos = np.full(k.shape + (cap,), -1, np.int32)
        pos[..., 0] = np.where(k % 3 >= 1, k, -1)
        pos[..., 1] = np.where(k % 3 == 2, 0, -1)
        return (k % 3).astype(np.int32), pos, pw

    def motif_run_multi(self, motif_amount, W, pc, cutoff, n_sweeps, seed, cnt, pos,
                        first_sweep=0, cap=None):
        self.calls.append(("motif_run_multi", motif_amount, W, pc, cutoff, n_sweeps, seed,
                           np.array(cnt).tolist(), np.array(pos).tolist(), first_sweep, cap))
        c, p, w = self._lists(1, cap)
        return c[0], p[0], w[0]

    def motif_run_multi_batch(self, motif_amount, W, pc, cutoff, n_sweeps, seeds, cnt=None,
                              pos=None, init_mode=0, first_sweep=0, cap=None, u=None):
        self.calls.append(("motif_run_multi_batch", motif_amount, W, pc, cutoff, n_sweeps,
                           list(seeds), None if cnt is None else np.array(cnt).tolist(),
                           None if pos is None else np.array(pos).tolist(), init_mode,
                           first_sweep, cap))
        R = len(seeds)
        status = np.zeros(R, np.int32) if self.status is None else np.asarray(self.status, np.int32)
        return self._lists(R, cap) + (status,)


def bind(monkeypatch, ctx):
    monkeypatch.setattr(sampler, "_bind", lambda *a, **k: ctx)
    return ctx


MEM = [createMotifIndex(0.5, [3]), createMotifIndex(0.0, []), createMotifIndex(1.0, [7])]


def test_the_default_keyword_makes_todays_calls(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    out = MotifSampler.runSweeps(5, 1e-4, 1.0, "ACGT", SOURCES, MEM, 20, 9, first_sweep=4)
    assert out == [createMotifIndex(0.0, [0]), createMotifIndex(0.25, [1]),
                   createMotifIndex(0.5, [2])]
    MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 20, [10, 11], [MEM, MEM],
                                  first_sweep=40)
    MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 7, [1, 2, 3], init_mode=1)
    MotifSampler.runSweeps(5, 1e-4, 1.0, "ACGT", SOURCES, MEM, 20, 9, motifAmount=1)
    assert ctx.calls == [
        ("motif_run", 5, 1e-4, 1.0, 20, 9, [3, -1, 7], 4),
        ("motif_run_batch", 5, 1e-4, 1.0, 20, [10, 11], [[3, -1, 7], [3, -1, 7]], 0, 40),
        ("motif_run_batch", 5, 1e-4, 1.0, 7, [1, 2, 3], None, 1, 0),
        ("motif_run", 5, 1e-4, 1.0, 20, 9, [3, -1, 7], 0),
    ]


def test_motif_amount_two_makes_the_list_calls(monkeypatch):
    ctx = bind(monkeypatch, FakeCtx())
    out = MotifSampler.runSweeps(5, 1e-4, 1.0, "ACGT", SOURCES, MEM, 20, 2**64 + 9,
                                 first_sweep=4, motifAmount=2)
    assert ctx.calls == [("motif_run_multi", 2, 5, 1e-4, 1.0, 20, 2**64 + 9, [1, 0, 1],
                          [[3, -1], [-1, -1], [7, -1]], 4, 2)]
    assert out == [createMotifIndex(0.0, []), createMotifIndex(0.25, [1]),
                   createMotifIndex(0.5, [2, 0])]
    ctx.calls.clear()
    out = MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 20, [10, 2**64 + 11],
                                        [MEM, MEM[::-1]], first_sweep=40, motifAmount=2)
    assert ctx.calls == [("motif_run_multi_batch", 2, 5, 1e-4, 1.0, 20, [10, 11],
                          [[1, 0, 1], [1, 0, 1]],
                          [[[3, -1], [-1, -1], [7, -1]], [[7, -1], [-1, -1], [3, -1]]], 0, 40, 2)]
    assert out == [[createMotifIndex(0.0, []), createMotifIndex(0.25, [1]),
                    createMotifIndex(0.5, [2, 0])],
                   [createMotifIndex(0.25, [1]), createMotifIndex(0.5, [2, 0]),
                    createMotifIndex(0.75, [])]]
    # without starts the init_mode goes through
    ctx.calls.clear()
    out = MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 7, [1, 2, 3], init_mode=1,
                                        motifAmount=3)
    assert ctx.calls == [("motif_run_multi_batch", 3, 5, 1e-4, 1.0, 7, [1, 2, 3], None, None, 1,
                          0, 3)]
    assert len(out) == 3 and all(len(chain) == len(SOURCES) for chain in out)


def test_a_list_of_two_positions_makes_the_list_calls(monkeypatch):
    """motifAmount 1 with a MotifIndex of two positions: the capacity widens to the list."""
    ctx = bind(monkeypatch, FakeCtx())
    mem = [createMotifIndex(0.5, [9, 3]), MEM[1], MEM[2]]
    MotifSampler.runSweeps(5, 1e-4, 1.0, "ACGT", SOURCES, mem, 3, 1)
    MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2], [MEM, mem])
    assert ctx.calls == [
        ("motif_run_multi", 1, 5, 1e-4, 1.0, 3, 1, [2, 0, 1], [[9, 3], [-1, -1], [7, -1]], 0, 2),
        ("motif_run_multi_batch", 1, 5, 1e-4, 1.0, 3, [1, 2], [[1, 0, 1], [2, 0, 1]],
         [[[3, -1], [-1, -1], [7, -1]], [[9, 3], [-1, -1], [7, -1]]], 0, 0, 2),
    ]


def test_a_set_status_raises_the_mapped_exception(monkeypatch):
    bind(monkeypatch, FakeCtx([0, _native.GS_E_OVERFLOW, 0]))
    with pytest.raises(ChecksumOverflowError) as e:
        MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2, 3], motifAmount=2)
    assert e.value.status == _native.GS_E_OVERFLOW
    bind(monkeypatch, FakeCtx([_native.GS_E_UNSUPPORTED, 0, 0]))
    with pytest.raises(_native.GibbsError) as e:
        MotifSampler.runSweepsBatched(5, 1e-4, 1.0, "ACGT", SOURCES, 3, [1, 2, 3], motifAmount=2)
    assert e.value.status == _native.GS_E_UNSUPPORTED


def test_the_header_declares_the_new_entry_points():
    names = _native.header_symbols()
    assert all(n in names for n in NEW)
