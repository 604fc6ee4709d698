"""The first-maximum fixtures (tests/first_max.py) are worth running (CPU only).

For every fixture: the visit-by-visit replays equal the oracle's drivers exactly; both
trap conditions (no near-tie of distinct motif products inside the kernels' band, no
fresh-against-stored comparison closer than 1e-9 relative unless both come from one
bit-identical product) hold at every visit of every pass, so the oracle's positions
are the truth for a device whose log differs from the C library's in the last place;
and the tied sets reach the geometry that the reductions can get wrong: enough
targets tie, a later tied window sits in a lower lane (k mod 64) than the first, the
first tied window lies beyond the first 64-window chunk, and (wide) tied windows fall
in different 512-thread blocks.  The thresholds are fixed; the seeds were tuned.
The reached counts are printed (pytest -s) and quoted in DESIGN section 3.
"""
import numpy as np
import pytest

import first_max as fm
from oracle import oracle_lib as ol

STAR = ["dna", "atgc", "protein", "wide"]


@pytest.mark.parametrize("name", STAR)
def test_star_and_site_fixtures(name):
    f = fm.fixture(name)
    assert int(np.diff(f.offsets).max()) == f.L and len(f.offsets) - 1 == f.N
    need = dict(fm.NEED, block=fm.NEED_BLOCK) if name == "wide" else fm.NEED
    for label, equal, visits, tie_case in fm.runs(f):
        g = fm.geometry(visits)
        t1, t2 = fm.traps(visits)
        print(f"{name}: {label}: {len(visits)} visits, {g}")
        assert equal, f"{name}: {label}: the replay differs from the oracle"
        assert not t1, f"{name}: {label}: trap 1 (near-tie of motif products) at (pass, n) {t1}"
        assert not t2, f"{name}: {label}: trap 2 (fresh against stored) at (pass, n) {t2}"
        if tie_case:
            for k, v in need.items():
                assert g[k] >= v, f"{name}: {label}: {k} = {g[k]} < {v}"


def test_protein_has_more_than_64_windows():
    f = fm.fixture("protein")
    assert int(np.diff(f.offsets).min()) - f.W + 1 > 64


def test_background_and_motif_ties_are_both_present():
    bg = motif = 0
    for name in STAR:
        f = fm.fixture(name)
        for cut in fm.CUTOFFS:
            g = fm.geometry(f.replay_greedy(cut)[3])
            bg, motif = bg + g["bg"], motif + g["motif"]
    print(f"targets tying at a background category {bg}, at a motif category {motif}")
    assert bg >= fm.NEED["tie"] and motif >= fm.NEED["tie"]


def test_background_ties_are_bit_exact_rotations():
    """Cut-off 1e9: the categories are raw binary64 products of the composite vector.
    Cyclic rotations of one multiset fold in another order and may differ in the last
    place, so the tied set is smaller than the set of windows within 1e-12: only the
    reference's own left fold finds it."""
    f = fm.fixture("dna")
    near = 0
    for n in range(f.N):  # the start snapshot's background categories
        G = ol.target_detail(f.seqs, f.W, fm.PC, f.pos0, n)["G"]
        tied = np.count_nonzero(G == G.max())
        near += tied >= 2 and np.count_nonzero(np.abs(G - G.max()) <= 1e-12 * G.max()) > tied
    print(f"dna: {near} targets hold a rotation within 1e-12 of their tied background maximum")
    assert near >= 2


@pytest.mark.parametrize("name", ["lists2", "lists3"])
def test_list_fixtures(name):
    f = fm.fixture(name)
    equal, visits, last = fm.list_run(f)
    t1, t2 = fm.traps(visits)
    print(f"{name}: {len(visits)} visits, {fm.geometry(visits)}, {last} tie at level {f.M}")
    assert equal, f"{name}: the replay differs from ol.greedy_lists"
    assert not t1, f"{name}: trap 1 at (pass, n) {t1}"
    assert not t2, f"{name}: trap 2 at (pass, n) {t2}"
    assert last >= fm.NEED_LAST_LEVEL


def test_zero_fixture():
    f = fm.fixture("zero")
    for label, equal, visits, _ in fm.runs(f):
        t1, t2 = fm.traps(visits)
        assert equal and not t1 and not t2, f"zero: {label}"
    score, pos, visits = f.replay_site_scan()
    K = np.diff(f.offsets) - f.W + 1
    # 0: a non-alphabet symbol in every window: (log2 0., 0)
    assert score[0] == -np.inf and pos[0] == 0 and len(visits[0].tied) == K[0]
    # 1: only windows k >= 64 score above zero
    assert pos[1] >= 64 and visits[1].tied[0] >= 64
    # 2: a homopolymer: every window ties, the first wins
    assert pos[2] == 0 and len(visits[2].tied) == K[2] and np.isfinite(score[2])
    g = f.replay_greedy(1.0)
    assert len(g[3][2].tied) == K[2]
