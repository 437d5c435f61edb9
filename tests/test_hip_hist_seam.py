"""k_hist's lean screen form meets the tile's barrier in front of the tile's LAST group, whose prefetch slot reads the first group of
the next tile into registers (FZ_HIST_SEAM; with FZ_HIST_WAIT_EARLY, compiled out by default, it also waits for the next record in
the middle of a step; docs/k_hist.md, "Waits for what the step consumes").  Waits and a barrier moved and nothing else -- every arithmetic operation, every ring slot and the order of every sum are the parent's --
so the expectation is what the kernel gave BEFORE the change, bit for bit: tests/golden/hist_seam_*.npz were recorded from a release
build of the commit in front of it (tools/record_hist_seam.py writes them from `problem` below).  Every case names the kernel form
it ran, and 40 of its objects are held against the oracle at the tolerances of tests/test_hip_hist_ahead.py, so that a fixture
recorded from a wrong build could not pass.

The 48 objects are those of tests/test_hip_hist_lean.py (0.05 / 1 / 10 x the SDSS noise interleaved, so that the waves of a block
drain at different steps; two self matches; one object handed to the sweep; the two poor fits; 16 identical ones) and one more
self match, with the FIRST model of the second tile -- lane 0 of the record that is carried across the seam in registers.  Tiles hold
384 models = 6 groups of 64; tests/test_hip_hist_ahead.py has M = 64, 65, 384, 385, 448, 769 and 1153, here are the sizes at which
a moved barrier or a carried record goes wrong:
  383      one tile, one lane short: no seam, the tail form's barrier alone
  768      two whole tiles and no tail: the second tile is the last, takes the tail form and receives a carried record
  1152     three whole tiles: buffer A is staged a second time while the waves still hold its first tile's last record
  1600     four whole tiles + one whole 64-model group: the last tile's final group with models is not the tile's sixth
in mode A with band-constant errors and in mode Ai; a fixture holds ln-max and ln-evidence of all 48 and the PDFs of 20 (KEEP).  `rounds` has three whole rounds of the launch plus one object (3 R + 1, R = 16
waves x CUs) at M = 1000, so that 15 waves of one block -- and all 16 of every other -- idle through a fourth round and meet its
barriers without work; its objects repeat the 48 (so every copy must give the same bits), and it keeps the PDFs of 32 seeded rows
and of the last object."""
import os

import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID64, SDSS_SIGMA
# the engine, the dictionaries, the one fit_predict of a case and the comparison of bits are those of the lean settle's test
from test_hip_hist_lean import MISFIT, POOR, SAME, SELF, compute, dicts, engine, same_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MS = (383, 768, 1152, 1600)
SEAMSELF = 7                      # the object that IS the first model of the second tile
ROUNDS = 3                        # whole rounds in front of the one with a single object
# the rows whose PDFs a fixture holds (ln-max and ln-evidence: every object's): the special ones, two of the identical ones, every noise level
KEEP = np.r_[np.arange(16), 20, 21, 36, 47]
# name: (M, lprob_kwargs, seed)
CASES = {}
for _k, _M in enumerate(MS):
    CASES['A_M%d' % _M] = (_M, {}, 200 + _k)
    CASES['Ai_M%d' % _M] = (_M, {'ignore_model_err': True}, 220 + _k)
CASES['A_rounds'] = (1000, {}, 240)
CASES['Ai_rounds'] = (1000, {'ignore_model_err': True}, 241)


def fixture_path(name):
    return os.path.join(GOLDEN, 'hist_seam_%s.npz' % name)


def rounds_n():
    return ROUNDS * 16 * engine().cu_count() + 1


def problem(name, N=None):
    """objects at 0.05 / 1 / 10 x the SDSS noise, interleaved, and the special ones of the module's docstring"""
    M, kw, seed = CASES[name]
    rounds = name.endswith('rounds')
    if N is None:
        N = int(np.load(fixture_path(name))['N']) if rounds else 48
    rs = np.random.RandomState(seed)
    B, NB = 5, 48
    Y = rs.lognormal(1., 1., size=(M, B))
    Ye = np.tile(SDSS_SIGMA, (M, 1))
    Ym = np.ones((M, B))
    scale = np.array([0.05, 1., 10.])[np.arange(NB) % 3][:, None]
    X = Y[rs.randint(0, M, NB)] + scale * SDSS_SIGMA * rs.standard_normal((NB, B))
    Xe = scale * np.tile(SDSS_SIGMA, (NB, 1))
    X[SELF[0]], X[SELF[1]] = Y[0], Y[M - 1]
    X[SEAMSELF] = Y[384 if M > 384 else M // 2]
    X[MISFIT] = 1e6 + Y[0]
    for i, c in zip(POOR, (-1.5, -2.5)):
        Xe[i] = 10. * SDSS_SIGMA
        X[i] = c * Xe[i]
    X[SAME] = X[SAME[0]]; Xe[SAME] = Xe[SAME[0]]
    rep = np.arange(N) % NB                                       # (rounds: the 48 again and again)
    X, Xe = X[rep].copy(), Xe[rep].copy()
    Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    keep = np.union1d(rs.choice(N, 32, replace=False), [N - 1]) if rounds else KEEP
    return dict(Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, kw=kw, keep=keep, rep=rep)


@pytest.mark.parametrize('name', list(CASES))
def test_bits_of_the_parent(name):
    want = np.load(fixture_path(name))
    pr = problem(name)
    got = compute(pr)
    N = len(pr['X'])
    rounds = name.endswith('rounds')
    if rounds:
        assert N == rounds_n()                                    # three whole rounds and one object: a fourth round with one working wave
    assert got['form'] == str(want['form']) == 'k_hist<screen>'
    for k in ('lmap', 'levid', 'pdfs'):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
        same_bits(got[k], want[k])
    assert not np.isnan(got['lmap']).any() and not np.isnan(got['levid']).any()
    # identical objects: identical results, whichever wave and round they fell to
    for k in ('lmap', 'levid'):
        assert (got[k] == got[k][pr['rep']]).all()
        assert (got[k][SAME] == got[k][SAME[0]]).all()
    first = {}
    for r, j in enumerate(pr['keep']):
        first.setdefault(pr['rep'][j], r)
    assert np.array_equal(got['pdfs'], got['pdfs'][[first[pr['rep'][j]] for j in pr['keep']]], equal_nan=True)
    # 40 objects against the oracle (rounds: 39 + the single object of the last round; the PDF of that one)
    _, od = dicts()
    idx = np.r_[np.arange(39), N - 1] if rounds else np.arange(40)
    with np.errstate(all='ignore'):
        rp, rlm, rle = fo.bruteforce_fit_predict(pr['X'][idx].copy(), pr['Xe'][idx].copy(), pr['Xm'][idx].copy(), pr['Y'], pr['Ye'], pr['Ym'],
                                                 pr['z'], pr['ze'], label_dict=od, **pr['kw'])
    both = np.intersect1d(pr['keep'], idx)                        # (rounds: the last object, at the least)
    assert len(both) >= (1 if rounds else 19)
    np.testing.assert_allclose(got['pdfs'][np.searchsorted(pr['keep'], both)], rp[np.searchsorted(idx, both)], rtol=1e-7, atol=1e-13)
    np.testing.assert_allclose(got['lmap'][idx], rlm, rtol=1e-9)
    np.testing.assert_allclose(got['levid'][idx], rle, **EVID64)
