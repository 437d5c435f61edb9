"""The waves of k_hist change their issue priority with their progress between two tile barriers (FZ_HIST_PRIO, FZ_HIST_PRIO_FORMS;
docs/k_hist.md, "Waves of a SIMD kept in step").  A priority moves time and no bits, and the headline's own outputs are already held
bit for bit by tests/test_hip_hist_lean.py, _ahead.py, _seam.py and _order.py.  This file holds the OTHER forms the priority is
compiled into -- per-object band counts, the direct forms (free scale; every weight in fp64 with band-constant errors, the kernel
of the broad likelihoods), the segmented kernel, the headline's siblings at 4 and 6 bands -- and the screen form with per-model
errors (10-double records, 256-model tiles), which keeps the parent's code: the guard for the change that gives it one.

The expectation is what the kernel gave before the change, bit for bit: tests/golden/hist_prio_*.npz were recorded from a release
build of the commit in front of it (tools/record_hist_prio.py writes them from `problem` below).  Every case names the kernel form
it ran, and 40 of its objects are held against the oracle at the tolerances of tests/test_hip_hist_ahead.py, so that a fixture
recorded from a wrong build could not pass.

The 48 objects are those of tests/test_hip_hist_lean.py (0.05 / 1 / 10 x the SDSS noise interleaved, two self matches, one object
handed to the sweep, the two poor fits, 16 identical ones), per form:
  merr     model errors that differ from model to model and band to band
  objk     2 % of the object bands unobserved (as tests/test_hip_hist_lean.py's M769_objk)
  B        free scale, model errors ignored
  exact    FZ_EXACT_EVIDENCE=1: every pair weighed in fp64 without the classifier (the kernel broad likelihoods run)
  seg      per-model errors and 6 % of the model bands masked (every model keeps four): the segment-ordered layout
  b4, b6   4 and 6 bands, band-constant errors
and per size (tiles hold 384, 256 or 128 models by record width):
  383      one 384-model tile, one lane short (a whole 256-model tile and a partial one)
  768      a regular tile plus the tail form (three whole 256-model tiles)
  1600     a partial last tile in every tiling
  rounds   three whole rounds of the launch plus one object (3 R + 1, R = 16 waves x CUs) at M = 1000: waves without work meet the
           barriers of a fourth round; the objects repeat the 48, so every copy must give the same bits
A fixture holds ln-max and ln-evidence of every object and the PDFs of 20 rows (rounds: 32 seeded rows and the last object)."""
import os

import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID64, SDSS_SIGMA
from test_hip_hist_lean import MISFIT, POOR, SAME, SELF, compute, dicts, engine, same_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROUNDS = 3                        # whole rounds in front of the one with a single object
KEEP = np.r_[np.arange(16), 20, 21, 36, 47]
# form: (bands, lprob_kwargs, per-model errors, share of masked model bands, share of unobserved object bands, kernel form, environment)
FORMS = {'merr': (5, {}, True, 0.0, 0.0, 'k_hist<screen>', {}),
         'objk': (5, {}, False, 0.0, 0.02, 'k_hist<screen> (per-object band counts)', {}),
         'B': (5, {'free_scale': True, 'ignore_model_err': True}, False, 0.0, 0.0, 'k_hist<exact>', {}),
         'exact': (5, {}, False, 0.0, 0.0, 'k_hist<exact>', {'FZ_EXACT_EVIDENCE': '1'}),
         'seg': (5, {}, True, 0.06, 0.0, 'k_hist<screen> (segmented models)', {}),
         'b4': (4, {}, False, 0.0, 0.0, 'k_hist<screen>', {}),
         'b6': (6, {}, False, 0.0, 0.0, 'k_hist<screen>', {})}
# name: (M, form, seed)
CASES = {}
for _f, _form in enumerate(FORMS):
    for _k, (_tag, _M) in enumerate((('M383', 383), ('M768', 768), ('M1600', 1600), ('rounds', 1000))):
        CASES['%s_%s' % (_form, _tag)] = (_M, _form, 300 + 10 * _f + _k)


def fixture_path(name):
    return os.path.join(GOLDEN, 'hist_prio_%s.npz' % name)


def rounds_n():
    return ROUNDS * 16 * engine().cu_count() + 1


def problem(name, N=None):
    """objects at 0.05 / 1 / 10 x the SDSS noise, interleaved, the special ones of the module's docstring, in the form's shape"""
    M, form, seed = CASES[name]
    B, kw, merr, mmask, omask = FORMS[form][:5]
    rounds = name.endswith('rounds')
    if N is None:
        N = int(np.load(fixture_path(name))['N']) if rounds else 48
    rs = np.random.RandomState(seed)
    NB = 48
    sig = np.resize(SDSS_SIGMA, B)
    Y = rs.lognormal(1., 1., size=(M, B))
    Ye = sig * rs.uniform(0.5, 1.5, size=(M, B)) if merr else np.tile(sig, (M, 1))      # (per model and band: the 10-double records)
    Ym = np.ones((M, B))
    if mmask > 0:
        Ym = (rs.uniform(size=(M, B)) >= mmask).astype(float)
        Ym[Ym.sum(axis=1) < 4] = 1.0
    scale = np.array([0.05, 1., 10.])[np.arange(NB) % 3][:, None]
    X = Y[rs.randint(0, M, NB)] + scale * sig * rs.standard_normal((NB, B))
    Xe = scale * np.tile(sig, (NB, 1))
    X[SELF[0]], X[SELF[1]] = Y[0], Y[M - 1]
    X[MISFIT] = 1e6 + Y[0]
    for i, c in zip(POOR, (-1.5, -2.5)):
        Xe[i] = 10. * sig
        X[i] = c * Xe[i]
    X[SAME] = X[SAME[0]]; Xe[SAME] = Xe[SAME[0]]
    rep = np.arange(N) % NB                                       # (rounds: the 48 again and again)
    Xm = np.ones((NB, B))
    if omask > 0:
        Xm = (rs.uniform(size=(NB, B)) >= omask).astype(float)
        Xm[[0, 1], [2, 4]] = 0.0                                  # (48 objects at 2 %: make sure some band IS unobserved)
        Xm[Xm.sum(axis=1) < 3] = 1.0
        Xm[SAME] = Xm[SAME[0]]
        X[Xm == 0] = -7e5                                         # garbage in the unobserved bands must not matter
    X, Xe, Xm = X[rep].copy(), Xe[rep].copy(), Xm[rep].copy()
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    keep = np.union1d(rs.choice(N, 32, replace=False), [N - 1]) if rounds else KEEP
    return dict(Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, kw=kw, keep=keep, rep=rep)


@pytest.mark.parametrize('name', list(CASES))
def test_bits_of_the_parent(name, monkeypatch):
    want = np.load(fixture_path(name))
    for k, v in FORMS[CASES[name][1]][6].items():
        monkeypatch.setenv(k, v)
    pr = problem(name)
    got = compute(pr)
    N = len(pr['X'])
    rounds = name.endswith('rounds')
    if rounds:
        assert N == rounds_n()                                    # three whole rounds and one object: a fourth round with one working wave
    assert got['form'] == str(want['form']) == FORMS[CASES[name][1]][5]
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
