"""k_hist's lean screen form pins the LDS reads of the next model record in front of the chi2 (docs/k_hist.md, "LDS reads a step
ahead").  The order of memory operations changed and nothing else -- every arithmetic operation, every ring slot and the order of
every sum are the parent's -- so the expectation is what the kernel gave BEFORE the change, bit for bit: tests/golden/hist_ahead_*.npz were
recorded from a build of the commit in front of it (tools/record_hist_ahead.py writes them from `problem` below).  Every case names
the kernel form it ran, and 12 of its objects are held against the oracle at the tolerances of tests/test_hip_hist_lean.py, so that
a fixture recorded from a wrong build could not pass.

The 48 objects are those of tests/test_hip_hist_lean.py (0.05 / 1 / 10 x the SDSS noise interleaved -- light objects and objects
that drain at every step --, two self matches, one object handed to the sweep, the two poor fits, 16 identical ones).  M sits at
the edges of the tile loop, where a drain carried from one step into the next (measured and not kept, see the document; any later
attempt at it meets these cases) goes wrong first; tiles hold 384 models = 6 groups of 64 (256 = 4 groups with per-model errors),
and a drain falls due when a step leaves 64 or more entries in the ring:
  64, 65   one partial tile (the tail form), a drain due at the only full step
  384      exactly one full tile: a drain falls due at the tile's last group
  385      ... and a one-model tail tile right after it
  448      a partial second tile
  769      two full tiles + 1
  1153     three full tiles + 1
in mode A with band-constant errors, mode Ai, and with 2 % of the object bands unobserved (the per-object band-count form);
per-model errors at 257 and 513 (one and two 256-model tiles + 1).  `rounds` has more objects than one round of the launch holds
(2 R + 37, R = 16 waves x CUs) at M = 1000 and keeps the PDFs of 32 seeded rows."""
import os

import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID64, SDSS_SIGMA
# the engine, the dictionaries, the one fit_predict of a case and the comparison of bits are those of the lean settle's test
from test_hip_hist_lean import MISFIT, ORACLE_ROWS, POOR, SAME, SELF, compute, dicts, engine, same_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MS = (64, 65, 384, 385, 448, 769, 1153)
# name: (M, lprob_kwargs, share of unobserved object bands, per-model errors, seed)
CASES = {}
for _k, _M in enumerate(MS):
    CASES['A_M%d' % _M] = (_M, {}, 0.0, False, 100 + _k)
    CASES['Ai_M%d' % _M] = (_M, {'ignore_model_err': True}, 0.0, False, 120 + _k)
    CASES['objk_M%d' % _M] = (_M, {}, 0.02, False, 140 + _k)
CASES['vary_M257'] = (257, {}, 0.0, True, 160)
CASES['vary_M513'] = (513, {}, 0.0, True, 161)
CASES['rounds'] = (1000, {}, 0.0, False, 170)


def fixture_path(name):
    return os.path.join(GOLDEN, 'hist_ahead_%s.npz' % name)


def problem(name, N=None):
    """objects at 0.05 / 1 / 10 x the SDSS noise, interleaved, and the special ones of the module's docstring"""
    M, kw, mask, vary, seed = CASES[name]
    if N is None:
        N = int(np.load(fixture_path(name))['N']) if name == 'rounds' else 48
    rs = np.random.RandomState(seed)
    B = 5
    Y = rs.lognormal(1., 1., size=(M, B))
    Ye = np.tile(SDSS_SIGMA, (M, 1))
    if vary:
        Ye = Ye * rs.uniform(0.5, 1.5, size=(M, B))               # per model and band
    Ym = np.ones((M, B))
    scale = np.array([0.05, 1., 10.])[np.arange(N) % 3][:, None]
    X = Y[rs.randint(0, M, N)] + scale * SDSS_SIGMA * rs.standard_normal((N, B))
    Xe = scale * np.tile(SDSS_SIGMA, (N, 1))
    Xm = np.ones((N, B))
    X[SELF[0]], X[SELF[1]] = Y[0], Y[M - 1]
    X[MISFIT] = 1e6 + Y[0]
    for i, c in zip(POOR, (-1.5, -2.5)):
        Xe[i] = 10. * SDSS_SIGMA
        X[i] = c * Xe[i]
    X[SAME] = X[SAME[0]]; Xe[SAME] = Xe[SAME[0]]
    if mask > 0:
        Xm = (rs.uniform(size=(N, B)) >= mask).astype(float)
        Xm[[0, 1], [2, 4]] = 0.0                                  # (48 objects at 2 %: make sure some band IS unobserved)
        Xm[Xm.sum(axis=1) < 3] = 1.0
        X[Xm == 0] = -7e5                                         # garbage in the unobserved bands must not matter
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    keep = np.sort(rs.choice(N, 32, replace=False)) if name == 'rounds' else np.arange(N)
    return dict(Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, kw=kw, keep=keep)


@pytest.mark.parametrize('name', list(CASES))
def test_bits_of_the_parent(name):
    want = np.load(fixture_path(name))
    pr = problem(name)
    got = compute(pr)
    N = len(pr['X'])
    if name == 'rounds':
        assert N > 16 * engine().cu_count()                       # more than one round
    assert got['form'] == str(want['form'])
    assert got['form'] == ('k_hist<screen> (per-object band counts)' if name.startswith('objk') else 'k_hist<screen>')
    for k in ('lmap', 'levid', 'pdfs'):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
        same_bits(got[k], want[k])
    # the identical objects: identical rows (in `rounds` the kept rows are seeded ones, so there ln-max and ln-evidence only)
    # (with unobserved bands: those of them that observe the same bands as the first)
    same = SAME[(pr['Xm'][SAME] == pr['Xm'][SAME[0]]).all(axis=1)]
    assert len(same) >= 8
    for k in ('lmap', 'levid') + (() if name == 'rounds' else ('pdfs',)):
        assert (got[k][same] == got[k][same[0]]).all()
    assert not np.isnan(got['lmap']).any() and not np.isnan(got['levid']).any()
    # 12 objects against the oracle
    _, od = dicts()
    idx = ORACLE_ROWS
    with np.errstate(all='ignore'):
        rp, rlm, rle = fo.bruteforce_fit_predict(pr['X'][idx].copy(), pr['Xe'][idx].copy(), pr['Xm'][idx].copy(), pr['Y'], pr['Ye'], pr['Ym'],
                                                 pr['z'], pr['ze'], label_dict=od, **pr['kw'])
    if name != 'rounds':
        np.testing.assert_allclose(got['pdfs'][idx], rp, rtol=1e-7, atol=1e-13)
    np.testing.assert_allclose(got['lmap'][idx], rlm, rtol=1e-9)
    np.testing.assert_allclose(got['levid'][idx], rle, **EVID64)
