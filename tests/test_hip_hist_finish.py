"""k_hist's per-object finish (FZ_HIST_FINISH, hist_finish_row in fz_kernels.h; docs/k_hist.md, "The finish") divides the histogram row by
the kernel mass with all of its loads issued together, convolves with a lane per block of 12 outputs and divides by the total from
registers.  Every operation, operand and order of operations is kde_finalize's, so the expectation is what the kernel gave BEFORE the
change, bit for bit: tests/golden/hist_finish_*.npz were recorded from a release build of the commit in front of it
(tools/record_hist_finish.py writes them from `problem` below).  Every case names the kernel form it ran, and 40 of its objects are
held against the oracle at the tolerances of tests/test_hip_hist_ahead.py, so that a fixture recorded from a wrong build could not pass.

The 48 objects are those of tests/test_hip_hist_lean.py (0.05 / 1 / 10 x the SDSS noise interleaved; two self matches; one object
handed to the sweep -- a row of NaNs, then redone; the two poor fits; 16 identical ones).  Every label has ONE error, so the dictionary
has one kernel of half-width w0 (the histogram form), and a quarter of the labels each sit on the first and on the last grid point, so
that the row's pad and the edge-truncated kernel mass carry weight.  The dictionaries are made for the case: a grid of G points and
a kernel of 2 w0 + 1 taps, also where the kernel is wider than the grid (which PDFDict's own constructor cannot make).
  G   5, 12      fewer outputs than one lane's block of 12, exactly one block
      13, 64, 127
      701        = 12 x 58 + 5: the last working lane's block is partial (the benchmark's grid); 661 = 12 x 55 + 1 with the widest kernels
      768        every lane's block is full
      769        a lane's block no longer covers the grid: kde_finalize, as before
    (16 rows of G + 2 w0 entries must fit the block's LDS beside the model tiles -- some 790 entries -- or the launch is k_fused's:
     the long grids come with narrow kernels, the wide kernels with G = 661)
  w0  1, 25
      31, 32     w2 = 62: every tap from the first tap register; w2 = 64: the first tap comes from the second register
      63, 64     w2 = 126, the largest two-register form; w2 = 128: kde_finalize's path for wide kernels, as before
      31 at G = 12: a window wider than the grid
At G = 701, w0 = 25: normalised and not (through the engine call), and one case each of mode B (the direct form), a masked object
(per-object band counts), per-model errors, a masked model band (the segmented form) and data of 4 and 6 bands.  M = 383 is one tile,
one lane short; M = 1000 three tiles.

Which cases run hist_finish_row: the plain 5-band cases (G.._w..), `raw` and `b4` -- band-constant errors at 4 and 5 bands, the forms
that have it (FIN in k_hist).  `B`, `objk`, `merr`, `seg` and `b6` run forms that keep the parent's kde_finalize: they hold the
parent's bits as a guard for the day one of those forms takes the routine."""
import os

import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID64, SDSS_SIGMA
# the engine, the one fit_predict of a case and the comparison of bits are those of the lean settle's test
import test_hip_hist_lean as lean
from test_hip_hist_lean import MISFIT, POOR, SAME, SELF, compute, engine, same_bits

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DELTA = 0.01
# the rows whose PDFs a fixture holds (ln-max and ln-evidence: every object's): the special ones, two of the identical ones, every noise level
KEEP = np.r_[np.arange(16), 20, 21, 36, 47]
SCREEN, DIRECT = 'k_hist<screen>', 'k_hist<exact>'
# name: (G, w0, M, bands, variant, normalize, form, seed)
CASES = {}
for _k, (_G, _w0, _M) in enumerate([(5, 1, 383), (12, 1, 383), (12, 31, 383), (13, 25, 383), (64, 32, 383), (64, 63, 383), (127, 63, 1000),
                                    (127, 64, 383), (701, 1, 383), (701, 25, 1000), (701, 31, 383), (701, 32, 383), (661, 63, 383),
                                    (661, 64, 383), (768, 1, 383), (768, 5, 1000), (769, 1, 383), (769, 5, 383)]):
    CASES['G%d_w%d' % (_G, _w0)] = (_G, _w0, _M, 5, '', True, SCREEN, 300 + _k)
CASES['G701_w25_raw'] = (701, 25, 1000, 5, '', False, SCREEN, 330)
CASES['G701_w25_B'] = (701, 25, 383, 5, 'B', True, DIRECT, 331)
CASES['G701_w25_objk'] = (701, 25, 383, 5, 'objk', True, SCREEN + ' (per-object band counts)', 332)
CASES['G701_w25_merr'] = (701, 25, 383, 5, 'merr', True, SCREEN, 333)
CASES['G701_w25_seg'] = (701, 25, 383, 5, 'seg', True, SCREEN + ' (segmented models)', 334)
CASES['G701_w25_b4'] = (701, 25, 383, 4, '', True, SCREEN, 335)
CASES['G701_w25_b6'] = (701, 25, 383, 6, '', True, SCREEN, 336)
_dicts = {}


def fixture_path(name):
    return os.path.join(GOLDEN, 'hist_finish_%s.npz' % name)


def case_dicts(G, w0):
    """(PDFDict, oracle KernelDict) with a grid of G points and ONE kernel of half-width w0 in force (a second, wider one fills the
    dictionary's sigma grid and is never asked for): both are built on a grid long enough for the kernels and then given the case's grid"""
    if (G, w0) not in _dicts:
        from frankenz_amd import PDFDict
        s = (w0 - 0.5) * DELTA / 5.                                 # ceil(5 s / delta) = w0
        long_grid = np.arange(max(G, 4 * w0 + 4)) * DELTA
        out = []
        for cls in (PDFDict, fo.KernelDict):
            d = cls(long_grid, np.array([s, 2. * s]))
            assert int(d.sigma_width[0]) == w0 and len(d.sigma_dict[0]) == 2 * w0 + 1 and len(d.sigma_dict[1]) == 2 * int(d.sigma_width[1]) + 1
            d.grid = long_grid[:G].copy()
            d.Ngrid, d.min, d.max = G, d.grid[0], d.grid[-1]
            out.append(d)
        _dicts[(G, w0)] = (tuple(out), s)
    return _dicts[(G, w0)]


def problem(name):
    """objects at 0.05 / 1 / 10 x the SDSS noise, interleaved, and the special ones of the module's docstring"""
    G, w0, M, B, var, normalize, form, seed = CASES[name]
    rs = np.random.RandomState(seed)
    N = 48
    sig = np.resize(SDSS_SIGMA, B)
    Y = rs.lognormal(1., 1., size=(M, B))
    Ye = np.tile(sig, (M, 1))
    Ym = np.ones((M, B))
    if var == 'merr':
        Ye = Ye * rs.uniform(0.5, 1.5, size=(M, B))                # per-model errors
    scale = np.array([0.05, 1., 10.])[np.arange(N) % 3][:, None]
    X = Y[rs.randint(0, M, N)] + scale * sig * rs.standard_normal((N, B))
    Xe = scale * np.tile(sig, (N, 1))
    Xm = np.ones((N, B))
    X[SELF[0]], X[SELF[1]] = Y[0], Y[M - 1]
    X[MISFIT] = 1e6 + Y[0]
    for i, c in zip(POOR, (-1.5, -2.5)):
        Xe[i] = 10. * sig
        X[i] = c * Xe[i]
    X[SAME] = X[SAME[0]]; Xe[SAME] = Xe[SAME[0]]
    if var == 'objk':
        Xm[[0, 1, 40], [2, 4, 0]] = 0.0                            # masked objects
        X[Xm == 0] = -7e5                                          # garbage in the unobserved bands must not matter
    if var == 'seg':
        Ym[rs.choice(M, 12, replace=False), rs.randint(0, B, 12)] = 0.0      # masked model bands
    (pd, od), s = case_dicts(G, w0)
    z = rs.uniform(0., (G - 1) * DELTA, M)
    z[0::4], z[1::4] = 0., (G - 1) * DELTA                         # piled on the first and the last grid point
    ze = np.full(M, s)
    kw = {'free_scale': True, 'ignore_model_err': True} if var == 'B' else {}
    return dict(Y=Y, Ye=Ye, Ym=Ym, X=X, Xe=Xe, Xm=Xm, z=z, ze=ze, kw=kw, keep=KEEP, dicts=(pd, od), normalize=normalize, form=form)


def run(pr):
    """one fit_predict with the case's dictionary: `compute` of the lean settle's test; not normalised: the same call with that option"""
    saved = lean._cache.get('dicts')
    lean._cache['dicts'] = pr['dicts']
    try:
        if pr['normalize']:
            return compute(pr)
        from frankenz_amd.engine import DeviceArray, kde_opts, like_opts
        eng = engine()
        eng.upload_models(pr['Y'], pr['Ye'], pr['Ym'])
        G = eng.set_labels(pr['z'], pr['ze'], label_dict=pr['dicts'][0])
        N = len(pr['X'])
        out = [DeviceArray(eng, (N, G)), DeviceArray(eng, (N, 1)), DeviceArray(eng, (N, 1))]
        for a in out:
            a.set_rows(0, np.full(a.shape, np.nan))
        eng.fit_predict_prior(pr['X'].copy(), pr['Xe'].copy(), pr['Xm'].copy(), like_opts(pr['kw']), kde_opts({}, normalize=False), None,
                              out[0], out[1], out[2], n=N)
        eng.sync()
        return dict(pdfs=out[0].numpy()[pr['keep']], lmap=out[1].numpy()[:, 0], levid=out[2].numpy()[:, 0], form=eng.last_form())
    finally:
        if saved is None:
            lean._cache.pop('dicts', None)
        else:
            lean._cache['dicts'] = saved


@pytest.mark.parametrize('name', list(CASES))
def test_bits_of_the_parent(name):
    want = np.load(fixture_path(name))
    pr = problem(name)
    got = run(pr)
    assert got['form'] == str(want['form']) == pr['form']
    for k in ('lmap', 'levid', 'pdfs'):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
        same_bits(got[k], want[k])
    assert not np.isnan(got['lmap']).any() and not np.isnan(got['levid']).any() and not np.isnan(got['pdfs']).any()
    # identical objects: identical results, whichever wave they fell to
    for k in ('lmap', 'levid'):
        assert (got[k][SAME] == got[k][SAME[0]]).all()
    assert (got['pdfs'][17] == got['pdfs'][16]).all()              # (rows 20 and 21)
    # 40 objects against the oracle
    idx = np.arange(40)
    with np.errstate(all='ignore'):
        rp, rlm, rle = fo.bruteforce_fit_predict(pr['X'][idx].copy(), pr['Xe'][idx].copy(), pr['Xm'][idx].copy(), pr['Y'], pr['Ye'], pr['Ym'],
                                                 pr['z'], pr['ze'], label_dict=pr['dicts'][1], **pr['kw'])
    both = np.intersect1d(pr['keep'], idx)
    assert len(both) >= 19
    p = got['pdfs'][np.searchsorted(pr['keep'], both)]
    if not pr['normalize']:
        # the stack of the weights relative to the evidence: its sum is the stacked share of the evidence, at most 1 and -- the
        # threshold drops weights below 1e-3 of the best -- not far below; the oracle holds the normalised row
        tot = p.sum(axis=1, keepdims=True)
        assert (tot <= 1. + 1e-12).all() and (tot > 0.5).all()
        p = p / tot
    np.testing.assert_allclose(p, rp[np.searchsorted(idx, both)], rtol=1e-7, atol=1e-13)
    np.testing.assert_allclose(got['lmap'][idx], rlm, rtol=1e-9)
    np.testing.assert_allclose(got['levid'][idx], rle, **EVID64)
