"""The summary kernels (fz_summary.h: k_rownorm, k_gemm_f64, k_summarize, k_resample, k_overlap) where their other tests do not go:
rows with NaN / infinite entries and all-zero rows against the reference (golden g21), grids shorter than a wave and shapes at the
edges of the 128 x 128 GEMM tile, the 16-deep K step and the four-wave block against the oracle, pdfs_resample against numpy.interp
row by row, loglike_nz at one-row, one-column and 257-block shapes.

Tolerances are those of tests/test_hip_summary.py: statistics against the reference 1e-10 / 1e-12, against the oracle on seeded
stacks 1e-9 / 1e-11, rows renormalised in place 1e-14, resampled rows 1e-13, loglike_nz 1e-13.  NaNs must sit exactly where the
expectation has them.  Every comparison prints its worst relative deviation before it asserts (pytest -s shows them)."""
import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROWS = ['mean', 'mean_std', 'mean_conf', 'mean_risk', 'med', 'med_std', 'med_conf', 'med_risk', 'mode', 'mode_std',
        'mode_conf', 'mode_risk', 'best', 'best_std', 'best_conf', 'best_risk', 'low95', 'low68', 'high68', 'high95', 'mc']
BEST = (12, 13, 14, 15)
CLEAN = [0, 8, 9, 10, 11]                      # the rows of g21's stack without an edit


def flat(res):
    return np.array([a for grp in res[:5] for a in grp] + [res[5]])


class Uniforms(object):
    """``rstate.rand()`` handing out a stored list, one number per object"""

    def __init__(self, u):
        self.u, self.k = u, 0

    def rand(self):
        self.k += 1
        return self.u[self.k - 1]


def close(got, want, rtol, atol, what):
    """NaNs in the same places, infinities equal, everything else within rtol / atol; prints the worst relative deviation"""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), '%s: NaNs at %s, expected at %s' % (
        what, np.argwhere(np.isnan(got))[:8].tolist(), np.argwhere(np.isnan(want))[:8].tolist())
    fin = np.isfinite(want) & np.isfinite(got) & (want != 0)
    worst = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.
    print('%-58s worst relative deviation %.3g' % (what, worst))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, equal_nan=True, err_msg=what)
    return worst


def close_stats(got, want, rtol, atol, what, rows=range(21)):
    for r in rows:
        close(got[r], want[r], rtol, atol, '%s %s' % (what, ROWS[r]))


# ---- 1. non-finite and all-zero rows against the reference ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def g21():
    return load_golden('g21_summary_edges')


@pytest.mark.parametrize('kern', ['lorentz', 'tophat'])
@pytest.mark.parametrize('ren', [True, False])
def test_nonfinite_rows_against_g21(g21, ren, kern):
    """NaN at column 0, 1, 33, 64, at two columns, an all-NaN and an all-zero row among clean ones, 65 grid points: all 21 statistics
    and the array as left in place; the five clean rows alone give the same bits as among the others (a bad row in the same
    workgroup or MFMA tile does not touch its neighbours)."""
    from frankenz_amd.pdf import pdfs_summarize
    tag = ('ren_' if ren else 'noren_') + kern
    work = g21['edge'].copy()
    got = flat(pdfs_summarize(work, g21['grid'], renormalize=ren, rstate=Uniforms(g21['urand']), pkern=kern))
    close_stats(got, g21[tag + '_stats'], 1e-10, 1e-12, tag)
    close(work, g21[tag + '_after'], 1e-14, 0, tag + ' rows in place')
    alone = g21['edge'][CLEAN].copy()
    got5 = flat(pdfs_summarize(alone, g21['grid'], renormalize=ren, rstate=Uniforms(g21['urand'][CLEAN]), pkern=kern))
    assert np.array_equal(got5.view(np.uint64), got[:, CLEAN].view(np.uint64))
    assert np.array_equal(alone.view(np.uint64), work[CLEAN].view(np.uint64))


def test_nonfinite_rows_with_a_window_function(g21):
    """a custom ``wconf_func`` on the same stack: the windows of the oracle's estimators through ``fo.interp_rows``; NaN where the
    estimator is NaN"""
    from frankenz_amd.pdf import pdfs_summarize
    wfun = lambda p: 0.02 + 0.05 * p
    grid, N = g21['grid'], len(g21['edge'])
    a, b = g21['edge'].copy(), g21['edge'].copy()
    got = flat(pdfs_summarize(a, grid, renormalize=False, rstate=Uniforms(g21['urand']), wconf_func=wfun))
    with np.errstate(all='ignore'):
        want = flat(fo.pdfs_summarize(b, grid, renormalize=False, urand=g21['urand']))
        assert np.array_equal(want, g21['noren_lorentz_stats'], equal_nan=True)
        cdfs = b.cumsum(axis=1)
        for e in range(4):
            est = want[4 * e]
            w = wfun(est)
            want[4 * e + 2] = [fo.interp_rows([est[i] + w[i]], grid, cdfs[i])[0] - fo.interp_rows([est[i] - w[i]], grid, cdfs[i])[0]
                               for i in range(N)]
    assert np.isnan(want[2, 1:7]).all() and np.isfinite(want[6, 3]) and np.isfinite(want[[2, 6, 10, 14]][:, CLEAN]).all()
    close_stats(got, want, 1e-10, 1e-12, 'window', rows=[r for r in range(21) if r % 4 != 2 or r > 15])
    close_stats(got, want, 1e-9, 1e-11, 'window', rows=(2, 6, 10, 14))
    assert np.array_equal(a, g21['edge'], equal_nan=True)


def test_infinite_rows_against_the_oracle():
    """rows of -inf (np.argmax / np.argmin of a constant row: its first point), with one +inf entry (the CDF is finite before it) and
    with -inf entries among finite ones, no renormalisation, next to clean rows"""
    from frankenz_amd.pdf import pdfs_summarize
    grid, pd = small_stack(65, 9, 77)
    pd /= pd.sum(axis=1)[:, None]
    pd[1] = -np.inf
    pd[2, 20] = np.inf
    pd[3, [0, 1, 40]] = -np.inf
    pd[5, 64] = np.inf
    pd[6, 2:] = -np.inf                       # the lanes from 1 on hold -inf only
    u = np.random.RandomState(5).rand(len(pd))
    for kern in ('lorentz', 'tophat'):
        a, b = pd.copy(), pd.copy()
        got = flat(pdfs_summarize(a, grid, renormalize=False, rstate=Uniforms(u), pkern=kern))
        with np.errstate(all='ignore'):
            want = flat(fo.pdfs_summarize(b, grid, renormalize=False, urand=u, pkern=kern))
        assert want[8, 1] == grid[0] and want[8, 2] == grid[20]
        assert np.array_equal(np.isinf(got), np.isinf(want)) and np.array_equal(got[np.isinf(want)], want[np.isinf(want)])
        close_stats(got, want, 1e-9, 1e-11, 'inf ' + kern)


# ---- 2. grids shorter than a wave, tile edges ---------------------------------------------------------------------------------------
def small_stack(G, N, seed):
    rs = np.random.RandomState(seed)
    grid = np.linspace(0., 3., G)
    mu = rs.uniform(0.1, 2.9, N)[:, None]
    sg = rs.uniform(0.05, 0.9, N)[:, None]
    return grid, np.exp(-0.5 * ((grid[None, :] - mu) / sg) ** 2) + 0.3 * np.exp(-0.5 * ((grid[None, :] - (3. - mu)) / (0.5 * sg)) ** 2) + 1e-3


SHAPES = [(G, 133) for G in (2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129)] + [(65, N) for N in (1, 4, 5, 127, 128, 129)]


@pytest.mark.parametrize('kern', ['lorentz', 'tophat'])
@pytest.mark.parametrize('G,N', SHAPES)
def test_small_grids_and_tile_edges(G, N, kern):
    """G from the entry point's lower limit of 2 across the 16-deep K step, the wave (a lane owns ceil(G / 64) points) and the
    128-column tile; N = 133: one full 128-row GEMM tile plus 5, 33 four-wave blocks plus one; N from 1 across the block and the tile.
    The four "best" rows where the arg-min of the risk row is decisive; elsewhere the device's choice is a grid point whose risk is
    the row's minimum within 1e-9, and its best_risk that entry.  Non-decisive shares measured with the oracle (lorentz: 0 at every
    shape; tophat, whose loss has exact ties: 0.068 at G = 2, 0.015 at 3, 0.0075 at 17, 0.023 at 63, 0.113 at 129, 0.0078 at
    (65, 128), 0 elsewhere): the cap is 0.15."""
    from frankenz_amd.pdf import pdfs_summarize
    grid, pd = small_stack(G, N, G if N == 133 else 1000 + N)
    u = np.random.RandomState(9).rand(N)
    a, b = pd.copy(), pd.copy()
    got = flat(pdfs_summarize(a, grid, rstate=np.random.RandomState(9), pkern=kern))
    want = flat(fo.pdfs_summarize(b, grid, urand=u, pkern=kern))
    what = 'G=%d N=%d %s' % (G, N, kern)
    close(a, b, 1e-14, 0, what + ' rows in place')
    risk = np.dot(b, fo.loss_matrix(grid, kern))
    srt = np.sort(risk, axis=1)
    decisive = (srt[:, 1] - srt[:, 0]) > 1e-9 * np.abs(srt[:, 0])
    print('%-58s non-decisive share %.4f' % (what, 1. - decisive.mean()))
    assert 1. - decisive.mean() <= 0.15
    close_stats(got, want, 1e-9, 1e-11, what, rows=[r for r in range(21) if r not in BEST])
    close_stats(got[:, decisive], want[:, decisive], 1e-9, 1e-11, what, rows=BEST)
    for i in np.flatnonzero(~decisive):
        k = np.flatnonzero(grid == got[12, i])
        assert len(k) == 1, (what, i)
        assert risk[i, k[0]] - srt[i, 0] <= 1e-9 * np.abs(srt[i, 0]), (what, i)
        np.testing.assert_allclose(got[15, i], risk[i, k[0]], rtol=1e-9, atol=1e-11)


# ---- 3. pdfs_resample ---------------------------------------------------------------------------------------------------------------
def np_resample(pdfs, og, ng, renormalize, left, right):
    with np.errstate(all='ignore'):
        out = np.array([np.interp(ng, og, p, left=left, right=right) for p in pdfs])
        if renormalize:
            out /= out.sum(axis=1)[:, None]
    return out


@pytest.mark.parametrize('N', [1, 5])
@pytest.mark.parametrize('G,Gn', [(1, 1), (2, 63), (65, 64), (65, 65), (701, 130)])
def test_resample_against_numpy_row_by_row(G, Gn, N):
    """new grids out of order that hold a NaN, points on old nodes and on both ends and points beyond both ends (``left`` / ``right``
    set); a zero row and a row with NaN entries, which ``renormalize=True`` turns into NaN rows"""
    from frankenz_amd.pdf import pdfs_resample
    rs = np.random.RandomState(100 * G + Gn)
    og = np.linspace(0., 3., G) if G > 1 else np.array([0.5])
    pd = rs.rand(N, G) + 0.1
    if N > 1:
        pd[2] = 0.
        pd[3, rs.choice(G, min(G, 3), replace=False)] = np.nan
    special = [np.nan, og[0], og[-1], og[G // 2], og[0] - 0.25, og[-1] + 0.25, og[G // 3]][:Gn]
    ng = np.concatenate([special, rs.uniform(og[0] - 0.3, og[-1] + 0.3, Gn - len(special))])
    ng = ng[rs.permutation(Gn)]
    what = 'resample G=%d Gn=%d N=%d' % (G, Gn, N)
    got = pdfs_resample(pd.copy(), og, ng, renormalize=False, left=-1., right=7.)
    close(got, np_resample(pd, og, ng, False, -1., 7.), 1e-13, 0, what + ' nan point')
    # without the NaN point (it makes every row sum NaN): the zero row and the NaN row alone go NaN under renormalisation
    ng2 = np.where(np.isnan(ng), og[-1] * 0.37 + og[0] * 0.63, ng)
    for kw in (dict(renormalize=True, left=0., right=0.), dict(renormalize=True, left=-1., right=7.), dict(renormalize=False, left=0.25, right=0.5)):
        want = np_resample(pd, og, ng2, kw['renormalize'], kw['left'], kw['right'])
        if N > 1 and kw['renormalize']:
            assert np.isnan(want[3]).all() and np.isfinite(want[[0, 1, 4]]).all()
            assert np.isnan(want[2]).all() or kw['left'] != 0.               # (the zero row has a sum where `left` / `right` give it one)
        close(pdfs_resample(pd.copy(), og, ng2, **kw), want, 1e-13, 0, what + ' %r' % sorted(kw.values(), key=str))


def test_resample_g21_nan_point_and_duplicate_node(g21):
    from frankenz_amd.pdf import pdfs_resample
    g = g21
    close(pdfs_resample(g['edge'].copy(), g['grid'], g['new_grid'], renormalize=False, left=-1., right=7.), g['resampled_lr'], 1e-13, 0,
          'g21 resampled_lr')
    close(pdfs_resample(g['edge'].copy(), g['grid'], g['new_grid']), g['resampled'], 1e-13, 0, 'g21 resampled')
    close(pdfs_resample(g['edge'].copy(), g['grid'], g['new_grid_finite']), g['resampled_finite'], 1e-13, 0, 'g21 resampled_finite')
    got = pdfs_resample(g['dup_pdfs'].copy(), g['dup_grid'], g['dup_new_grid'], renormalize=False, left=-1., right=7.)
    close(got, g['dup_resampled_lr'], 1e-13, 0, 'g21 duplicate node')
    assert g['dup_new_grid'][0] == 1. and got[0, 0] == 5.                   # on the duplicated node: the later entry
    close(pdfs_resample(g['dup_pdfs'].copy(), g['dup_grid'], g['dup_new_grid']), g['dup_resampled'], 1e-13, 0, 'g21 duplicate node, renormalised')


# ---- 4. loglike_nz ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 3, 4, 5, 1025])
@pytest.mark.parametrize('G', [1, 63, 64, 65])
def test_loglike_nz_small_shapes(G, N):
    """rows of sum 1/2 and an n(z) of sum 1, so that every overlap is below 1 and every log negative (no cancellation in the total);
    N = 1025 gives 257 block partials, one more than k_sum_partials' 256 threads take in a pass; pairs at both ends of the grid in both
    orders; a row orthogonal to n(z) (overlap exactly 0, -inf) and a row the pair step drives negative (NaN, as numpy)"""
    from frankenz_amd.samplers import loglike_nz
    rs = np.random.RandomState(1000 * G + N)
    pd = 0.5 * rs.dirichlet(np.full(G, 0.8), size=N)
    nz = rs.dirichlet(np.full(G, 1.5))
    h = G // 2
    nz[:h] = 0.                                         # the first half of the grid carries no n(z)
    nz /= nz.sum()
    what = 'loglike_nz G=%d N=%d' % (G, N)
    for pair, step in ((None, None), ((0, G - 1), 1e-3), ((G - 1, 0), 1e-3)):
        ll, ov = loglike_nz(nz, pd, return_overlap=True, pair=pair, pair_step=step)
        wl, wo = fo.loglike_nz(nz, pd, pair, step)
        assert (wo > 0).all() and (wo < 1).all()
        close(ov, wo, 1e-13, 0, what + ' overlap %r' % (pair,))
        close(ll, wl, 1e-13, 0, what + ' total %r' % (pair,))
    # a row orthogonal to n(z)
    q = pd.copy()
    q[0] = 0.
    q[0, :max(h, 1)] = 0.5 / max(h, 1)
    if G == 1:
        q[0] = 0.
    ll, ov = loglike_nz(nz, q, return_overlap=True)
    with np.errstate(all='ignore'):
        wl, wo = fo.loglike_nz(nz, q)
    assert wo[0] == 0. and wl == -np.inf
    assert ov[0] == 0. and ll == -np.inf
    close(ov, wo, 1e-13, 0, what + ' overlap, orthogonal row')
    # ... which the pair step drives negative: all its mass on point 0, where n(z) is zero
    if G > 1:
        q[0] = 0.
        q[0, 0] = 0.5
        ll, ov = loglike_nz(nz, q, return_overlap=True, pair=(G - 1, 0), pair_step=1e-3)
        with np.errstate(all='ignore'):
            wl, wo = fo.loglike_nz(nz, q, (G - 1, 0), 1e-3)
        assert wo[0] < 0 and np.isnan(wl)
        assert np.isnan(ll)
        close(ov, wo, 1e-13, 0, what + ' overlap, negative row')
