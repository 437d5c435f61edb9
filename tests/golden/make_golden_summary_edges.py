"""G21: the reference's pdfs_summarize and pdfs_resample (pdf.py:855-1074) on rows the other goldens leave out -- NaN entries, an
all-NaN row, an all-zero row -- on a grid of 65 points (one more than a wave), recorded for tests/test_oracle_golden.py and
tests/test_hip_summary_edges.py.  Run from the repository root with the reference importable (as make_golden.py is):

    python tests/golden/make_golden_summary_edges.py

Stack ``edge``: 12 two-bump rows plus a floor of 1e-3, divided by their sums, then
    row 1: NaN at column 0        row 2: NaN at column 1         row 3: NaN at column 33       row 4: NaN at column 64
    row 5: NaN at columns 10, 50  row 6: all NaN                 row 7: all zero               rows 0, 8-11: clean
so that with four objects per workgroup rows 0-3 share one and rows 4-7 another.  Every array the reference is given is stored (a
regenerated exp could differ in its last bit)."""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings('ignore')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('FRANKENZ_REFERENCE', '/root/reference'))

from frankenz import pdf as rpdf  # noqa: E402

SEED = 21


def flat(res):
    return np.array([a for grp in res[:5] for a in grp] + [res[5]])          # (21, N)


class Uniforms(object):
    """``rstate.rand()`` of pdf.py:1000 handing out a stored list, one number per object"""

    def __init__(self, u):
        self.u, self.k = u, 0

    def rand(self):
        self.k += 1
        return self.u[self.k - 1]


def main():
    rs = np.random.RandomState(SEED)
    N, G = 12, 65
    grid = np.linspace(0., 3., G)
    mu = rs.uniform(0.1, 2.9, N)[:, None]
    sg = rs.uniform(0.05, 0.9, N)[:, None]
    edge = np.exp(-0.5 * ((grid[None, :] - mu) / sg) ** 2) + 0.3 * np.exp(-0.5 * ((grid[None, :] - (3. - mu)) / (0.5 * sg)) ** 2) + 1e-3
    edge /= edge.sum(axis=1)[:, None]             # unit sums: without renormalisation the quantiles of a partly NaN row mean something
    edge[1, 0] = np.nan
    edge[2, 1] = np.nan
    edge[3, 33] = np.nan
    edge[4, 64] = np.nan
    edge[5, [10, 50]] = np.nan
    edge[6] = np.nan
    edge[7] = 0.
    # numpy.interp starts its search for a quantile at the cell of the one before it, and a search that starts among NaN nodes stays
    # there: behind the 97.5 % point of a partly NaN CDF (rows 2, 3, 5) the reference draws NaN whatever the uniform is, an accident
    # of the order of the six points.  Their uniforms are put beyond the finite part of the CDF, where the draw is NaN by any route.
    urand = rs.rand(N)
    urand[[2, 3, 5]] = 0.99
    out = dict(grid=grid, edge=edge.copy(), urand=urand)
    with np.errstate(all='ignore'):
        for ren in (True, False):
            for kern in ('lorentz', 'tophat'):
                work = edge.copy()
                res = rpdf.pdfs_summarize(work, grid, renormalize=ren, rstate=Uniforms(urand), pkern=kern)
                tag = ('ren_' if ren else 'noren_') + kern
                out[tag + '_stats'], out[tag + '_after'] = flat(res), work
                # no recorded quantile depends on numpy's search path: each one again by a call of its own
                for i, cdf in enumerate(work.cumsum(axis=1)):
                    for r, q in zip((16, 17, 4, 18, 19, 20), (0.025, 0.16, 0.5, 0.84, 0.975, urand[i])):
                        assert np.array_equal(out[tag + '_stats'][r, i], np.interp(q, cdf, grid), equal_nan=True), (tag, i, r)
        # "best" is an arg-min over a matrix product: the clean rows' minima are clear of the runner-up by far more than a summation order
        for kern in ('lorentz', 'tophat'):
            ptrue, pguess = grid.reshape(G, 1), grid.reshape(1, G)
            kg = (ptrue - pguess) / ((1. + ptrue) * 0.15)
            loss = 1. - (1. / (1. + np.square(kg)) if kern == 'lorentz' else (np.square(kg) < 1.))
            srt = np.sort(np.dot(edge[[0, 8, 9, 10, 11]], loss), axis=1)
            assert ((srt[:, 1] - srt[:, 0]) > 1e-6 * srt[:, 0]).all()
        # what a non-finite row gives in the reference: checked here so that a change of the reference shows: checked here so that a change of the reference shows
        s = out['noren_lorentz_stats']
        assert np.isfinite(s[[4, 6, 14, 16, 17], 3]).all() and np.isnan(s[[0, 1, 2, 3, 5, 7, 18, 19], 3]).all()
        assert s[8, 3] == grid[33] and s[8, 5] == grid[10] and s[8, 6] == grid[0] and (s[12, 1:7] == grid[0]).all()
        assert s[0, 7] == 0. and (s[[4, 16, 17, 18, 19, 20], 7] == grid[-1]).all()
        assert np.isfinite(s[20, [0, 4, 8, 9, 10, 11]]).all()
        r = out['ren_lorentz_stats']
        assert np.isnan(np.delete(r[:, 1:8], [8, 12], axis=0)).all() and (r[[8, 12], 1] == grid[0]).all()

        # pdfs_resample: unsorted points with a NaN, on nodes and on both ends, beyond both ends
        ng = np.array([2.5, -1., grid[21], np.nan, 3., 3.5, 0., grid[21] + 1e-7, 1., grid[63]])
        out['new_grid'] = ng
        out['resampled_lr'] = rpdf.pdfs_resample(edge.copy(), grid, ng, renormalize=False, left=-1., right=7.)
        out['resampled'] = rpdf.pdfs_resample(edge.copy(), grid, ng)                       # the NaN point makes every sum NaN
        out['new_grid_finite'] = ng[np.isfinite(ng)]
        out['resampled_finite'] = rpdf.pdfs_resample(edge.copy(), grid, out['new_grid_finite'])
        # an old grid with a duplicated node: at x = 1 the later entry
        out['dup_grid'] = np.array([0., 1., 1., 2., 3.])
        out['dup_pdfs'] = np.array([[1., 2., 5., 3., 4.], [0., 0., 0., 0., 0.]])
        out['dup_new_grid'] = np.array([1., 0.5, 1. - 1e-9, 1. + 1e-9, 0., 3., 2.5, -0.5, 3.5])
        out['dup_resampled_lr'] = rpdf.pdfs_resample(out['dup_pdfs'].copy(), out['dup_grid'], out['dup_new_grid'], renormalize=False,
                                                     left=-1., right=7.)
        out['dup_resampled'] = rpdf.pdfs_resample(out['dup_pdfs'].copy(), out['dup_grid'], out['dup_new_grid'])
    assert out['dup_resampled_lr'][0, 0] == 5. and np.isnan(out['dup_resampled'][1]).all()
    path = os.path.join(HERE, 'g21_summary_edges.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 100000, size
    print('wrote %s (%d bytes)' % (path, size))


if __name__ == '__main__':
    main()
