"""Bin masses and CDFs without a GPU (docs/bins.md): `pdf.gaussian_bin` against the reference's outputs (golden g23), the NumPy law
of tests/_bins_ref.py against the reference's mixture, the refusals the Python layer raises before any device call, and the
precondition of the bars tests/test_hip_bins.py holds the kernels to."""
import numpy as np
import pytest

import _bins_ref as br
from conftest import load_golden


def test_gaussian_bin_against_the_reference():
    from frankenz_amd import gaussian_bin, pdf
    g = load_golden('g23_bins')
    assert pdf.gaussian_bin is gaussian_bin
    for edges, want in ((g['edges_u'], g['bin_u']), (g['edges_t'], g['bin_t'])):
        got = np.array([gaussian_bin(m, s, edges) for m, s in zip(g['mu'], g['std'])])
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0.)
    assert (g['mu'] < 0).any() and (g['mu'] > 7).any() and np.isin(g['mu'], g['edges_u']).sum() >= 40
    assert g['std'].min() <= 0.011 and g['std'].max() > 5.


def test_the_numpy_law_against_the_reference_mixture():
    g = load_golden('g23_bins')
    w, y, s = g['mix_w'], g['mix_y'], g['mix_s']
    rows = np.log(w)[None, :]
    assert rows.max() == 0.
    for edges, want in ((g['edges_u'], g['mix_u']), (g['edges_t'], g['mix_t'])):
        for dtype in (br.LD, np.float64):
            p, below, above, nskip = br.bins_ref(rows, y, s, edges, wt_thresh=None, dtype=dtype)
            assert nskip == 0
            br.assert_close(p[0], want / w.sum(), 500, "mixture")
            br.assert_close(np.array(p[0].sum() + below[0] + above[0]), np.array(1.), 500, "total")
    # the CDF at the edges, differenced, is the same mixture
    C, _ = br.cdf_ref(rows, y, s, g['edges_t'], wt_thresh=None)
    br.assert_close(np.diff(C[0]), g['mix_t'] / w.sum(), 500, "cdf differences", factor=2.)


def test_the_law_s_edge_rules():
    e = np.array([0., 1., 2., 4.])
    y = np.array([1., 1.5, 4., -1., 0.])
    s = np.zeros(5)
    for j, want in ((0, [0, 1, 0]), (1, [0, 1, 0]), (2, [0, 0, 0]), (3, [0, 0, 0]), (4, [1, 0, 0])):
        rows = np.full((1, 5), -np.inf); rows[0, j] = 0.
        p, below, above, _ = br.bins_ref(rows, y, s, e)
        assert list(p[0]) == want and below[0] == (j == 3) and above[0] == (j == 2)
        C, _ = br.cdf_ref(rows, y, s, e)
        assert list(C[0]) == [float(x >= y[j]) for x in e]           # the CDF itself is right-continuous
    # an entry exactly at the cut is excluded, its nextafter towards the max is kept
    cut = np.log(1e-3)
    rows = np.array([[0., cut], [0., np.nextafter(cut, 0.)]])
    p, _, _, _ = br.bins_ref(rows, np.array([0.5, 1.5]), np.array([0., 0.]), e)
    assert list(p[0]) == [1., 0., 0.] and p[1, 1] > 0. and p[1, 0] < 1.
    # rows without a posterior
    rows = np.array([[-np.inf, -np.inf], [0., np.nan], [np.inf, 0.]])
    p, below, above, nskip = br.bins_ref(rows, np.array([0.5, 1.5]), np.array([0.1, 0.1]), e)
    assert nskip == 3 and np.isnan(p).all() and np.isnan(below).all() and np.isnan(above).all()


def test_python_layer_refusals():
    from frankenz_amd import BruteForce, NearestNeighbors, SparseFits, pdf
    rows, nbr, nnbr, y, s, e = br.width_case(65, 1)
    N, W = rows.shape
    kw = dict(neighbors=nbr, Nneighbors=nnbr)
    for bad in (dict(neighbors=nbr), dict(neighbors=nbr[:4], Nneighbors=nnbr), dict(neighbors=nbr, Nneighbors=nnbr[:4]), dict()):
        with pytest.raises(ValueError):                              # (the last: dense rows of 65 entries over 1000 models)
            pdf.posterior_bins(rows, y, s, e, **bad)
        with pytest.raises(ValueError):
            pdf.posterior_cdf(rows, y, s, e, **bad)
    for args in ((rows[0], y, s, e), (rows, y[:, None], s[:, None], e), (rows, y, s[:-1], e), (rows, y, s, e[:1]), (rows, y, s, e[None, :]),
                 (rows, y, s, e[::-1].copy()), (rows, y, s, np.array([0., 1., 1., 2.])), (rows, y, s, np.array([0., np.nan, 2.])),
                 (rows, y, s, np.array([0., 1., np.inf]))):
        with pytest.raises(ValueError):
            pdf.posterior_bins(*args, **kw)
    for wt in (1., -0.1, 2., np.nan):
        with pytest.raises(ValueError):
            pdf.posterior_bins(rows, y, s, e, wt_thresh=wt, **kw)
        with pytest.raises(ValueError):
            pdf.posterior_cdf(rows, y, s, e, wt_thresh=wt, **kw)
    for out in (np.zeros((N, 9)), np.zeros((N, 8), dtype=np.float32), np.zeros((8, N)).T):
        with pytest.raises(ValueError):
            pdf.posterior_bins(rows, y, s, e, out=out, **kw)
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        pdf.posterior_bins(rows, y, s, np.arange(258.), **kw)
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        pdf.posterior_cdf(rows, y, s, np.arange(257.), **kw)
    for pts in (np.zeros((2, 3)), np.zeros((N, 3, 1)), np.zeros(0), np.array([0., np.nan]), np.full((N, 2), np.inf)):
        with pytest.raises(ValueError):
            pdf.posterior_cdf(rows, y, s, pts, **kw)
    # the fitters take their rows as moments() does
    Y = np.ones((4, 5))
    for f in (BruteForce(Y, Y, Y), NearestNeighbors(Y, Y, Y, K=1, rstate=np.random.RandomState(1), verbose=False)):
        with pytest.raises(ValueError, match="Fits have not been computed"):
            f.predict_bins(np.zeros(4), np.ones(4), e)
        with pytest.raises(ValueError, match="Fits have not been computed"):
            f.predict_cdf(np.zeros(4), np.ones(4), e)
    sp = SparseFits(nbr, nnbr, 1000, np.zeros(N), np.zeros(N), np.zeros(N))
    with pytest.raises(ValueError, match="Fits have not been computed"):
        sp.predict_bins(y, s, e)
    with pytest.raises(ValueError, match="labels for"):
        sp.predict_cdf(y[:-1], s[:-1], e, logwt=rows)


def _order_precondition(rows, y, s, e, nbr=None, nnbr=None, points=None):
    """float64 sums in index order and in a shuffled order against the longdouble sums, at the bar of the GPU tests"""
    W = rows.shape[1]
    ref = br.bins_ref(rows, y, s, e, nbr, nnbr)
    for perm in (None, np.random.RandomState(11)):
        got = br.bins_ref(rows, y, s, e, nbr, nnbr, dtype=np.float64, perm=perm)
        br.assert_bins(got[0], ref, W, got[1], got[2])
    if points is not None:
        C, _ = br.cdf_ref(rows, y, s, points, nbr, nnbr)
        for perm in (None, np.random.RandomState(12)):
            br.assert_close(br.cdf_ref(rows, y, s, points, nbr, nnbr, dtype=np.float64, perm=perm)[0], C, W, "C")


@pytest.mark.parametrize("W", br.WIDTHS)
def test_precondition_of_the_gpu_bars_sparse(W):
    for k in (0, 1):
        rows, nbr, nnbr, y, s, e = br.width_case(W, k)
        _order_precondition(rows, y, s, e, nbr, nnbr, points=br.cdf_points(65, len(rows))[W % 2])


def test_precondition_of_the_gpu_bars_bins_and_dense():
    for NB in br.NBINS:
        rows, nbr, nnbr, y, s, e = br.nbins_case(NB)
        assert len(e) == NB + 1 and (y < e[0]).any() and (y > e[-1]).any() and np.isin(y, e).any()
        bw = (e[-1] - e[0]) / NB
        assert s.min() < 2e-3 * bw and s.max() > 5. * (e[-1] - e[0])
        _order_precondition(rows, y, s, e, nbr, nnbr)
    for M in br.DENSE:
        rows, y, s, e = br.dense_case(M)
        _order_precondition(rows, y, s, e, points=e)
