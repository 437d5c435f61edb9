"""Posterior quantiles without a GPU (docs/quantiles.md): the precondition of the bar tests/test_hip_quantiles.py holds the kernel to, on
that file's own inputs -- a float64 C in index order and in a shuffled order lies within tau of the longdouble C at the points a
longdouble bisection finds --, Cantelli's bracket around the longdouble quantile on the same inputs, the NumPy law's own edge rules,
and the refusals the Python layer raises before any device call."""
import numpy as np
import pytest

import _bins_ref as br
import _quantile_ref as qr


@pytest.fixture(autouse=True)
def the_call_under_test():
    """everything here is about one call: without it nothing in this file has a subject"""
    from frankenz_amd import pdf
    from frankenz_amd.rows import RowConsumers
    return pdf.posterior_quantiles, RowConsumers.predict_quantiles


def _rows_of(case):
    rows, nbr, nnbr, y, s = case
    for i in range(len(rows)):
        mix = qr.mixture(rows, i, y, s, nbr, nnbr, 1e-3)
        if mix is not None:
            yield i, mix


@pytest.mark.parametrize("W", br.WIDTHS)
def test_precondition_of_the_bar_and_cantelli_on_the_gpu_inputs(W):
    tau = qr.tol(W)
    nrows = 0
    for k in (0, 1):
        for zeros in (False, True):
            case = qr.width_case(W, k, zeros)
            rows, nbr, nnbr, y, s = case
            pts = np.zeros((len(rows), 2 * len(qr.PROBS)))
            for i, (w, yy, ss) in _rows_of(case):
                nrows += 1
                a, b = qr.bisect(w, yy, ss, qr.PROBS)
                a0, b0, delta = qr.hull(yy, ss)
                assert (b - a <= delta).all() and (qr.C(w, yy, ss, b) >= qr.PROBS).all()
                assert ((qr.C(w, yy, ss, a) < qr.PROBS) | (a == a0)).all()
                pts[i] = np.concatenate((a, b))
                # Cantelli's bracket, as the kernel forms it, holds the quantile
                for pk, ak, bk in zip(qr.PROBS, a, b):
                    sa, sb = qr.cantelli(w, yy, ss, pk)
                    assert sa <= bk and ak <= sb, (W, k, zeros, i, pk)
                # the hull's ends as evaluated
                assert qr.C(w, yy, ss, np.array([a0]), left=True)[0] == 0. and qr.C(w, yy, ss, np.array([b0]))[0] == 1.
            ref = br.cdf_ref(rows, y, s, pts, nbr, nnbr)[0]
            for perm in (None, np.random.RandomState(13)):
                got = br.cdf_ref(rows, y, s, pts, nbr, nnbr, dtype=np.float64, perm=perm)[0]
                br.assert_close(got, ref, W, "C at the quantiles")
    assert nrows >= 8                                                # (of 20: at W = 1 three rows of five have no entry)
    assert tau == 4. * (W / 64. + 16.) * 2. ** -53


def test_the_contract_s_three_shapes_in_the_numpy_law():
    """assert_quantiles itself: it takes the exact quantile of each shape and refuses a point off by far more than the margin"""
    y, s = np.array([0., 5., 1.]), np.array([1e-3, 1e-3, 0.])
    # one Gaussian: y + s ndtri(p)
    from scipy.special import ndtri
    rows = np.array([[0., -np.inf, -np.inf]])
    x = y[0] + s[0] * ndtri(qr.PROBS)
    with pytest.raises(AssertionError):                              # ndtri is good to a few ulp of x, not to tau / density in C
        qr.assert_quantiles((x + 1e-9)[None, :], rows, y, s, qr.PROBS)
    a, b = qr.bisect(np.ones(1, dtype=qr.LD), y[:1], s[:1], qr.PROBS)
    qr.assert_quantiles(b[None, :], rows, y, s, qr.PROBS)
    z = ndtri(qr.PROBS)                                             # (p itself is known to u: u / density in x)
    assert (np.abs(b - x) <= 4. * qr.U / (np.exp(-0.5 * z * z) / (np.sqrt(2. * np.pi) * s[0])) + 1e-17).all()
    # a point mass: the label itself, and nothing further than 2 delta from it
    rows = np.array([[-np.inf, -np.inf, 0.]])
    qr.assert_quantiles(np.array([[1., 1.]]), rows, y, s, [0.3, 0.9])
    for off in (1e-12, -1e-12):
        with pytest.raises(AssertionError):
            qr.assert_quantiles(np.array([[1. + off]]), rows, y, s, [0.3])
    # a gap: any point between the components is a quantile of the first one's mass, none inside a component is
    rows = np.array([[0., 0., -np.inf]])
    for xx in (0.1, 2.5, 4.9):
        qr.assert_quantiles(np.array([[xx]]), rows, y, s, [0.5])
    for xx in (0., 5., 5.1):
        with pytest.raises(AssertionError):
            qr.assert_quantiles(np.array([[xx]]), rows, y, s, [0.5])
    with pytest.raises(AssertionError, match="hull"):
        qr.assert_quantiles(np.array([[6.]]), rows, y, s, [1. - 1e-6])
    # rows without a posterior are nan, and only they
    rows = np.array([[0., 0., -np.inf], [np.nan, 0., 0.]])
    assert qr.assert_quantiles(np.array([[2.5], [np.nan]]), rows, y, s, [0.5], got_nskip=1) <= 1.
    with pytest.raises(AssertionError):
        qr.assert_quantiles(np.array([[2.5], [2.5]]), rows, y, s, [0.5])
    with pytest.raises(AssertionError):
        qr.assert_quantiles(np.array([[np.nan], [np.nan]]), rows, y, s, [0.5])


def test_python_layer_refusals():
    from frankenz_amd import BruteForce, NearestNeighbors, SparseFits, pdf
    rows, nbr, nnbr, y, s = qr.width_case(65, 1, False)
    N, W = rows.shape
    kw = dict(neighbors=nbr, Nneighbors=nnbr)
    q = np.array([0.16, 0.5, 0.84])
    for bad in (dict(neighbors=nbr), dict(neighbors=nbr[:4], Nneighbors=nnbr), dict(neighbors=nbr, Nneighbors=nnbr[:4]), dict()):
        with pytest.raises(ValueError):                              # (the last: dense rows of 65 entries over 1000 models)
            pdf.posterior_quantiles(rows, y, s, q, **bad)
    for args in ((rows[0], y, s, q), (rows, y[:, None], s[:, None], q), (rows, y, s[:-1], q), (rows, y, s, q[None, :]), (rows, y, s, np.zeros(0))):
        with pytest.raises(ValueError):
            pdf.posterior_quantiles(*args, **kw)
    for bad in (0., 1., -0.1, 1.5, np.nan, np.inf, [0.5, 0.], [0.5, np.nan]):
        with pytest.raises(ValueError, match="inside"):
            pdf.posterior_quantiles(rows, y, s, bad, **kw)
    for wt in (1., -0.1, 2., np.nan):
        with pytest.raises(ValueError):
            pdf.posterior_quantiles(rows, y, s, q, wt_thresh=wt, **kw)
    for k, v in ((0, np.nan), (0, np.inf), (1, -1e-300), (1, np.nan), (1, np.inf)):     # s = inf: posterior_bins takes it, this call does not
        t = [y.copy(), s.copy()]
        t[k][17] = v
        with pytest.raises(ValueError):
            pdf.posterior_quantiles(rows, t[0], t[1], q, **kw)
    t = [y.copy(), s.copy()]
    t[0][[400, 23]] = 1.7e308; t[1][[400, 23]] = 1e307
    with pytest.raises(ValueError, match="model 23"):
        pdf.posterior_quantiles(rows, t[0], t[1], q, **kw)
    for out in (np.zeros((N, 4)), np.zeros((N, 3), dtype=np.float32), np.zeros((3, N)).T, np.zeros(N)):
        with pytest.raises(ValueError):
            pdf.posterior_quantiles(rows, y, s, q, out=out, **kw)
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        pdf.posterior_quantiles(rows, y, s, np.linspace(0.1, 0.9, 257), **kw)
    # the fitters take their rows as moments() does
    Y = np.ones((4, 5))
    for f in (BruteForce(Y, Y, Y), NearestNeighbors(Y, Y, Y, K=1, rstate=np.random.RandomState(1), verbose=False)):
        with pytest.raises(ValueError, match="Fits have not been computed"):
            f.predict_quantiles(np.zeros(4), np.ones(4))
    sp = SparseFits(nbr, nnbr, 1000, np.zeros(N), np.zeros(N), np.zeros(N))
    with pytest.raises(ValueError, match="Fits have not been computed"):
        sp.predict_quantiles(y, s)
    with pytest.raises(ValueError, match="labels for"):
        sp.predict_quantiles(y[:-1], s[:-1], logwt=rows)
