"""Posterior scoring rules without a GPU (docs/scores.md): the closed forms of the law, as tests/_scores_ref.py restates them, against
quadrature; the single-component identities and the point-mass rules; the precondition of the bars tests/test_hip_scores.py holds the
kernels to, on that file's own inputs -- float64 sums in index order and in a shuffled order lie within the bars of the longdouble
sums --; and the refusals the Python layer raises before any device call."""
import numpy as np
import pytest

import _scores_ref as sr

SQPI = np.sqrt(np.pi)


@pytest.fixture(autouse=True)
def the_call_under_test():
    """everything here is about one call: without it nothing in this file has a subject"""
    from frankenz_amd import pdf, posterior_scores
    from frankenz_amd.rows import RowConsumers
    assert posterior_scores is pdf.posterior_scores and pdf.SCORES_NMAX == sr.NMAX
    return pdf.posterior_scores, RowConsumers.predict_scores


def _mixture7():
    rs = np.random.RandomState(41)
    y, s = rs.uniform(0., 6., 7), np.exp(rs.uniform(np.log(0.05), np.log(1.5), 7))
    rows = -rs.uniform(0., 4., size=(1, 7))
    return rows, y, s


def test_closed_forms_against_quadrature_on_a_7_component_mixture():
    from scipy.integrate import quad
    from scipy.special import erfc
    rows, y, s = _mixture7()
    w = np.exp(rows[0] - rows[0].max()); w /= w.sum()
    x = np.array([-1., 2.7, y[3], 9.])
    ref = sr.scores_ref(rows, y, s, x, wt_thresh=None)
    assert ref['ninc'][0] == 7 and ref['nskip'] == 0
    pdf = lambda t: float((w * np.exp(-0.5 * ((t - y) / s) ** 2) / (np.sqrt(2. * np.pi) * s)).sum())
    cdf = lambda t: float((w * 0.5 * erfc(-(t - y) / (s * np.sqrt(2.)))).sum())
    brk = sorted(np.concatenate((y, y - 3 * s, y + 3 * s)))
    sq = quad(lambda t: pdf(t) ** 2, -20., 30., points=brk, limit=400, epsabs=1e-13, epsrel=1e-13)[0]
    assert abs(ref['sqnorm'][0] - sq) <= 1e-11 * sq
    for k, xk in enumerate(x):
        assert abs(ref['lnpdf'][0, k] - np.log(pdf(xk))) <= 1e-13 * max(1., abs(np.log(pdf(xk))))
        lo = quad(lambda t: cdf(t) ** 2, -20., xk, points=[b for b in brk if -20. < b < xk] or None, limit=400, epsabs=1e-13, epsrel=1e-13)[0]
        hi = quad(lambda t: (1. - cdf(t)) ** 2, xk, 30., points=[b for b in brk if xk < b < 30.] or None, limit=400, epsabs=1e-13, epsrel=1e-13)[0]
        assert abs(ref['crps'][0, k] - (lo + hi)) <= 1e-11 * (lo + hi), k
        assert ref['crps'][0, k] == pytest.approx(ref['term'][0, k] - ref['spread'][0], abs=1e-15)
    # the CRPS as E|X - x| - E|X - X'| / 2 by draws: a loose cross-check of the signs and the factor 1/2
    rs = np.random.RandomState(5)
    j, j2 = rs.choice(7, 400000, p=w), rs.choice(7, 400000, p=w)
    X, X2 = y[j] + s[j] * rs.randn(400000), y[j2] + s[j2] * rs.randn(400000)
    assert abs((np.abs(X - x[1]).mean() - 0.5 * np.abs(X - X2).mean()) - ref['crps'][0, 1]) < 0.01


def test_single_component_identities():
    y, s = np.array([3., -2., 1e3]), np.array([0.25, 1e-6, 40.])
    rows = np.full((3, 3), -np.inf)
    rows[np.arange(3), np.arange(3)] = 0.
    x = np.array([[3.1, 2.], [-2., -2. + 3e-6], [900., 1e3]])
    ref = sr.scores_ref(rows, y, s, x)
    for i in range(3):
        A, _ = sr.A_G(x[i] - y[i], s[i] ** 2)
        np.testing.assert_allclose(ref['crps'][i], (A - sr.LD(s[i]) / np.sqrt(sr.PI)).astype(np.float64), rtol=0, atol=4 * sr.U * s[i])
        assert ref['spread'][i] == pytest.approx(s[i] / SQPI, rel=4 * sr.U)
        assert ref['sqnorm'][i] == pytest.approx(1. / (2. * s[i] * SQPI), rel=4 * sr.U)
        z = (x[i] - y[i]) / s[i]
        np.testing.assert_allclose(ref['lnpdf'][i], -0.5 * z * z - np.log(s[i]) - 0.5 * np.log(2. * np.pi), rtol=0,
                                   atol=8 * sr.U * (1. + np.max(z * z) + abs(np.log(s[i]))))
    assert (ref['crps'] > 0).all()


def test_point_mass_rules():
    # two point masses and a Gaussian; row 0: the point masses alone, row 1: all three, row 2: equal labels with s == 0
    y, s = np.array([1., 4., 2., 1.]), np.array([0., 0., 0.5, 0.])
    rows = np.array([[np.log(0.25), 0., -np.inf, -np.inf], [0., 0., 0., -np.inf], [0., -np.inf, -np.inf, 0.]])
    x = np.array([1., 2., 4., 5.])
    ref = sr.scores_ref(rows, y, s, x, wt_thresh=None)
    assert np.isinf(ref['sqnorm']).all() and (ref['sqnorm'] > 0).all()
    # point masses alone: +inf at a label, -inf elsewhere; CRPS = E|X - x| - E|X - X'| / 2 with weights 1/5, 4/5
    np.testing.assert_array_equal(ref['lnpdf'][0], [np.inf, -np.inf, np.inf, -np.inf])
    w = np.array([0.2, 0.8])
    for k, xk in enumerate(x):
        want = (w * np.abs(y[:2] - xk)).sum() - 0.5 * 2 * w[0] * w[1] * 3.
        assert ref['crps'][0, k] == pytest.approx(want, abs=1e-15)
    assert ref['spread'][0] == pytest.approx(0.2 * 0.8 * 3., abs=1e-16)
    # a mix: +inf only at x == y_t of a point mass, finite elsewhere
    assert ref['lnpdf'][1, 0] == np.inf and ref['lnpdf'][1, 2] == np.inf and np.isfinite(ref['lnpdf'][1, [1, 3]]).all()
    assert ref['lnpdf'][1, 1] == pytest.approx(np.log(1. / 3.) - np.log(0.5) - 0.5 * np.log(2 * np.pi), abs=1e-15)
    # equal labels with s == 0: one point mass of the whole weight: CRPS = |x - 1|, no spread
    np.testing.assert_allclose(ref['crps'][2], np.abs(x - 1.), rtol=0, atol=1e-16)
    assert ref['spread'][2] == 0. and ref['ninc'][2] == 2
    # a row without a posterior
    bad = sr.scores_ref(np.array([[np.nan, 0., 0., 0.], [-np.inf] * 4]), y, s, x)
    assert bad['nskip'] == 2 and all(np.isnan(bad[k]).all() for k in ('lnpdf', 'crps', 'spread', 'sqnorm')) and (bad['ninc'] == 0).all()


def _precondition(rows, y, s, x, nbr, nnbr, ref, W, what, wt_thresh=1e-3, shuffled=True):
    b = sr.bars(ref, W)
    worst = 0.
    for perm in (None, np.random.RandomState(13))[:2 if shuffled else 1]:
        got = sr.scores_ref(rows, y, s, x, nbr, nnbr, wt_thresh=wt_thresh, dtype=np.float64, perm=perm)
        for k in ('term', 'spread', 'sqnorm', 'crps'):
            ok = np.isfinite(ref[k])
            np.testing.assert_array_equal(got[k][~ok], ref[k][~ok])
            if ok.any():
                share = np.max(np.abs(got[k][ok] - ref[k][ok]) / np.maximum(b[k][ok], 1e-300))
                assert share <= 1., (what, k, share)
                worst = max(worst, share)
    # lnpdf: a float64 evaluation of the law's exponent, summed in index order
    for i in range(len(rows)):
        got = sr._row(np.asarray(rows, dtype=np.float64), i, nbr, nnbr, wt_thresh)
        if got is None:
            continue
        w, j = got
        xi = x if x.ndim == 1 else x[i]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            q = 1. / (s[j] * np.sqrt(2.))
            z = (xi[None, :] - y[j][:, None]) * q[:, None]
            a = (np.log(w.astype(np.float64))[:, None] - z * z) - np.log(s[j])[:, None]
            a = np.where(s[j][:, None] == 0, np.where(xi[None, :] == y[j][:, None], np.inf, -np.inf), a)
            am = a.max(axis=0)
            e = np.where(a == am, 1., np.exp(a - am))
            ln = am + np.log(np.cumsum(e, axis=0)[-1]) - np.log(np.cumsum(w.astype(np.float64))[-1]) - 0.5 * np.log(2. * np.pi)
        r = ref['lnpdf'][i]
        ok = np.isfinite(r)
        np.testing.assert_array_equal(ln[~ok], r[~ok])
        if ok.any():
            share = np.max(np.abs(ln[ok] - r[ok]) / b['lnpdf'][i][ok])
            assert share <= 1., (what, 'lnpdf', i, share)
            worst = max(worst, share)
    return worst


@pytest.mark.parametrize("W,k,zeros", sr.WIDTH_CASES)
def test_precondition_of_the_bars_on_the_gpu_inputs(W, k, zeros):
    """(at 4 096 entries a row has 2.9e6 pairs and a longdouble pass takes seconds: only the M = 1000 rows are also summed in a
    shuffled order)"""
    rows, nbr, nnbr, y, s, x = sr.width_case(W, k, zeros)
    worst = _precondition(rows, y, s, x, nbr, nnbr, sr.ref_cached('width', W, k, zeros, 1e-3), W, (W, k, zeros),
                          shuffled=W < 4096 or k == 1)
    print("W = %d, M = %d: worst share of a bar %.3g" % (W, len(y), worst))
    assert worst > 0. or W <= 2


@pytest.mark.parametrize("P", sr.PCOUNTS)
def test_precondition_of_the_bars_on_the_point_counts(P):
    rows, nbr, nnbr, y, s, x = sr.pcount_case(P)
    _precondition(rows, y, s, x, nbr, nnbr, sr.ref_cached('pcount', P), 65, ('P', P))


@pytest.mark.parametrize("M", sr.DENSE + sr.DENSE4)
def test_precondition_of_the_bars_on_the_dense_rows(M):
    """(the 4 096-entry rows, 2.9e6 pairs each, are summed in index order only)"""
    rows, y, s, x = (sr.dense_case if M in sr.DENSE else sr.dense4_case)(M)
    ref = sr.ref_cached('dense' if M in sr.DENSE else 'dense4', M)
    if M in sr.DENSE4:
        assert (ref['ninc'] > 500).all() and (ref['ninc'] < 700).all()
    _precondition(rows, y, s, x[:, None], None, None, ref, M, ('dense', M), shuffled=M != 4096)


@pytest.mark.parametrize("kind", ('block', 'bits'))
def test_precondition_of_the_bars_on_the_block_and_the_bit_for_bit_rows(kind):
    rows, nbr, nnbr, y, s, x = sr.block_case() if kind == 'block' else sr.bits_case()
    n = sr.BLOCK_REF if kind == 'block' else sr.BITS_REF
    _precondition(rows[:n], y, s, x[:n].reshape(n, -1), nbr[:n], nnbr[:n], sr.ref_cached(kind), rows.shape[1], kind)


def test_the_point_mass_rule_of_tiny_errors():
    y = np.array([1., 2.])
    rows = np.zeros((1, 2))
    x = np.array([1., 1.5])
    zero = sr.scores_ref(rows, y, np.array([0., 0.3]), x)
    tiny = sr.scores_ref(rows, y, np.array([2. ** -538, 0.3]), x)
    for k in ('lnpdf', 'crps', 'spread', 'sqnorm'):
        np.testing.assert_array_equal(tiny[k], zero[k])
    assert np.isfinite(sr.scores_ref(rows, y, np.array([2. ** -536, 0.3]), x)['sqnorm']).all()


def test_python_layer_refusals():
    from frankenz_amd import BruteForce, NearestNeighbors, SparseFits, pdf
    rows, nbr, nnbr, y, s, x = sr.width_case(65, 1, False)
    N, W = rows.shape
    kw = dict(neighbors=nbr, Nneighbors=nnbr)
    for bad in (dict(neighbors=nbr), dict(neighbors=nbr[:4], Nneighbors=nnbr), dict(neighbors=nbr, Nneighbors=nnbr[:4]), dict()):
        with pytest.raises(ValueError):                              # (the last: dense rows of 65 entries over 1000 models)
            pdf.posterior_scores(rows, y, s, x, **bad)
    for args in ((rows[0], y, s, x), (rows, y[:, None], s[:, None], x), (rows, y, s[:-1], x), (rows, y, s, np.zeros((N + 1, 2))),
                 (rows, y, s, np.zeros((N, 2, 2))), (rows, y, s, np.zeros((N, 0)))):
        with pytest.raises(ValueError):
            pdf.posterior_scores(*args, **kw)
    for bad in (np.nan, np.inf, -np.inf):
        t = x.copy(); t[2, 1] = bad
        with pytest.raises(ValueError, match="finite"):
            pdf.posterior_scores(rows, y, s, t, **kw)
    for wt in (1., -0.1, 2., np.nan):
        with pytest.raises(ValueError):
            pdf.posterior_scores(rows, y, s, x, wt_thresh=wt, **kw)
    for k, v in ((0, np.nan), (0, np.inf), (1, -1e-300), (1, np.nan), (1, np.inf)):     # s = inf: posterior_bins takes it, this call does not
        t = [y.copy(), s.copy()]
        t[k][17] = v
        with pytest.raises(ValueError):
            pdf.posterior_scores(rows, t[0], t[1], x, **kw)
    for want in ((), ('lnpdf', 'pit'), 'cde'):
        with pytest.raises(ValueError, match="want"):
            pdf.posterior_scores(rows, y, s, x, want=want, **kw)
    with pytest.raises(NotImplementedError, match="FZ_BINS_MAX"):
        pdf.posterior_scores(rows, y, s, np.zeros((N, 257)), **kw)
    # the fitters take their rows as moments() does
    Y = np.ones((4, 5))
    for f in (BruteForce(Y, Y, Y), NearestNeighbors(Y, Y, Y, K=1, rstate=np.random.RandomState(1), verbose=False)):
        with pytest.raises(ValueError, match="Fits have not been computed"):
            f.predict_scores(np.zeros(4), np.ones(4), np.zeros(3))
    sp = SparseFits(nbr, nnbr, 1000, np.zeros(N), np.zeros(N), np.zeros(N))
    with pytest.raises(ValueError, match="Fits have not been computed"):
        sp.predict_scores(y, s, x)
    with pytest.raises(ValueError, match="labels for"):
        sp.predict_scores(y[:-1], s[:-1], x, logwt=rows)
