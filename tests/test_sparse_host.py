"""Sparse fits, the part that needs no GPU: the NumPy law (tests/_sparse_ref.py) against an independent restatement, the prefix
property, the refusals made before any device call -- and the precondition of tests/test_hip_sparse.py, from the oracle alone: on
every fitted problem the GPU tests use, the objects whose kept set or order hangs on a difference of FIT_TOL (the only ones that
may be left out of an index comparison with the oracle) are at most 1 %."""
import numpy as np
import pytest

import _draw_ref as dr
import _sparse_ref as sr
from frankenz_amd.sparse import LMAX, WMAX, check_keep          # the package's own mapping (Nkeep, wt_thresh) -> (W, lncut)

WS = (1, 8, 64, 300)
CUTS = (1e-3, 0.)
CUT3 = check_keep(1, 1e-3)[1]


def hand_problems():
    for L, S, N in dr.HAND_CASES:
        if L <= 513:
            yield dr.hand_rows(L, S, N)[0]
    yield dr.no_posterior_rows()[0]
    for L in (1, 65, 257, 4097):
        yield sr.special_rows(L)


def test_law_against_the_stable_sort():
    for rows in hand_problems():
        for W in (1, 2, 63, 64, 65, 257):
            for lncut in (-np.inf, CUT3, -1e-300):
                a = sr.sparse_ref(rows, W, lncut)
                b = sr.sparse_ref(rows, W, lncut, order=sr.kept_order_restated)
                for k in a:
                    np.testing.assert_array_equal(a[k], b[k])
                nn, nbr, vals = a['Nneighbors'], a['neighbors'], a['vals']
                for i, r in enumerate(rows):
                    if not sr.has_posterior(r):
                        assert nn[i] == 0
                        continue
                    E = int(((r - r.max()) > lncut).sum())
                    assert nn[i] == min(W, E) >= 1 and nbr[i, 0] == np.argmax(r)          # the first maximum is the MAP column
                    k = nbr[i, :nn[i]]
                    assert len(set(k)) == nn[i] and (np.diff(vals[i, :nn[i]]) <= 0).all()
                    ties = np.diff(vals[i, :nn[i]]) == 0
                    assert (np.diff(k)[ties] > 0).all()                                     # equal values: index ascending
                    if nn[i] < len(r):                                                      # nothing left out beats what is kept
                        rest = np.setdiff1d(np.arange(len(r)), k)
                        rest = rest[(r[rest] - r.max()) > lncut]
                        assert len(rest) == 0 or r[rest].max() <= vals[i, nn[i] - 1]
                    assert (nbr[i, nn[i]:] == -99).all() and (vals[i, nn[i]:] == -np.inf).all()
                    assert a['lnkept'][i] <= a['levid'][i] + 1e-12


def test_rows_without_a_posterior_and_the_cut():
    rows = dr.no_posterior_rows()[0]
    a = sr.sparse_ref(rows, 8, -np.inf)
    np.testing.assert_array_equal(a['Nneighbors'], [0, 0, 0, 8])
    assert a['lmap'][0] == -np.inf and np.isnan(a['lmap'][1]) and a['lmap'][2] == np.inf
    # -inf entries are never eligible, entries 800 below the maximum are at lncut = -inf
    r = np.array([[-np.inf, -800., 0., -np.inf, -801.]])
    np.testing.assert_array_equal(sr.sparse_ref(r, 5, -np.inf)['neighbors'], [[2, 1, 4, -99, -99]])
    np.testing.assert_array_equal(sr.sparse_ref(r, 5, CUT3)['neighbors'], [[2, -99, -99, -99, -99]])
    # an entry exactly at m + lncut is excluded, its nextafter towards m is kept; lncut = -1e-300 keeps the ties of the maximum
    for lncut in (CUT3, -6.5):
        row, (at, above) = sr.cut_rows(257, lncut)
        k = sr.sparse_ref(row, 257, lncut)
        kept = set(k['neighbors'][0, :k['Nneighbors'][0]])
        assert at not in kept and above in kept
    rep = sr.special_rows(257)[5:6]
    k = sr.sparse_ref(rep, 64, -1e-300)
    assert k['Nneighbors'][0] == 7 and (k['vals'][0, :7] == 0.75).all() and (np.diff(k['neighbors'][0, :7]) > 0).all()


def test_prefix_property():
    for rows in hand_problems():
        for lncut in (-np.inf, CUT3):
            full = sr.sparse_ref(rows, 300, lncut)
            for W in (1, 2, 63, 64, 65, 299):
                a = sr.sparse_ref(rows, W, lncut)
                np.testing.assert_array_equal(a['neighbors'], full['neighbors'][:, :W])
                np.testing.assert_array_equal(a['vals'], full['vals'][:, :W])
                np.testing.assert_array_equal(a['Nneighbors'], np.minimum(full['Nneighbors'], W))


def test_refusals_before_any_device_call():
    from frankenz_amd import BruteForce, SparseFits, pdf
    assert (WMAX, LMAX) == (4096, 1 << 20)
    assert check_keep(256, 1e-3) == (256, np.log(1e-3)) and sr.lncut_of(1e-3) == CUT3 and sr.lncut_of(0.) == -np.inf
    assert check_keep(1, 0)[1] == -np.inf and check_keep(4096, None)[1] == -np.inf
    ones = np.ones((4, 5))
    bf = BruteForce(ones, ones, ones)
    rows = np.zeros((2, 4))
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match='Nkeep'):
            bf.fit_sparse(ones[:2], ones[:2], ones[:2], Nkeep=bad, verbose=False)
        with pytest.raises(ValueError, match='Nkeep'):
            pdf.sparsify_logwt(rows, Nkeep=bad)
    for bad in (1., 1.5, -1e-3, np.nan):
        with pytest.raises(ValueError, match='wt_thresh'):
            bf.fit_sparse(ones[:2], ones[:2], ones[:2], wt_thresh=bad, verbose=False)
        with pytest.raises(ValueError, match='wt_thresh'):
            pdf.sparsify_logwt(rows, wt_thresh=bad)
    with pytest.raises(NotImplementedError, match='FZ_SPARSE_WMAX = 4096'):
        bf.fit_sparse(ones[:2], ones[:2], ones[:2], Nkeep=4097, verbose=False)
    with pytest.raises(NotImplementedError, match='FZ_SPARSE_WMAX = 4096'):
        pdf.sparsify_logwt(rows, Nkeep=4097)
    with pytest.raises(NotImplementedError, match='FZ_DRAW_LMAX = 1048576'):
        pdf.sparsify_logwt(np.zeros((1, (1 << 20) + 1)), Nkeep=4)
    with pytest.raises(ValueError, match='logwt'):
        pdf.sparsify_logwt(np.zeros(4))
    with pytest.raises(ValueError):
        bf.fit_sparse(ones[:2], ones[:2], ones[:2], lprob_func='not callable', verbose=False)
    with pytest.raises(NotImplementedError, match='resident'):
        bf.fit_sparse(ones[:2], ones[:2], ones[:2], lprob_func=lambda *a: None, resident=True, verbose=False)
    assert bf.fit_lnprob is None and bf.NDATA is None
    # a SparseFits without the rows a consumer needs says so
    sf = SparseFits(np.full((2, 3), -99, dtype=np.int64), np.zeros(2, dtype=np.int64), 4, np.zeros(2), np.zeros(2), np.full(2, -np.inf))
    with pytest.raises(ValueError, match='Fits have not been computed'):
        sf.sample(3)
    with pytest.raises(ValueError, match='not kept'):
        sf.weight_sampler()
    with pytest.raises(ValueError, match='logwt'):
        sf.sample(3, logwt=np.zeros((2, 4)))
    with pytest.raises(ValueError, match='label_dict'):
        sf.predict(np.zeros(4), np.zeros(4))
    np.testing.assert_array_equal(SparseFits(sf.neighbors, sf.Nneighbors, 4, np.zeros(2), np.array([1., 2.]), np.array([0., 2.])).cover(),
                                  np.exp([-1., 0.]))


# ---- the precondition of the fitted GPU tests ----------------------------------------------------------------------------------------
def check_share(name, rows):
    for W in WS:
        for wt in CUTS:
            share = sr.fragile(rows, W, check_keep(W, wt)[1]).mean()
            print('%s W %d wt_thresh %g: fragile share %.4f' % (name, W, wt, share))
            assert share <= sr.FRAGILE_CAP


@pytest.mark.parametrize('case', dr.FIT_CASES, ids=dr.fit_id)
def test_fitted_problems_meet_the_precondition(case):
    check_share(dr.fit_id(case), dr.fit_problem(case)['rows'])


def test_added_problems_meet_the_precondition():
    import frankenz_oracle as fo
    from frankenz_amd.pdf import lerp_cells
    for B in (5, 12, 32):
        X, Xe, Xm, Y, Ye, Ym, u = dr.masked_problem(B)
        check_share('masked-%d' % B, fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym)['lnprob'])
    X, Xe, Xm, Y, Ye, Ym, tab, prow, vals, grid, coord, u = dr.prior_problem()
    check_share('prior-table', fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, lnprior=tab[prow])['lnprob'])
    r, f = lerp_cells(grid, coord)
    lp = np.log((1 - f)[:, None] * vals[r] + f[:, None] * vals[r + 1])
    check_share('prior-lerp', fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, lnprior=lp)['lnprob'])


def test_fragile_marks_what_it_should():
    r = np.array([[0., -1., -1. - 5e-9, -3., -9.], [0., -1., -2., -3., -9.], [0., CUT3 + 5e-9, -20., -21., -22.]])
    np.testing.assert_array_equal(sr.fragile(r, 2, -np.inf), [True, False, False])
    np.testing.assert_array_equal(sr.fragile(r, 1, -np.inf), [False, False, False])      # the close pair is beyond the first W + 1
    np.testing.assert_array_equal(sr.fragile(r, 4, CUT3), [True, False, True])
