"""Sparse fits on the GPU (csrc/fz_sparse.h, docs/sparse_fits.md) against the NumPy law of tests/_sparse_ref.py.  Every comparison on
given rows is exact: indices, counts, values, padding.  On fitted problems `fit_sparse` is the law applied to the device's own
`fit()` planes, exactly; against the oracle's rows the indices match for every object that tests/test_sparse_host.py does not mark
fragile (none, on the problems here)."""
import numpy as np
import pytest

import _draw_ref as dr
import _mw_ref as mw
import _sparse_ref as sr
from conftest import DevArray

pytestmark = pytest.mark.gpu

WS = (1, 2, 63, 64, 65, 256, 257, 1024, 4096)
CUT3 = np.log(1e-3)
FITS = ('fit_lnprior', 'fit_lnlike', 'fit_lnprob', 'fit_Ndim', 'fit_chi2', 'fit_scale', 'fit_scale_err')
PLANE_OF = dict(fit_lnprior='lnprior', fit_lnlike='lnlike', fit_lnprob='lnprob', fit_Ndim='Ndim', fit_chi2='chi2', fit_scale='scale',
                fit_scale_err='scale_err')


class Fixed(object):
    """a generator whose uniforms are given"""

    def __init__(self, u):
        self.u = u

    def rand(self, *shape):
        assert shape == self.u.shape
        return self.u.copy()


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def sparsify(rows, W, lncut):
    """-> the dict of sr.sparse_ref.  Through pdf.sparsify_logwt where a wt_thresh gives the cut, else through the engine"""
    from frankenz_amd import pdf
    if lncut == -np.inf or lncut == CUT3:
        sf = pdf.sparsify_logwt(rows, Nkeep=W, wt_thresh=0. if lncut == -np.inf else 1e-3)
        assert sf.NMODEL == rows.shape[1] and sf.fit_lnlike is None and sf.fit_chi2 is None
        return dict(neighbors=sf.neighbors, Nneighbors=sf.Nneighbors, vals=sf.fit_lnprob, lmap=sf.lmap, levid=sf.levid, lnkept=sf.lnkept)
    N = len(rows)
    out = dict(neighbors=np.zeros((N, W), dtype=np.int64), Nneighbors=np.zeros(N, dtype=np.int64), vals=np.zeros((N, W)), lmap=np.zeros(N),
               levid=np.zeros(N), lnkept=np.zeros(N))
    engine().sparsify_logwt(rows, W, lncut, out['neighbors'], out['Nneighbors'], vals=out['vals'], lmap=out['lmap'], levid=out['levid'],
                            lnkept=out['lnkept'], M=rows.shape[1])
    return out


def draw_gof(rows):
    """lmap / levid as Engine.draw_logwt reports them"""
    N = len(rows)
    idx = np.zeros((N, 1), dtype=np.int64); lmap, levid = np.zeros(N), np.zeros(N)
    engine().draw_logwt(rows, 1, idx, key=(1, 2), lmap=lmap, levid=levid)
    return lmap, levid


class Ref(object):
    """the law at W = 4096 once per (rows, cut); smaller caps are its first columns (the prefix property, tests/test_sparse_host.py)"""

    def __init__(self, rows, lncut):
        self.full = sr.sparse_ref(rows, 4096, lncut)

    def at(self, W):
        f = self.full
        vals = f['vals'][:, :W]
        with np.errstate(invalid='ignore'):
            lnkept = np.array([sr.logsumexp(v[:n]) if n else -np.inf for v, n in zip(vals, np.minimum(f['Nneighbors'], W))])
        return dict(neighbors=f['neighbors'][:, :W], Nneighbors=np.minimum(f['Nneighbors'], W), vals=vals, lnkept=lnkept)


def assert_exact(got, ref):
    for k in ('neighbors', 'Nneighbors', 'vals'):
        assert got[k].dtype == ref[k].dtype
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    np.testing.assert_allclose(got['lnkept'], ref['lnkept'], rtol=1e-12, atol=0)


def check_rows(rows, lncuts, Ws=WS):
    lmap, levid = draw_gof(rows)
    for lncut in lncuts:
        ref = Ref(rows, lncut)
        for W in Ws:
            got = sparsify(rows, W, lncut)
            assert_exact(got, ref.at(W))
            np.testing.assert_array_equal(got['lmap'], lmap); np.testing.assert_array_equal(got['levid'], levid)    # bit for bit (nan == nan)


# ---- rows given ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L,N', [(1, 1), (1, 37), (63, 3), (64, 37), (65, 37), (255, 1), (256, 37), (257, 37), (513, 37), (4096, 37), (4097, 37),
                                 (70001, 3)])
def test_hand_made_rows(L, N):
    """every row kind of _draw_ref.hand_rows (-inf ends and whole segments, a single entry with mass, entries 800 below the max, which
    are eligible without a cut), every cap from 1 to 4096, W > L included"""
    check_rows(dr.hand_rows(L, 3, N)[0], (-np.inf, CUT3))


def test_rows_without_a_posterior():
    for L in (257, 4097):
        rows = dr.no_posterior_rows(L)[0]
        got = sparsify(rows, 64, -np.inf)
        np.testing.assert_array_equal(got['Nneighbors'], [0, 0, 0, 64])
        assert (got['neighbors'][:3] == -99).all() and (got['vals'][:3] == -np.inf).all() and (got['lnkept'][:3] == -np.inf).all()
        check_rows(rows, (-np.inf, CUT3), Ws=(1, 64, 4096))


@pytest.mark.parametrize('L', [257, 4097, 70001])
def test_rows_whose_difficulty_is_the_order(L):
    """a constant row, tie groups that straddle the W-th place, equal values at the segment and geometry seams, the maximum repeated, a
    row sorted ascending (the worst case for a rising bar) and one descending; with lncut = -1e-300 only ties of the maximum remain"""
    rows = sr.special_rows(L)
    check_rows(rows, (-np.inf, CUT3, -1e-300), Ws=(1, 2, 64, 257, 4096) if L > 4097 else WS)
    got = sparsify(rows, 64, -1e-300)
    ties = (rows == rows.max(axis=1, keepdims=True)).sum(axis=1)
    assert ties[0] == L and ties[2] == ties[3] == 1 and ties[4] == sum(j < L for j in (255, 256, 257, 4095, 4096, 4097)) and ties[5] == 7
    np.testing.assert_array_equal(got['Nneighbors'], np.minimum(ties, 64))


@pytest.mark.parametrize('L', [4096, 5000])
def test_exactly_as_many_eligible_as_the_cap(L):
    """E = W - 1, W, W + 1 and E >> W under a cut, in both geometries"""
    rs = np.random.RandomState(12)
    for W in WS:
        Es = [e for e in (max(1, W - 1), W, W + 1, L) if e <= L]
        rows = np.full((len(Es), L), -20.)
        for i, E in enumerate(Es):
            at = rs.permutation(L)[:E]
            rows[i, at] = -rs.uniform(0., 6., E); rows[i, at[0]] = 0.
        got = sparsify(rows, W, CUT3)
        np.testing.assert_array_equal(got['Nneighbors'], np.minimum(Es, W))
        assert_exact(got, Ref(rows, CUT3).at(W))


def test_an_entry_at_the_cut_is_excluded_and_the_next_double_is_kept():
    for L, lncut in ((257, CUT3), (4097, -6.5), (63, -0.25)):
        row, (at, above) = sr.cut_rows(L, lncut)
        W = min(L, 4096)                                              # (more than the row's eligible entries)
        got = sparsify(row, W, lncut)
        kept = set(got['neighbors'][0, :got['Nneighbors'][0]])
        assert got['Nneighbors'][0] < W and at not in kept and above in kept
        assert_exact(got, Ref(row, lncut).at(W))


def test_pointers_chunking_object_order_and_geometry_do_not_change_a_row(monkeypatch):
    """host pointers under a 1 MiB workspace limit (chunks of a few objects) against device pointers; a permutation of the objects;
    both launch geometries: bit for bit"""
    eng = engine()
    for L in (513, 8193):
        rows = np.concatenate([dr.hand_rows(L, 3, 37)[0], sr.special_rows(L)])
        N, W = len(rows), 300
        base = sparsify(rows, W, CUT3)
        keys = ('neighbors', 'Nneighbors', 'vals', 'lmap', 'levid', 'lnkept')

        def same(got, sel=slice(None)):
            for k in keys:
                np.testing.assert_array_equal(np.asarray(got[k]), base[k][sel], err_msg=k)

        before = eng.workspace_limit()
        eng.set_workspace_limit(1 << 20)
        try:
            if L > 4096:
                assert (1 << 20) // (L * 8 + 2 * W * 8 + 32) < N // 2
            same(sparsify(rows, W, CUT3))
        finally:
            eng.set_workspace_limit(before)
        dev = dict(neighbors=DevArray(np.zeros((N, W), dtype=np.int64)), Nneighbors=DevArray(np.zeros(N, dtype=np.int64)),
                   vals=DevArray(np.zeros((N, W))), lmap=DevArray(np.zeros(N)), levid=DevArray(np.zeros(N)), lnkept=DevArray(np.zeros(N)))
        eng.sparsify_logwt(DevArray(rows), W, CUT3, dev['neighbors'], dev['Nneighbors'], vals=dev['vals'], lmap=dev['lmap'], levid=dev['levid'],
                           lnkept=dev['lnkept'], n=N, M=L)
        same({k: to_host(dev[k], base[k].dtype) for k in keys})
        perm = np.random.RandomState(5).permutation(N)
        same(sparsify(rows[perm], W, CUT3), perm)
        monkeypatch.setenv('FZ_SPARSE_WPO', '4' if L <= 4096 else '1')
        same(sparsify(rows, W, CUT3))
        monkeypatch.delenv('FZ_SPARSE_WPO')


def to_host(a, dtype):
    from frankenz_amd._lib import check, ptr
    eng = engine()
    out = np.empty(a.shape, dtype=dtype)
    check(eng.lib.fz_dev_copy(eng.h, ptr(out), a.data_ptr(), out.nbytes))
    return out


# ---- objects given: fit_sparse ---------------------------------------------------------------------------------------------------------
def fitted(tag):
    """-> (X, Xe, Xm, Y, Ye, Ym, lprob_func, lprob_kwargs, track_scale, the oracle's planes)"""
    import frankenz_oracle as fo
    from frankenz_amd import pdf
    from frankenz_amd.pdf import lerp_cells
    if tag.startswith('masked'):
        X, Xe, Xm, Y, Ye, Ym, _ = dr.masked_problem(int(tag[6:]))
        return X, Xe, Xm, Y, Ye, Ym, None, {}, False, fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym)
    if tag.startswith('prior'):
        X, Xe, Xm, Y, Ye, Ym, tab, prow, vals, grid, coord, _ = dr.prior_problem()
        kw = {'free_scale': True} if tag.endswith('-C') else {}
        if tag.startswith('prior-table'):
            func, lp = pdf.logprob_prior(tab, rows=prow), tab[prow]
        else:
            r, f = lerp_cells(grid, coord)
            func, lp = pdf.logprob_prior_lerp(vals, grid, coord), np.log((1 - f)[:, None] * vals[r] + f[:, None] * vals[r + 1])
        return X, Xe, Xm, Y, Ye, Ym, func, kw, False, fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, lnprior=lp, **kw)
    if tag == 'scaleB':
        p = dr.fit_problem(dr.FIT_CASES[1])
        kw = dict(p['kw'], return_scale=True)
        return (p['X'], p['Xe'], p['Xm'], p['Y'], p['Ye'], p['Ym'], None, kw, True,
                fo.bruteforce_fit(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), p['Y'], p['Ye'], p['Ym'], track_scale=True, **kw))
    p = dr.fit_problem(dr.FIT_CASES[int(tag[3:])])
    return p['X'], p['Xe'], p['Xm'], p['Y'], p['Ye'], p['Ym'], None, p['kw'], False, dict(lnprob=p['rows'])


@pytest.mark.parametrize('tag', ['fit0', 'fit1', 'fit2', 'fit3', 'fit4', 'fit5', 'masked5', 'masked12', 'masked32', 'prior-table', 'prior-lerp',
                                 'prior-table-C', 'scaleB'])
def test_fit_sparse_is_the_law_on_the_planes(tag):
    """fit0..5: _draw_ref.FIT_CASES (modes A, B, dim_prior=False, W > Nmodel, 70 001 models, and mode C at 12 bands: fit5);
    prior-table-C: the table prior under mode C at 5 bands"""
    from frankenz_amd import BruteForce
    X, Xe, Xm, Y, Ye, Ym, func, kw, track, oracle = fitted(tag)
    N, M = len(X), len(Y)
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=func, lprob_kwargs=kw, track_scale=track, verbose=False)
    planes = {k: getattr(bf, k).copy() for k in FITS}
    lmap, levid = draw_gof(planes['fit_lnprob'])
    for W in (8, 300):
        for wt in (1e-3, 0.):
            lncut = sr.lncut_of(wt)
            sf = BruteForce(Y, Ye, Ym).fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=W, wt_thresh=wt, lprob_func=func, lprob_kwargs=kw,
                                                  track_scale=track, verbose=False)
            ref = sr.sparse_ref(planes['fit_lnprob'], W, lncut)
            assert sf.neighbors.dtype == np.int64 and sf.neighbors.shape == (N, W) and sf.NMODEL == M
            np.testing.assert_array_equal(sf.neighbors, ref['neighbors']); np.testing.assert_array_equal(sf.Nneighbors, ref['Nneighbors'])
            for k in FITS:
                got = getattr(sf, k)
                if k in ('fit_scale', 'fit_scale_err') and not track:
                    assert got is None
                    continue
                want = sr.gather_ref(planes[k], ref['neighbors'], ref['Nneighbors'], sr.PADS[PLANE_OF[k]])
                assert got.dtype == want.dtype
                np.testing.assert_array_equal(got, want, err_msg=k)                 # bit for bit the plane's value
            np.testing.assert_array_equal(sf.lmap, lmap); np.testing.assert_array_equal(sf.levid, levid)
            np.testing.assert_allclose(sf.lnkept, ref['lnkept'], rtol=1e-12, atol=0)
            assert ((sf.cover() > 0) & (sf.cover() <= 1 + 1e-12)).all()
            # against the oracle: indices for every object that is not fragile, values at the planes' tolerance
            ok = ~sr.fragile(oracle['lnprob'], W, lncut)
            assert (~ok).mean() <= sr.FRAGILE_CAP
            oref = sr.sparse_ref(oracle['lnprob'], W, lncut)
            np.testing.assert_array_equal(sf.neighbors[ok], oref['neighbors'][ok]); np.testing.assert_array_equal(sf.Nneighbors[ok], oref['Nneighbors'][ok])
            for k in FITS:
                if PLANE_OF[k] in oracle and getattr(sf, k) is not None:
                    want = sr.gather_ref(oracle[PLANE_OF[k]], oref['neighbors'], oref['Nneighbors'], sr.PADS[PLANE_OF[k]])
                    np.testing.assert_allclose(getattr(sf, k)[ok], want[ok], err_msg=k, **sr.PLANE_TOL)
    assert BruteForce(Y, Ye, Ym).fit_lnprob is None


def test_fit_sparse_touches_nothing_and_chunks_alike():
    """no attribute of the fitter changes; a 1 MiB workspace limit and device-resident objects give the same bits"""
    from frankenz_amd import BruteForce
    rs = np.random.RandomState(31)
    N, M, W = 37, 8193, 65
    X, Xe, Xm, Y, Ye, Ym = dr.photometry(rs, N, M, 5)
    bf = BruteForce(Y, Ye, Ym)
    state = dict(vars(bf))
    sf = bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=W, verbose=False)
    assert dict(vars(bf)) == state
    eng = engine()
    before = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)
    try:
        sf2 = bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=W, verbose=False)
    finally:
        eng.set_workspace_limit(before)
    sf3 = bf.fit_sparse(DevArray(X), DevArray(Xe), DevArray(Xm), Nkeep=W, verbose=False)
    for other in (sf2, sf3):
        for k in ('neighbors', 'Nneighbors', 'lmap', 'levid', 'lnkept') + FITS[:5]:
            np.testing.assert_array_equal(getattr(other, k), getattr(sf, k), err_msg=k)


def test_a_foreign_callable_gives_what_the_built_in_route_gives():
    from frankenz_amd import BruteForce, pdf
    p = dr.fit_problem(dr.FIT_CASES[0])
    bf = BruteForce(p['Y'], p['Ye'], p['Ym'])
    calls = []

    def foreign(x, xe, xm, ys, yes, yms):
        calls.append(1)
        return pdf.logprob(x, xe, xm, ys, yes, yms)

    sf = bf.fit_sparse(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), Nkeep=64, lprob_func=foreign, verbose=False)
    assert len(calls) == len(p['X'])
    ref = bf.fit_sparse(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), Nkeep=64, verbose=False)
    np.testing.assert_array_equal(sf.neighbors, ref.neighbors); np.testing.assert_array_equal(sf.Nneighbors, ref.Nneighbors)
    for k in FITS[:5]:
        np.testing.assert_allclose(getattr(sf, k), getattr(ref, k), err_msg=k, **sr.PLANE_TOL)
    assert sf.fit_scale is None and ref.fit_scale is None
    np.testing.assert_allclose(sf.levid, ref.levid, rtol=1e-9); np.testing.assert_allclose(sf.lnkept, ref.lnkept, rtol=1e-9)


# ---- consumers -------------------------------------------------------------------------------------------------------------------------
def consumer_fits(**kw):
    from frankenz_amd import BruteForce
    p = dr.fit_problem(dr.FIT_CASES[0])
    bf = BruteForce(p['Y'], p['Ye'], p['Ym'])
    return p, bf, bf.fit_sparse(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), verbose=False, **kw)


def test_predict_from_sparse_rows_is_the_dense_predict():
    from frankenz_amd import PDFDict
    p, bf, sf = consumer_fits(Nkeep=256, wt_thresh=1e-4)
    assert (sf.Nneighbors < 256).all() and (sf.Nneighbors > 0).all()           # everything above 1e-4 of the best is in the rows
    M = len(p['Y'])
    rs = np.random.RandomState(6)
    z, ze = rs.uniform(0, 6, M), np.full(M, 0.05)
    d = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    kk = {'wt_thresh': 1e-3}
    got, (lm, le) = sf.predict(z, ze, label_dict=d, kde_kwargs=kk, return_gof=True, verbose=False)
    bf.fit(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), verbose=False)
    ref = bf.predict(z, ze, label_dict=d, kde_kwargs=kk, verbose=False)
    np.testing.assert_allclose(got, ref, rtol=1e-8, atol=1e-14)
    np.testing.assert_array_equal(lm, sf.lmap)


def test_sample_from_sparse_rows():
    p, bf, sf = consumer_fits(Nkeep=64)
    N, S = len(p['X']), 33
    u = np.random.RandomState(9).rand(N, S)
    close = dr.near(sf.fit_lnprob, u, dr.SUM_TOL, sf.Nneighbors)
    assert close.mean() <= dr.NEAR_CAP
    ref, rlm, rle = dr.draw_ref(sf.fit_lnprob, u, sf.neighbors, sf.Nneighbors)
    idx, (lm, le) = sf.sample(S, rstate=Fixed(u), draws='host', return_gof=True)
    dr.assert_draws(idx, ref, sf.fit_lnprob, close, sf.neighbors, sf.Nneighbors)
    np.testing.assert_array_equal(lm, rlm); np.testing.assert_allclose(le, rle, rtol=1e-12)
    sf.sample(S, rstate=np.random.RandomState(3))
    np.testing.assert_array_equal(sf.philox_key, np.random.RandomState(3).randint(0, 2**32, size=2, dtype=np.uint32))


def test_weight_sampler_and_resident_rows():
    p, bf, sf = consumer_fits(Nkeep=64)
    M = len(p['Y'])
    alpha = np.full(M, 0.5)
    pos0 = mw.stack_start(sf.fit_lnlike, M, sf.neighbors, sf.Nneighbors)
    counts, pos, worst = mw.chain_host(sf.fit_lnlike, M, alpha, pos0, np.random.RandomState(17), 10, sf.neighbors, sf.Nneighbors)
    assert worst <= dr.NEAR_CAP
    s = sf.weight_sampler()
    assert s.NMODEL == M and s.W == 64
    s.run_mcmc(3, alpha=alpha, pos_init=pos0, thin=3, rstate=np.random.RandomState(17), verbose=False, draws='host')
    np.testing.assert_array_equal(np.array(s.sweep_counts), counts)               # every one of the 10 sweeps
    # resident=True: the same rows left on the device, used in place; its device chain is bit for bit the one on the NumPy outputs
    res = bf.fit_sparse(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), Nkeep=64, resident=True, verbose=False)
    for k in ('neighbors', 'Nneighbors', 'fit_lnlike', 'fit_lnprob'):
        assert not isinstance(getattr(res, k), np.ndarray)
        np.testing.assert_array_equal(getattr(res, k).numpy(), getattr(sf, k), err_msg=k)
    assert res.fit_chi2 is None and isinstance(res.lnkept, np.ndarray)
    np.testing.assert_array_equal(res.lnkept, sf.lnkept); np.testing.assert_array_equal(res.levid, sf.levid)
    a, b = sf.weight_sampler(), res.weight_sampler()
    for smp in (a, b):
        smp.run_mcmc(3, alpha=alpha, pos_init=pos0, thin=2, rstate=np.random.RandomState(4), verbose=False)
    assert b._dev[0] is res.fit_lnlike
    assert np.array(a.samples).tobytes() == np.array(b.samples).tobytes()
    np.testing.assert_array_equal(a.sweep_counts, b.sweep_counts)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from frankenz_amd import _lib
    from frankenz_amd.engine import like_opts
    eng = engine()
    rows = -np.random.RandomState(0).uniform(0, 5, (3, 40))

    def call(W, lncut, rows=rows, nbr='own'):
        n = len(rows)
        nb = np.full((n, max(int(W), 1)), -7, dtype=np.int64) if nbr == 'own' else nbr
        eng.sparsify_logwt(rows, W, lncut, nb, np.zeros(n, dtype=np.int64), M=rows.shape[1])
        return nb

    with pytest.raises(_lib._EXC[-5], match='FZ_SPARSE_WMAX = 4096'):
        call(4097, -1.)
    with pytest.raises(_lib._EXC[-5], match='FZ_DRAW_LMAX = 1048576'):
        call(4, -1., rows=np.zeros((1, (1 << 20) + 1)))
    for W in (0, -2):
        with pytest.raises(_lib._EXC[-4], match='Nkeep'):
            call(W, -1.)
    for cut in (0., 0.5, np.nan):
        with pytest.raises(_lib._EXC[-4], match='cut'):
            call(4, cut)
    with pytest.raises(RuntimeError, match='NULL'):
        call(4, -1., nbr=None)
    assert (call(4, -np.inf) >= 0).all()
    # the longest row and the largest cap the limits allow
    long = np.zeros((1, 1 << 20)); long[0, ::3] = -1.
    nb = call(4096, -np.inf, rows=long)
    np.testing.assert_array_equal(nb[0], np.nonzero(long[0] == 0.)[0][:4096])
    # fz_fit_sparse refuses alike, ahead of any launch
    one = np.ones((4, 5))
    eng.upload_models(one, one, one)
    nb, cnt = np.full((2, 4), -7, dtype=np.int64), np.zeros(2, dtype=np.int64)
    with pytest.raises(_lib._EXC[-5], match='FZ_SPARSE_WMAX = 4096'):
        eng.fit_sparse(one[:2].copy(), one[:2].copy(), one[:2].copy(), like_opts(None), None, 4097, -1., nb, cnt)
    with pytest.raises(_lib._EXC[-4], match='cut'):
        eng.fit_sparse(one[:2].copy(), one[:2].copy(), one[:2].copy(), like_opts(None), None, 4, 0., nb, cnt)
    with pytest.raises(RuntimeError, match='NULL'):
        eng.fit_sparse(one[:2].copy(), one[:2].copy(), one[:2].copy(), like_opts(None), None, 4, -1., None, cnt)
    assert (nb == -7).all()
