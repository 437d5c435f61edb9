"""Posterior draws over the model set on the GPU (csrc/fz_draw.h, docs/draws.md) against the NumPy definition of tests/_draw_ref.py,
index for index.  tests/test_draw_host.py shows that on every problem here no draw lies close enough to a cdf value for an index
to flip legitimately; `assert_draws` would still only let such a draw move to the adjacent entry."""
import numpy as np
import pytest

import _draw_ref as dr
from conftest import EVID64, DevArray

pytestmark = pytest.mark.gpu


class Fixed(object):
    """a generator whose uniforms are given (the edges u = 0 and u = 1 - 2^-53 are not left to chance)"""

    def __init__(self, u):
        self.u = u

    def rand(self, *shape):
        assert shape == self.u.shape
        return self.u.copy()


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine()


def to_host(a, dtype):
    """a DevArray's contents"""
    from frankenz_amd._lib import check, ptr
    eng = engine()
    out = np.empty(a.shape, dtype=dtype)
    check(eng.lib.fz_dev_copy(eng.h, ptr(out), a.data_ptr(), out.nbytes))
    return out


def bruteforce(M=4):
    from frankenz_amd import BruteForce
    one = np.ones((M, 5))
    return BruteForce(one, one, one)


def gof_close(got, ref):
    np.testing.assert_allclose(got[0], ref[0], **EVID64)
    np.testing.assert_allclose(got[1], ref[1], **EVID64)


# ---- rows given: sample(logwt=rows) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', dr.HAND_CASES, ids=lambda c: 'L%d-S%d-N%d' % c)
def test_sample_on_hand_made_rows(case, monkeypatch):
    L, S, N = case
    rows, u = dr.hand_rows(L, S, N)
    close = dr.near(rows, u, dr.SUM_TOL)
    assert close.mean() <= dr.NEAR_CAP
    ref, rlm, rle = dr.draw_ref(rows, u)
    idx, gof = bruteforce().sample(S, logwt=rows, rstate=Fixed(u), draws='host', return_gof=True)
    dr.assert_draws(idx, ref, rows, close)
    gof_close(gof, (rlm, rle))
    np.testing.assert_array_equal(gof[0], rlm)                     # the max is exact
    # a draw is a function of (row, u): the other launch geometry, and rows in device memory, give the same bits
    monkeypatch.setenv('FZ_DRAW_WPO', '4' if L <= 4096 else '1')
    idx2, gof2 = bruteforce().sample(S, logwt=DevArray(rows), rstate=Fixed(u), draws='host', return_gof=True)
    monkeypatch.delenv('FZ_DRAW_WPO')
    np.testing.assert_array_equal(to_host(idx2, np.int64), idx)
    np.testing.assert_array_equal(to_host(gof2[0], np.float64), gof[0]); np.testing.assert_array_equal(to_host(gof2[1], np.float64), gof[1])


def test_rows_without_a_posterior_give_minus_one():
    rows, u = dr.no_posterior_rows()
    ref, rlm, rle = dr.draw_ref(rows, u)
    idx, (lm, le) = bruteforce().sample(u.shape[1], logwt=rows, rstate=Fixed(u), draws='host', return_gof=True)
    np.testing.assert_array_equal(idx, ref)
    assert (idx[:3] == -1).all() and (idx[3] >= 0).all()
    np.testing.assert_array_equal(lm, rlm)
    np.testing.assert_allclose(le, rle, **EVID64)


# ---- objects given: fit_sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', dr.FIT_CASES, ids=dr.fit_id)
def test_fit_sample_against_the_oracle_rows(case):
    from frankenz_amd import BruteForce
    p = dr.fit_problem(case)
    S = p['u'].shape[1]
    close = dr.near(p['rows'], p['u'], dr.FIT_TOL)
    assert close.mean() <= dr.NEAR_CAP
    bf = BruteForce(p['Y'], p['Ye'], p['Ym'])
    idx, gof = bf.fit_sample(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), S, lprob_kwargs=p['kw'], rstate=Fixed(p['u']), draws='host',
                             return_gof=True, verbose=False)
    dr.assert_draws(idx, p['idx'], p['rows'], close)
    gof_close(gof, (p['lmap'], p['levid']))
    assert bf.fit_lnprob is None                                    # nothing of (Ndata, Nmodel) is kept


def small_problem():
    return dr.fit_problem(dr.FIT_CASES[0])


def priors_of(M, N):
    from frankenz_amd import pdf
    X, Xe, Xm, Y, Ye, Ym, tab, prow, vals, grid, coord, u = dr.prior_problem()
    return (X, Xe, Xm, Y, Ye, Ym, u), pdf.logprob_prior(tab, rows=prow), pdf.logprob_prior_lerp(vals, grid, coord), tab[prow], (vals, grid, coord)


@pytest.mark.parametrize('which', ['none', 'table', 'lerp'])
def test_fit_sample_is_fit_then_sample(which):
    """bit for bit, like the reference's fit_predict == fit + predict; with a ln-prior table (P = 7, row indices) and an interpolated one"""
    import frankenz_oracle as fo
    from frankenz_amd import BruteForce
    from frankenz_amd.pdf import lerp_cells
    (X, Xe, Xm, Y, Ye, Ym, u), ptab, plerp, lp_tab, (vals, grid, coord) = priors_of(257, 37)
    func = {'none': None, 'table': ptab, 'lerp': plerp}[which]
    S = u.shape[1]
    bf = BruteForce(Y, Ye, Ym)
    idx, (lm, le) = bf.fit_sample(X.copy(), Xe.copy(), Xm.copy(), S, lprob_func=func, rstate=np.random.RandomState(5), draws='host',
                                  return_gof=True, verbose=False)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=func, verbose=False)
    idx2, (lm2, le2) = bf.sample(S, rstate=np.random.RandomState(5), draws='host', return_gof=True)
    np.testing.assert_array_equal(idx2, idx); np.testing.assert_array_equal(lm2, lm); np.testing.assert_array_equal(le2, le)
    # ... and what the oracle's rows give
    if which == 'lerp':
        r, f = lerp_cells(grid, coord)
        lp = np.log((1 - f)[:, None] * vals[r] + f[:, None] * vals[r + 1])
    else:
        lp = lp_tab if which == 'table' else None
    rows = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, lnprior=lp)['lnprob']
    uu = np.random.RandomState(5).rand(*u.shape)
    close = dr.near(rows, uu, dr.FIT_TOL)
    assert close.mean() <= dr.NEAR_CAP
    ref, rlm, rle = dr.draw_ref(rows, uu)
    dr.assert_draws(idx, ref, rows, close)
    gof_close((lm, le), (rlm, rle))


@pytest.mark.parametrize('final', ['in-kernel', 'separate'])
def test_fit_sample_mode_c_with_a_prior_table(final, monkeypatch):
    """free scale WITH model errors (mode C at 5 bands) under a ln-prior table: the prior is added in place on the ln-like state
    plane, which the iteration kernel finishes itself or (FZ_MODEC_FINAL=1) a separate k_modec_final pass does.  Against the oracle's
    rows; and under FZ_CHUNK=16 (three chunks) the call returns the same bits."""
    import frankenz_oracle as fo
    from frankenz_amd import BruteForce
    (X, Xe, Xm, Y, Ye, Ym, u), ptab, _, lp_tab, _ = priors_of(257, 37)
    S = u.shape[1]
    if final == 'separate':
        monkeypatch.setenv('FZ_MODEC_FINAL', '1')
    run = lambda: BruteForce(Y, Ye, Ym).fit_sample(X.copy(), Xe.copy(), Xm.copy(), S, lprob_func=ptab, lprob_kwargs={'free_scale': True},
                                                   rstate=np.random.RandomState(5), draws='host', return_gof=True, verbose=False)
    idx, (lm, le) = run()
    rows = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, lnprior=lp_tab, free_scale=True)['lnprob']
    uu = np.random.RandomState(5).rand(*u.shape)
    close = dr.near(rows, uu, dr.FIT_TOL)
    assert close.mean() <= dr.NEAR_CAP
    ref, rlm, rle = dr.draw_ref(rows, uu)
    dr.assert_draws(idx, ref, rows, close)
    gof_close((lm, le), (rlm, rle))
    monkeypatch.setenv('FZ_CHUNK', '16')
    idx2, (lm2, le2) = run()
    np.testing.assert_array_equal(idx2, idx); np.testing.assert_array_equal(lm2, lm); np.testing.assert_array_equal(le2, le)


def test_device_draws_are_philox_at_object_and_draw():
    from frankenz_amd import BruteForce
    from frankenz_amd.samplers import _philox_uniform
    p = small_problem()
    N, S = p['u'].shape
    bf = BruteForce(p['Y'], p['Ye'], p['Ym'])
    idx = bf.fit_sample(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), S, rstate=np.random.RandomState(21), verbose=False)
    np.testing.assert_array_equal(bf.philox_key, np.random.RandomState(21).randint(0, 2**32, size=2, dtype=np.uint32))
    u = np.stack([_philox_uniform(bf.philox_key, s, N) for s in range(S)], axis=1)
    close = dr.near(p['rows'], u, dr.FIT_TOL)
    assert close.mean() <= dr.NEAR_CAP
    dr.assert_draws(idx, dr.draw_ref(p['rows'], u)[0], p['rows'], close)
    # sample() from given rows draws the same way
    idx2 = bf.sample(S, logwt=p['rows'], rstate=np.random.RandomState(21))
    dr.assert_draws(idx2, dr.draw_ref(p['rows'], u)[0], p['rows'], dr.near(p['rows'], u, dr.SUM_TOL))


@pytest.mark.parametrize('draws', ['host', 'device'])
def test_chunking_and_object_order_do_not_change_a_draw(draws):
    """the same call at a workspace limit of 1 MiB (three chunks of 15 objects) and on permuted objects: bit for bit.  With the device
    generator this is what catches an object index counted from the start of the chunk."""
    from frankenz_amd import BruteForce
    rs = np.random.RandomState(31)
    N, M, S = 37, 8193, 33
    X, Xe, Xm, Y, Ye, Ym = dr.photometry(rs, N, M, 5)
    bf = BruteForce(Y, Ye, Ym)
    run = lambda x, xe, xm, seed: bf.fit_sample(x.copy(), xe.copy(), xm.copy(), S, rstate=np.random.RandomState(seed), draws=draws,
                                                return_gof=True, verbose=False)
    idx, (lm, le) = run(X, Xe, Xm, 8)
    assert (idx >= 0).all() and len(np.unique(idx)) > N
    eng = engine()
    before = eng.workspace_limit()
    eng.set_workspace_limit(1 << 20)
    try:
        assert (1 << 20) // (M * 8 + 2 * S * 8 + 16) < N // 2
        idx2, (lm2, le2) = run(X, Xe, Xm, 8)
    finally:
        eng.set_workspace_limit(before)
    assert eng.workspace_limit() == before
    np.testing.assert_array_equal(idx2, idx); np.testing.assert_array_equal(lm2, lm); np.testing.assert_array_equal(le2, le)
    perm = rs.permutation(N)
    if draws == 'host':
        u = np.random.RandomState(8).rand(N, S)
        idx3, (lm3, le3) = bf.fit_sample(X[perm].copy(), Xe[perm].copy(), Xm[perm].copy(), S, rstate=Fixed(u[perm]), draws='host',
                                         return_gof=True, verbose=False)
        np.testing.assert_array_equal(idx3, idx[perm])
    else:
        # the device's uniform belongs to the object's POSITION: the permuted call's draws are the definition's with Philox at the
        # new positions, and its ln-evidence is the row's whatever the position
        from frankenz_amd.samplers import _philox_uniform
        idx3, (lm3, le3) = run(X[perm], Xe[perm], Xm[perm], 8)
        bf.fit(X[perm].copy(), Xe[perm].copy(), Xm[perm].copy(), verbose=False)
        u = np.stack([_philox_uniform(bf.philox_key, s, N) for s in range(S)], axis=1)
        dr.assert_draws(idx3, dr.draw_ref(bf.fit_lnprob, u)[0], bf.fit_lnprob, dr.near(bf.fit_lnprob, u, dr.SUM_TOL))
    np.testing.assert_array_equal(lm3, lm[perm]); np.testing.assert_array_equal(le3, le[perm])


@pytest.mark.parametrize('B', [5, 12, 32])
def test_masked_bands_on_objects_and_models(B):
    import frankenz_oracle as fo
    from frankenz_amd import BruteForce
    X, Xe, Xm, Y, Ye, Ym, u = dr.masked_problem(B)
    rows = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym)['lnprob']
    close = dr.near(rows, u, dr.FIT_TOL)
    assert close.mean() <= dr.NEAR_CAP
    ref, rlm, rle = dr.draw_ref(rows, u)
    idx, gof = BruteForce(Y, Ye, Ym).fit_sample(X.copy(), Xe.copy(), Xm.copy(), u.shape[1], rstate=Fixed(u), draws='host',
                                               return_gof=True, verbose=False)
    dr.assert_draws(idx, ref, rows, close)
    gof_close(gof, (rlm, rle))


def test_a_foreign_callable_draws_what_the_built_in_route_draws():
    from frankenz_amd import BruteForce, pdf
    p = small_problem()
    S = p['u'].shape[1]
    bf = BruteForce(p['Y'], p['Ye'], p['Ym'])
    calls = []

    def foreign(x, xe, xm, ys, yes, yms):
        calls.append(1)
        return pdf.logprob(x, xe, xm, ys, yes, yms)

    idx, gof = bf.fit_sample(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), S, lprob_func=foreign, rstate=Fixed(p['u']), draws='host',
                             return_gof=True, verbose=False)
    assert len(calls) == len(p['X'])
    ref, rgof = bf.fit_sample(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), S, rstate=Fixed(p['u']), draws='host', return_gof=True,
                              verbose=False)
    np.testing.assert_array_equal(idx, ref)
    gof_close(gof, rgof)
    dr.assert_draws(idx, p['idx'], p['rows'], dr.near(p['rows'], p['u'], dr.FIT_TOL))


# ---- k-NN --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,k', [(5, 4), (25, 24)])
def test_knn_fit_sample_and_sample(K, k):
    from frankenz_amd import NearestNeighbors
    X, Xe, Xm, Y, Ye, Ym, S = dr.knn_problem(K, k)
    N = len(X)
    nn = NearestNeighbors(Y, Ye, Ym, K=K, rstate=np.random.RandomState(1), verbose=False)
    rs = np.random.RandomState(44)
    nn.fit(X.copy(), Xe.copy(), Xm.copy(), rstate=rs, k=k, verbose=False)
    u = rs.rand(N, S)                                               # the query draw first, then the uniforms
    nbr, cnt, rows = nn.neighbors.copy(), nn.Nneighbors.copy(), nn.fit_lnprob.copy()
    assert rows.shape == (N, K * k) and (cnt < K * k).any() and (cnt > 0).all()
    close = dr.near(rows, u, dr.SUM_TOL, cnt)
    assert close.mean() <= dr.NEAR_CAP
    ref, rlm, rle = dr.draw_ref(rows, u, nbr, cnt)
    idx, gof = nn.fit_sample(X.copy(), Xe.copy(), Xm.copy(), S, rstate=np.random.RandomState(44), k=k, draws='host', return_gof=True,
                             verbose=False)
    dr.assert_draws(idx, ref, rows, close, nbr, cnt)
    gof_close(gof, (rlm, rle))
    for i in range(N):                                              # model indices of the object's own neighbours; padding (-99) is never drawn
        assert set(idx[i]) <= set(nbr[i, :cnt[i]])
    idx2, gof2 = nn.sample(S, rstate=Fixed(u), draws='host', return_gof=True)
    np.testing.assert_array_equal(idx2, idx); np.testing.assert_array_equal(gof2[0], gof[0]); np.testing.assert_array_equal(gof2[1], gof[1])
    # the device generator: Philox at (object, draw), drawn after the query features
    from frankenz_amd.samplers import _philox_uniform
    idx3 = nn.fit_sample(X.copy(), Xe.copy(), Xm.copy(), S, rstate=np.random.RandomState(44), k=k, verbose=False)
    ud = np.stack([_philox_uniform(nn.philox_key, s, N) for s in range(S)], axis=1)
    dr.assert_draws(idx3, dr.draw_ref(rows, ud, nbr, cnt)[0], rows, dr.near(rows, ud, dr.SUM_TOL, cnt), nbr, cnt)


# ---- device-resident ---------------------------------------------------------------------------------------------------------------
def test_device_resident_objects_and_outputs():
    from frankenz_amd import BruteForce
    p = small_problem()
    N, S = p['u'].shape
    bf = BruteForce(p['Y'], p['Ye'], p['Ym'])
    idx, (lm, le) = bf.fit_sample(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), S, rstate=np.random.RandomState(3), return_gof=True,
                                  verbose=False)
    out = (DevArray(np.zeros((N, S), dtype=np.int64)), DevArray(np.zeros(N)), DevArray(np.zeros(N)))
    got = bf.fit_sample(DevArray(p['X']), DevArray(p['Xe']), DevArray(p['Xm']), S, rstate=np.random.RandomState(3), return_gof=True,
                        verbose=False, out=out)
    assert got[0] is out[0] and got[1][0] is out[1]
    np.testing.assert_array_equal(to_host(out[0], np.int64), idx)
    np.testing.assert_array_equal(to_host(out[1], np.float64), lm); np.testing.assert_array_equal(to_host(out[2], np.float64), le)
    # out= with host objects, idx alone
    only = (np.zeros((N, S), dtype=np.int64),)
    assert bf.fit_sample(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), S, rstate=np.random.RandomState(3), verbose=False, out=only) is only[0]
    np.testing.assert_array_equal(only[0], idx)
    with pytest.raises(ValueError):
        bf.fit_sample(p['X'].copy(), p['Xe'].copy(), p['Xm'].copy(), S, verbose=False, out=(np.zeros((N, S)),))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from frankenz_amd import _lib
    eng = engine()
    rows = -np.random.RandomState(0).uniform(0, 5, (3, 40))
    idx = np.full((3, 4), -7, dtype=np.int64)
    for bad in (1.5, -1e-9, np.nan):
        u = np.full((3, 4), 0.5); u[2, 3] = bad
        with pytest.raises(_lib._EXC[-4], match=r'outside \[0, 1\]'):
            eng.draw_logwt(rows, 4, idx, u=u)
        assert (idx == -7).all()                                    # refused ahead of the draw
    eng.draw_logwt(rows, 4, idx, u=np.array([[0., 1., 0.5, 1.]] * 3))   # the closed interval is accepted
    assert (idx[:, 1] == 39).all() and (idx >= 0).all()
    with pytest.raises(_lib._EXC[-5], match='FZ_DRAW_SMAX = 65536'):
        eng.draw_logwt(rows, 65537, idx, key=(1, 2))
    with pytest.raises(_lib._EXC[-4], match='Nsamples'):
        eng.draw_logwt(rows, 0, idx, key=(1, 2))
    long = np.zeros((1, (1 << 20) + 1))
    with pytest.raises(_lib._EXC[-5], match='FZ_DRAW_LMAX = 1048576'):
        eng.draw_logwt(long, 4, idx[:1], key=(1, 2))
    # the longest row and the most draws the limits allow
    one = np.zeros((1, 4096), dtype=np.int64)
    eng.draw_logwt(long[:, :1 << 20], 4096, one, key=(1, 2))
    assert one.min() >= 0 and one.max() < (1 << 20) and len(np.unique(one)) > 4000
    with pytest.raises(ValueError, match='Nsamples'):
        bruteforce().sample(0, logwt=rows)
    # a neighbour count outside [0, W]
    with pytest.raises(_lib._EXC[-3]):
        eng.draw_logwt(rows, 4, idx, key=(1, 2), neighbors=np.zeros((3, 40), dtype=np.int64), nnbr=np.array([40, 41, 0]))
