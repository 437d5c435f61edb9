"""GPU parity of the interpolated prior (docs/bpz_prior.md): ``priors.logprob_bpz`` against the reference's own ``lprob_bpz`` hook
(golden g18) and ``pdf.logprob_prior_lerp`` against the dense ``pdf.logprob_prior(np.log(values))`` route and the oracle."""
import functools

import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import load_golden

pytestmark = pytest.mark.gpu
SDSS5 = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
MODES = {'A': {}, 'A_nodim': {'dim_prior': False}, 'B': {'free_scale': True, 'ignore_model_err': True}, 'C': {'free_scale': True}}


def close(a, b, rtol=1e-9, atol=1e-11):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)


def close_ln(a, b):
    """ln of an interpolated value against np.log of the same value formed in NumPy: the argument differs by one rounding (the
    device fuses the second product into the sum: 2.3e-16 on the logarithm), log_pos is specified to 4e-16 + 2e-16 |ln x| and
    np.log itself is good to one unit in the last place, 1.2e-16 |ln x|"""
    a, b = np.asarray(a), np.asarray(b)
    np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b))
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    ok = np.isfinite(b)
    err = np.abs(a[ok] - b[ok]) - (6.3e-16 + 3.2e-16 * np.abs(b[ok]))
    print('ln-prior: max |difference| %.3g' % (np.abs(a[ok] - b[ok]).max() if ok.any() else 0.))
    assert not ok.any() or err.max() <= 0.


@functools.lru_cache(maxsize=None)
def dicts():
    from frankenz_amd import PDFDict
    grid, sg = np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500)
    return PDFDict(grid, sg), fo.KernelDict(grid, sg)


@functools.lru_cache(maxsize=None)
def problem(seed, N, M, B=5):
    rs = np.random.RandomState(seed)
    Y = rs.lognormal(1., 1., size=(M, B)) * 4; Ye = 0.05 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5[:B] * rs.randn(N, B); Xe = np.tile(SDSS5[:B], (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = rs.uniform(0.02, 0.1, M)
    return Y, Ye, Ym, X, Xe, Xm, z, ze


GRID7 = np.array([-1., 0., 0.5, 2., 2.25, 7., 11.])


@functools.lru_cache(maxsize=None)
def lerp_table(seed, N, M, special=True):
    """(table (7, M) of prior values on the uneven GRID7, coord (N,), dense (N, M) values formed in NumPy).  special: object 0 sits
    on an interior node (f == 0), object 1 on the top node (r = P - 2, f = 1), object 2 in the cell whose two rows are all zero
    (every ln-prob -inf); zeros in one row only and in both rows of another cell."""
    from frankenz_amd.pdf import lerp_cells
    rs = np.random.RandomState(seed)
    P = len(GRID7)
    table = rs.dirichlet(np.full(max(M, 2), 0.5), size=P)[:, :M].copy()
    coord = rs.uniform(GRID7[1], GRID7[-1] + 1., N)            # (some above the grid: clipped)
    if special:
        table[0] = 0.; table[1] = 0.
        table[2, 3:9] = 0.
        k = min(11, M - 1)
        table[3, k] = 0.; table[4, k] = 0.
        coord[0], coord[1], coord[2] = GRID7[3], GRID7[-1], -0.4
    r, f = lerp_cells(GRID7, coord)
    dense = (1. - f)[:, None] * table[r] + f[:, None] * table[r + 1]
    return table, coord, dense


def lnof(dense):
    with np.errstate(divide='ignore'):
        return np.log(dense)


def run_bf(prob, hook, kw, **extra):
    from frankenz_amd import BruteForce
    Y, Ye, Ym, X, Xe, Xm, z, ze = prob
    p, (lm, le) = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, lprob_func=hook, lprob_kwargs=kw,
                                                    label_dict=dicts()[0], return_gof=True, verbose=False, save_fits=False, **extra)
    return p, lm, le


@functools.lru_cache(maxsize=None)
def oracle_run(seed, N, M, mode):
    Y, Ye, Ym, X, Xe, Xm, z, ze = problem(seed, N, M)
    lp = lnof(lerp_table(seed + 100, N, M)[2])
    with np.errstate(all='ignore'):
        return fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=dicts()[1], lnprior=lp, **MODES[mode])


# ---- 3: the reference's own hook -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['A', 'B'])
def test_g18_bpz_golden(tag):
    from frankenz_amd import BruteForce, priors
    kw = MODES[tag]
    g, g7 = load_golden('g18_bpz_prior'), load_golden('g7_config1')
    Y = g7['mphot']; Ye = np.zeros_like(Y); Ym = np.ones_like(Y)
    X, Xe, Xm, z = g['X'], g['Xe'], g['Xm'], g['model_z']
    ze = np.full(len(z), 0.03)
    d, od = dicts()
    lnprior, lnlike = g['lnprior'], g[tag + '_lnlike']
    lnprob = lnlike + lnprior                            # bit for bit the reference's fit_lnprob (asserted by make_golden_bpz.py)
    assert np.isneginf(lnprior).sum() == 24 * 8 and not np.isnan(lnprob).any()
    hook = priors.logprob_bpz(z, g['model_type'], g['mag'])
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=hook, lprob_kwargs=kw, verbose=False)
    np.testing.assert_array_equal(np.isneginf(bf.fit_lnprior), np.isneginf(lnprior))
    fin = np.isfinite(lnprior)
    print('fit_lnprior: max |difference| %.3g at |ln p| up to %.4g' % (np.abs(bf.fit_lnprior[fin] - lnprior[fin]).max(),
                                                                      np.abs(lnprior[fin]).max()))
    np.testing.assert_allclose(bf.fit_lnprior[fin], lnprior[fin], rtol=1e-13, atol=1e-14)
    close(bf.fit_lnlike, lnlike); close(bf.fit_lnprob, lnprob)
    p, (lm, le) = bf.predict(z, ze, label_dict=d, return_gof=True, verbose=False)
    close(p, g[tag + '_pred'], rtol=1e-8, atol=1e-13); close(lm, g[tag + '_lmap']); close(le, g[tag + '_levid'])
    close(bf.predict(z, ze, label_dict=d, logwt=bf.fit_lnlike, verbose=False), g[tag + '_pred_like'], rtol=1e-8, atol=1e-13)
    for save_fits in (False, True):
        p, (lm, le) = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, lprob_func=hook, lprob_kwargs=kw,
                                                        label_dict=d, verbose=False, save_fits=save_fits, return_gof=True)
        close(p, g[tag + '_fp'], rtol=1e-8, atol=1e-13); close(lm, g[tag + '_lmap']); close(le, g[tag + '_levid'])
    # the grid KDE: the oracle on the reference's own ln-prior planes
    p = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, lprob_func=hook, lprob_kwargs=kw,
                                          label_grid=d.grid, verbose=False, save_fits=False)
    rp, _, _ = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_grid=od.grid, lnprior=lnprior, **kw)
    close(p, rp, rtol=1e-7, atol=1e-13)
    # generator twins and the one-object call
    gen = list(BruteForce(Y, Ye, Ym)._fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, lprob_func=hook, lprob_kwargs=kw,
                                                  label_dict=d, save_fits=False))
    close(np.array([r[0] for r in gen]), g[tag + '_fp'], rtol=1e-8, atol=1e-13)
    rows = list(BruteForce(Y, Ye, Ym)._fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=hook, lprob_kwargs=kw, save_fits=False))
    close(np.array([r[2] for r in rows]), lnprob)
    for i in (0, 4, 23):
        one = hook(X[i].copy(), Xe[i].copy(), Xm[i].copy(), Y, Ye, Ym, index=i, **kw)
        close(one[2], lnprob[i])
        np.testing.assert_array_equal(np.isneginf(one[0]), np.isneginf(lnprior[i]))
        np.testing.assert_allclose(one[0][fin[i]], lnprior[i][fin[i]], rtol=1e-13, atol=1e-14)


def test_bpz_table_builder_matches_host_functions():
    """the (1000, M) device table against priors.bpz_pz_tm at the tabulated magnitudes, models on and off the redshift nodes"""
    from frankenz_amd import priors
    rs = np.random.RandomState(3)
    M = 777
    z = rs.uniform(0., 16., M); z[:4] = [0., 15., 15. / 999 * 123, 20.]
    t = rs.randint(0, 3, M)
    hook = priors.logprob_bpz(z, t, np.array([21., 25.]))
    tab = hook.table.numpy()
    assert tab.shape == (1000, M)
    for r in (0, 1, 417, 998, 999):
        ref = priors.bpz_pz_tm(z, t, priors._MGRID[r])
        np.testing.assert_array_equal(tab[r] == 0, ref == 0)
        np.testing.assert_allclose(tab[r], ref, rtol=1e-13, atol=0)


# ---- 4: against the dense route and the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('M', [1, 256, 257, 800])
def test_lerp_vs_dense_and_oracle(M, mode):
    from conftest import DevArray
    from frankenz_amd import BruteForce
    from frankenz_amd.pdf import logprob_prior, logprob_prior_lerp
    N, kw = 33, MODES[mode]
    prob = problem(71, N, M)
    table, coord, dense = lerp_table(171, N, M)
    assert (dense[2] == 0).all() and (dense[0] == table[3]).all() and (dense[1] == table[-1]).all()
    rp, rlm, rle = oracle_run(71, N, M, mode)
    assert np.isnan(rp[2]).all() and (M == 1 or np.isfinite(rp).all(axis=1).sum() >= 20)
    dp, dlm, dle = run_bf(prob, logprob_prior(lnof(dense)), kw)
    for tab in (table, DevArray(table)):
        p, lm, le = run_bf(prob, logprob_prior_lerp(tab, GRID7, coord), kw)
        close(p, dp, rtol=1e-8, atol=1e-13); close(lm, dlm); close(le, dle)
        close(p, rp, rtol=1e-7, atol=1e-13); close(lm, rlm); close(le, rle)
    # the three planes
    Y, Ye, Ym, X, Xe, Xm, z, ze = prob
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=logprob_prior_lerp(table, GRID7, coord), lprob_kwargs=kw, verbose=False)
    close_ln(bf.fit_lnprior, lnof(dense))
    assert np.isneginf(bf.fit_lnprob[2]).all()
    bd = BruteForce(Y, Ye, Ym)
    bd.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=logprob_prior(lnof(dense)), lprob_kwargs=kw, verbose=False)
    close(bf.fit_lnprob, bd.fit_lnprob); close(bf.fit_lnlike, bd.fit_lnlike, rtol=0, atol=0)


# ---- 5: the other launch geometry of the fused kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['A', 'B'])
def test_lerp_large_chunk_geometry(mode):
    from frankenz_amd.pdf import logprob_prior, logprob_prior_lerp
    N, M = 16391, 300
    prob = problem(72, N, M)
    table, coord, dense = lerp_table(172, N, M)
    p, lm, le = run_bf(prob, logprob_prior_lerp(table, GRID7, coord), MODES[mode])
    dp, dlm, dle = run_bf(prob, logprob_prior(lnof(dense)), MODES[mode])
    assert np.isfinite(dp).all(axis=1).sum() > N // 2
    close(p, dp, rtol=1e-8, atol=1e-13); close(lm, dlm); close(le, dle)


# ---- 6: an object's result does not depend on the chunk's order --------------------------------------------------------------
@pytest.mark.parametrize('mode', ['A', 'B'])
@pytest.mark.parametrize('M', [257, 800])
def test_lerp_order_independence(M, mode):
    from frankenz_amd.pdf import logprob_prior_lerp
    N = 33
    Y, Ye, Ym, X, Xe, Xm, z, ze = problem(71, N, M)
    table, coord, _ = lerp_table(171, N, M)
    p, lm, le = run_bf((Y, Ye, Ym, X, Xe, Xm, z, ze), logprob_prior_lerp(table, GRID7, coord), MODES[mode])
    perm = np.random.RandomState(6).permutation(N)
    sp, slm, sle = run_bf((Y, Ye, Ym, X[perm], Xe[perm], Xm[perm], z, ze), logprob_prior_lerp(table, GRID7, coord[perm]), MODES[mode])
    np.testing.assert_array_equal(sp, p[perm]); np.testing.assert_array_equal(slm, lm[perm]); np.testing.assert_array_equal(sle, le[perm])


# ---- 7: nearest neighbours ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['A', 'B'])
def test_knn_lerp_vs_dense(mode):
    from frankenz_amd import NearestNeighbors
    from frankenz_amd.pdf import logprob_prior, logprob_prior_lerp
    N, M, kw = 40, 300, MODES[mode]
    Y, Ye, Ym, X, Xe, Xm, z, ze = problem(73, N, M)
    table, coord, dense = lerp_table(173, N, M)
    res = []
    for hook in (logprob_prior_lerp(table, GRID7, coord), logprob_prior(lnof(dense))):
        nn = NearestNeighbors(Y, Ye, Ym, K=5, feature_map='identity', rstate=np.random.RandomState(1), verbose=False)
        p, (lm, le) = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, lprob_func=hook, lprob_kwargs=kw,
                                     rstate=np.random.RandomState(2), k=4, label_dict=dicts()[0], return_gof=True, verbose=False)
        res.append((nn, p, lm, le))
    (a, pa, lma, lea), (b, pb, lmb, leb) = res
    np.testing.assert_array_equal(a.neighbors, b.neighbors); np.testing.assert_array_equal(a.Nneighbors, b.Nneighbors)
    close_ln(a.fit_lnprior, b.fit_lnprior)                                           # padding -inf included
    want = np.full_like(b.fit_lnprior, -np.inf)
    for i in range(N):
        n = a.Nneighbors[i]
        want[i, :n] = lnof(dense)[i, a.neighbors[i, :n]]
    np.testing.assert_array_equal(b.fit_lnprior, want)
    close(a.fit_lnprob, b.fit_lnprob); close(pa, pb, rtol=1e-8, atol=1e-13); close(lma, lmb); close(lea, leb)
    assert np.isnan(pa[2]).all() and np.isfinite(pa).all(axis=1).sum() >= 30


# ---- 8: refusals, before any kernel reads the table ----------------------------------------------------------------------------
def test_lerp_refusals():
    from frankenz_amd import BruteForce, NearestNeighbors, priors
    from frankenz_amd.engine import get_engine
    from frankenz_amd.pdf import logprob_prior_lerp
    N, M = 12, 100
    Y, Ye, Ym, X, Xe, Xm, z, ze = problem(74, N, M)
    table, coord, _ = lerp_table(174, N, M, special=False)
    P = len(GRID7)
    bf = BruteForce(Y, Ye, Ym)

    def bad_hook(what):
        hook = logprob_prior_lerp(table, GRID7, coord)
        if what == 'row':
            hook.rows[5] = P - 1
        elif what == 'neg':
            hook.rows[0] = -1
        else:
            hook.frac[7] = what
        return hook
    for what in ('row', 'neg', 1.5, -0.25, np.nan):
        with pytest.raises(RuntimeError):
            bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=bad_hook(what), verbose=False)
        with pytest.raises(RuntimeError):
            bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, lprob_func=bad_hook(what), label_dict=dicts()[0], verbose=False,
                           save_fits=False)
    nn = NearestNeighbors(Y, Ye, Ym, K=3, feature_map='identity', rstate=np.random.RandomState(1), verbose=False)
    with pytest.raises(RuntimeError):
        nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, lprob_func=bad_hook(1.5), rstate=np.random.RandomState(2), k=4,
                       label_dict=dicts()[0], verbose=False)
    with pytest.raises(ValueError):                      # the table's model count
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=logprob_prior_lerp(table[:, :99], GRID7, coord), verbose=False)
    with pytest.raises(ValueError):                      # one coordinate per object
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=logprob_prior_lerp(table, GRID7, coord[:-1]), verbose=False)
    with pytest.raises(ValueError):
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=priors.logprob_bpz(z[:99], np.zeros(99, dtype=int), coord + 22.), verbose=False)
    with pytest.raises(NotImplementedError):
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=logprob_prior_lerp(table, GRID7, coord), lprob_args=[True], verbose=False)
    with pytest.raises(ValueError):
        priors.logprob_bpz(z, np.zeros(M, dtype=int), np.array([22., np.nan]))
    # the table builder refuses cells, types and weights out of range
    from frankenz_amd.engine import DeviceArray
    eng = get_engine()
    base = np.ones((4, 5, 3))
    out = DeviceArray(eng, (4, 6))
    iz, gg, tt = np.array([0, 1, 2, 3, 0, 1], dtype=np.int32), np.array([0., .5, 1., 0., .5, 1.]), np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    eng.prior_rows_from_grid(base, iz, gg, tt, out)
    np.testing.assert_array_equal(out.numpy(), np.ones((4, 6)))
    for k, (a, v) in enumerate(((iz, 4), (iz, -1), (tt, 3), (gg, 1.25))):
        b = a.copy(); b[2] = v
        args = [iz, gg, tt]; args[[0, 0, 2, 1][k]] = b
        with pytest.raises(RuntimeError):
            eng.prior_rows_from_grid(base, args[0], args[1], args[2], out)
    # nothing was left bound: a plain run still works
    p0 = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=dicts()[0], verbose=False, save_fits=False)
    assert np.isfinite(p0).all()
