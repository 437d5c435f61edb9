"""GPU parity: the HIP path (through the C ABI / drop-in classes) against the
oracle and the golden vectors.  Tolerance: north_star's 1e-5 relative on
log-likelihoods and PDFs; we assert much tighter where fp64 allows it."""
import numpy as np
import pytest

import frankenz_oracle as fo
from conftest import EVID, EVID64, load_golden

pytestmark = pytest.mark.gpu

SDSS5 = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
RTOL = 1e-5            # the bar stated in BASELINE.json north_star
TIGHT = 1e-9           # what fp64 kernels actually achieve on well-conditioned rows
MODES = [(fs, ime, dp) for fs in (False, True) for ime in (False, True) for dp in (False, True)]


def close(a, b, rtol=TIGHT, atol=1e-11):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)


def dicts():
    from frankenz_amd import PDFDict
    grid, sg = np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500)
    return PDFDict(grid, sg), fo.KernelDict(grid, sg)


@pytest.mark.parametrize('mi', range(8))
def test_g1_loglike_golden(mi):
    from frankenz_amd import pdf as hp
    g = load_golden('g1_loglike')
    fs, ime, dp = MODES[mi]
    for oi in range(len(g['X'])):
        for mk, mdt in (('f', float), ('b', bool)):
            x, xe, xm = g['X'][oi].copy(), g['Xe'][oi].copy(), g['Xm'][oi].astype(mdt)
            res = hp.loglike(x, xe, xm, g['Y'], g['Ye'], g['Ym'].astype(mdt), free_scale=fs,
                             ignore_model_err=ime, dim_prior=dp, return_scale=fs)
            key = 'm%d_o%d_%s' % (mi, oi, mk)
            tol = dict(rtol=1e-7, atol=1e-9) if (fs and not ime) else dict(rtol=TIGHT, atol=1e-10)
            want = g[key + '_lnl']
            ok = np.ones(len(want), dtype=bool)
            if fs and dp:
                # free scale + dim prior with exactly ONE usable band: chi2 is 0 up to
                # rounding and a = 0, so the reference itself returns nan (chi2 == 0) or
                # -inf (chi2 ~ 1e-32) by rounding luck (x - s*y == 0 in ~54% of cases).
                # Both sides must be non-finite there; the value is not defined.
                ok = np.asarray(g[key + '_ndim']) != 1
                assert not np.isfinite(res[0][~ok]).any() and not np.isfinite(want[~ok]).any()
            close(res[0][ok], want[ok], **tol)
            np.testing.assert_array_equal(res[1], g[key + '_ndim'])
            assert res[1].dtype == g[key + '_ndim'].dtype
            close(res[2], g[key + '_chi2'], **tol)
            if fs:
                close(res[3], g[key + '_scale'], **tol)
                close(res[4], g[key + '_scale_err'], **tol)
            if mk == 'f':
                close(x, g['clean_o%d_x' % oi]); close(xe, g['clean_o%d_xe' % oi])
                close(xm, g['clean_o%d_xm' % oi])


def test_g2_mode_c_global_stop():
    from frankenz_amd import pdf as hp
    g = load_golden('g2_modec')
    for oi in range(3):
        for dp in (False, True):
            for tname, ltol in (('t4', 1e-4), ('t8', 1e-8)):
                r = hp.loglike(g['X'][oi].copy(), g['Xe'][oi].copy(), g['Xm'][oi].copy(), g['Y'],
                               g['Ye'], g['Ym'], free_scale=True, ignore_model_err=False,
                               dim_prior=dp, ltol=ltol, return_scale=True)
                k = 'o%d_dp%d_%s' % (oi, int(dp), tname)
                # identical iteration count => agreement far below ltol
                close(r[0], g[k + '_lnl'], rtol=1e-8, atol=1e-8)
                close(r[2], g[k + '_chi2'], rtol=1e-8, atol=1e-8)
                close(r[3], g[k + '_scale'], rtol=1e-8, atol=1e-10)
                close(r[4], g[k + '_scale_err'], rtol=1e-8, atol=1e-10)


def test_g4_kde_functions():
    from frankenz_amd import pdf as hp
    g = load_golden('g4_kde')
    d, _ = dicts()
    y, ys, wt, grid = g['y'], g['ys'], g['wt'], g['grid']
    close(hp.gauss_kde_dict(d, y=y, y_std=ys, y_wt=wt), g['dict_default'], atol=1e-14)
    close(hp.gauss_kde_dict(d, y=y, y_std=ys, y_wt=wt, wt_thresh=0.25), g['dict_thresh25'], atol=1e-14)
    close(hp.gauss_kde_dict(d, y=y, y_std=ys, y_wt=wt, wt_thresh=None, cdf_thresh=None),
          g['dict_nothresh'], atol=1e-14)
    close(hp.gauss_kde_dict(d, y=y, y_std=ys), g['dict_unit'], atol=1e-14)
    close(hp.gauss_kde_dict(d, y_idx=g['yi'], y_std_idx=g['ysi'], y_wt=wt), g['dict_idx'], atol=1e-14)
    close(hp.gauss_kde(y, ys, grid, y_wt=wt), g['kde_default'], atol=1e-14)
    close(hp.gauss_kde(y, ys, grid, y_wt=wt, wt_thresh=0.25), g['kde_thresh25'], atol=1e-14)
    close(hp.gauss_kde(y, ys, grid, y_wt=wt, wt_thresh=None, cdf_thresh=None), g['kde_nothresh'], atol=1e-14)
    close(hp.gauss_kde(y, ys, grid, y_wt=wt, sig_thresh=3.), g['kde_sig3'], atol=1e-14)
    close(hp.gauss_kde(g['y2'], g['ys2'], grid, y_wt=g['w2']), g['kde_tiny'], atol=1e-14)
    # the reference's CDF rule (wt_thresh=None): everything but the minimal top-K is stacked
    close(hp.gauss_kde_dict(d, y=y, y_std=ys, y_wt=wt, wt_thresh=None), g['dict_cdf'], atol=1e-14)
    close(hp.gauss_kde(y, ys, grid, y_wt=wt, wt_thresh=None), g['kde_cdf'], atol=1e-14)
    close(hp.gauss_kde_dict(d, y=y, y_std=ys, y_wt=wt, wt_thresh=None, cdf_thresh=0.2),
          fo.gauss_kde_dict(fo.KernelDict(d.grid, d.sigma_grid), y=y, y_std=ys, y_wt=wt, wt_thresh=None, cdf_thresh=0.2),
          atol=1e-14)


def test_g5_bruteforce_fit_and_predict():
    from frankenz_amd import BruteForce
    g = load_golden('g5_bruteforce')
    d, _ = dicts()
    bf = BruteForce(g['Y'], g['Ye'], g['Ym'])
    X, Xe, Xm = g['X'].copy(), g['Xe'].copy(), g['Xm'].copy()
    bf.fit(X, Xe, Xm, verbose=False)
    close(X, g['clean_X']); close(Xe, g['clean_Xe']); close(Xm, g['clean_Xm'])
    for nm in ('lnprior', 'lnlike', 'lnprob', 'Ndim', 'chi2', 'scale', 'scale_err'):
        a = getattr(bf, 'fit_' + nm)
        assert a.dtype == g['fitA_' + nm].dtype and a.shape == g['fitA_' + nm].shape
        close(a, g['fitA_' + nm])
    p, (lm, le) = bf.predict(g['z'], g['ze'], label_dict=d, return_gof=True, verbose=False)
    close(p, g['predA_dict'], atol=1e-14); close(lm, g['predA_lmap']); close(le, g['predA_levid'])
    close(bf.predict(g['z'], g['ze'], label_grid=d.grid, verbose=False), g['predA_grid'], atol=1e-14)
    close(bf.predict(g['z'], g['ze'], label_dict=d, logwt=-0.5 * bf.fit_chi2, verbose=False),
          g['predA_logwt_chi2'], atol=1e-14)
    close(bf.predict(g['z'], g['ze'], label_dict=d, verbose=False, kde_kwargs={'wt_thresh': 1e-2}),
          g['predA_thresh'], atol=1e-14)
    with pytest.raises(ValueError):
        bf.predict(g['z'], g['ze'])


FUSED = [('A', {}), ('An', {'dim_prior': False}), ('Ai', {'ignore_model_err': True}),
         ('B', {'free_scale': True, 'ignore_model_err': True}),
         ('Bn', {'free_scale': True, 'ignore_model_err': True, 'dim_prior': False}),
         ('C', {'free_scale': True, 'ignore_model_err': False}),
         ('Cn', {'free_scale': True, 'ignore_model_err': False, 'dim_prior': False})]


@pytest.mark.parametrize('tag,kw', FUSED)
@pytest.mark.parametrize('save_fits', [False, True])
def test_g5_bruteforce_fused_golden(tag, kw, save_fits):
    from frankenz_amd import BruteForce
    g = load_golden('g5_bruteforce')
    d, _ = dicts()
    bf = BruteForce(g['Y'], g['Ye'], g['Ym'])
    ts = bool(kw.get('free_scale'))
    kw2 = dict(kw, return_scale=True) if ts else dict(kw)
    p, (lm, le) = bf.fit_predict(g['X'].copy(), g['Xe'].copy(), g['Xm'].copy(), g['z'], g['ze'],
                                 label_dict=d, lprob_kwargs=kw2, return_gof=True, track_scale=ts,
                                 verbose=False, save_fits=save_fits)
    tol = dict(rtol=1e-7, atol=1e-12) if tag.startswith('C') else dict(rtol=TIGHT, atol=1e-13)
    close(p, g['fp%s_pdfs' % tag], **tol)
    close(lm, g['fp%s_lmap' % tag], **tol); close(le, g['fp%s_levid' % tag], **tol)
    if save_fits:
        close(bf.fit_lnprob, g['fp%s_lnprob' % tag], rtol=tol['rtol'], atol=1e-9)
        if ts:
            close(bf.fit_scale, g['fp%s_scale' % tag], rtol=tol['rtol'], atol=1e-10)
            close(bf.fit_scale_err, g['fp%s_scale_err' % tag], rtol=tol['rtol'], atol=1e-10)
            close(bf.fit_chi2, g['fp%s_chi2' % tag], rtol=tol['rtol'], atol=1e-9)
    else:
        assert bf.fit_lnprob is None


def test_g5_fused_grid_kde_and_generators():
    from frankenz_amd import BruteForce
    g = load_golden('g5_bruteforce')
    d, _ = dicts()
    bf = BruteForce(g['Y'], g['Ye'], g['Ym'])
    p = bf.fit_predict(g['X'].copy(), g['Xe'].copy(), g['Xm'].copy(), g['z'], g['ze'],
                       label_grid=d.grid, verbose=False, save_fits=False)
    close(p, g['fpA_grid_pdfs'], atol=1e-13)
    # generator twins yield the same rows
    rows = list(bf._fit_predict(g['X'].copy(), g['Xe'].copy(), g['Xm'].copy(), g['z'], g['ze'],
                                label_dict=d, save_fits=False))
    close(np.array([r[0] for r in rows]), g['fpA_pdfs'], atol=1e-13)
    close(np.array([r[1][1] for r in rows]), g['fpA_levid'])
    res = list(bf._fit(g['X'].copy(), g['Xe'].copy(), g['Xm'].copy()))
    close(np.array([r[1] for r in res]), g['fitA_lnlike'])
    assert len(res[0]) == 5
    prs = list(bf._predict(g['z'], g['ze'], label_dict=d))
    close(np.array([r[0] for r in prs]), g['predA_dict'], atol=1e-14)


def test_g7_config1_reference_mock():
    """config 1: the reference simulator's 1000-object SDSS mock, model-grid mode
    (free scale) and training-set mode (default likelihood)."""
    from frankenz_amd import BruteForce
    g = load_golden('g7_config1')
    d, _ = dicts()
    obs, err, mphot = g['obs'], g['err'], g['mphot']
    kw = {'free_scale': True, 'ignore_model_err': True, 'return_scale': True}
    bf = BruteForce(mphot, np.zeros_like(mphot), np.ones_like(mphot))
    p, (lm, le) = bf.fit_predict(obs.copy(), err.copy(), np.ones_like(obs), g['mz'],
                                 np.full(len(g['mz']), 0.03), label_dict=d, lprob_kwargs=kw,
                                 return_gof=True, track_scale=True, verbose=False)
    close(p[:16], g['grid_pdfs16'], rtol=1e-8, atol=1e-14)
    close(p.sum(axis=0), g['grid_pdfsum'], rtol=1e-8, atol=1e-12)
    close(lm, g['grid_lmap'], rtol=1e-10, atol=0); close(le, g['grid_levid'], **EVID)
    close(bf.fit_lnprob[:4], g['grid_lnprob_rows'], rtol=1e-9, atol=1e-9)
    close(bf.fit_lnprob.sum(axis=1), g['grid_lnprob_rowsum'], rtol=1e-9)
    close(bf.fit_scale[:4], g['grid_scale_rows'], rtol=1e-9, atol=0)
    bf = BruteForce(obs, err, np.ones_like(obs))
    p, (lm, le) = bf.fit_predict(obs.copy(), err.copy(), np.ones_like(obs), g['redshifts'],
                                 np.full(len(obs), 0.03), label_dict=d, return_gof=True,
                                 verbose=False)
    close(p[:16], g['train_pdfs16'], rtol=1e-8, atol=1e-14)
    close(p.sum(axis=0), g['train_pdfsum'], rtol=1e-8, atol=1e-12)
    close(lm, g['train_lmap'], rtol=1e-10, atol=0); close(le, g['train_levid'], **EVID)
    close(bf.fit_lnprob[:4], g['train_lnprob_rows'], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('B', [3, 5, 8, 12, 20, 32])
@pytest.mark.parametrize('kw', [{}, {'free_scale': True, 'ignore_model_err': True},
                                {'ignore_model_err': True, 'dim_prior': False}])
def test_oracle_parity_band_counts(B, kw):
    """seeded random problems vs the oracle at several band counts (padded kernels)."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(100 + B)
    M, N = 700, 37
    sig = rs.uniform(0.3, 3.0, B)
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.05 * Y * rs.uniform(0.5, 2, size=(M, B))
    # at most one masked band per model / per object, so Ndim >= B-2 >= 1
    Ym = np.ones((M, B)); hit = rs.rand(M) < 0.15; Ym[hit, rs.randint(0, B, hit.sum())] = 0
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .3, N)[:, None] + sig * rs.randn(N, B)
    Xe = np.tile(sig, (N, 1))
    Xm = np.ones((N, B)); hit = rs.rand(N) < 0.3; Xm[hit, rs.randint(0, B, hit.sum())] = 0
    z = rs.uniform(0, 6, M); ze = rs.uniform(0.01, 0.2, M)
    bf = BruteForce(Y, Ye, Ym)
    p, (lm, le) = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d,
                                 lprob_kwargs=kw, return_gof=True, verbose=False, save_fits=True)
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze,
                                             label_dict=od, **kw)
    rf = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, **kw)
    np.testing.assert_array_equal(bf.fit_Ndim, rf['Ndim'])
    close(bf.fit_chi2, rf['chi2'], rtol=TIGHT, atol=1e-9)
    defined = np.ones_like(rf['lnlike'], dtype=bool)
    if kw.get('free_scale') and kw.get('dim_prior', True):
        # one usable band + free scale: nan or -inf by rounding luck in the reference
        defined = rf['Ndim'] != 1
        assert not np.isfinite(bf.fit_lnlike[~defined]).any()
        assert not np.isfinite(rf['lnlike'][~defined]).any()
    close(bf.fit_lnlike[defined], rf['lnlike'][defined], rtol=TIGHT, atol=1e-9)
    # objects whose row holds a nan on either side have an all-nan PDF on that side
    rows = ~(np.isnan(bf.fit_lnlike).any(axis=1) | np.isnan(rf['lnlike']).any(axis=1))
    assert rows.sum() >= 1 and np.isnan(rp[np.isnan(rf['lnlike']).any(axis=1)]).all()
    assert np.isnan(p[np.isnan(bf.fit_lnlike).any(axis=1)]).all()
    close(p[rows], rp[rows], rtol=1e-8, atol=1e-13); close(lm[rows], rlm[rows]); close(le[rows], rle[rows], **EVID)


@pytest.mark.parametrize('kw', [{}, {'dim_prior': False}, {'ignore_model_err': True},
                                {'free_scale': True, 'ignore_model_err': True}])
def test_wild_values_take_the_ieee_variant(kw):
    """zero / huge / infinite variances and fluxes switch the kernels to IEEE division and
    the fully special-cased log; results must still follow NumPy's inf/nan arithmetic."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(909)
    M, N, B = 300, 25, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.1 * Y; Ym = np.ones((M, B))
    Ye[3, 1] = np.inf          # infinite model error: that band contributes 0 (or nan in the log-variance sum)
    Ye[4, :] = 0.0             # exact model
    Ye[5, 2] = 1e200           # variance overflows to inf
    Y[6, 0] = 1e160            # chi2 overflows
    Ym[7, 3] = 0
    X = Y[rs.choice(np.arange(10, M), N)] + 0.3 * rs.randn(N, B)
    Xe = np.full((N, B), 0.3); Xm = np.ones((N, B))
    Xe[2, 1] = 1e-170          # variance underflows towards 0
    X[3, 4] = 1e40
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    bf = BruteForce(Y, Ye, Ym)
    with np.errstate(all='ignore'):
        p, (lm, le) = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                     return_gof=True, verbose=False, save_fits=True)
        rf = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, **kw)
        rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze,
                                                 label_dict=od, **kw)
    close(bf.fit_chi2, rf['chi2'], rtol=1e-9, atol=1e-9)
    close(bf.fit_lnlike, rf['lnlike'], rtol=1e-9, atol=1e-9)
    close(lm, rlm, rtol=1e-9); close(le, rle, **EVID64)          # the IEEE variant is all fp64
    close(p, rp, rtol=1e-8, atol=1e-13)


def test_two_pass_fallback_matches_single_pass():
    """with no room for the candidate lists the library takes the two-pass kernels
    (k_stats + k_kde); both routes must give the same PDFs."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(11)
    M, N, B = 5000, 300, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.1 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + 0.5 * rs.randn(N, B); Xe = np.full((N, B), 0.5); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = rs.uniform(0.01, 0.1, M)          # many sigma classes: window-scatter path
    eng = get_engine()
    out = {}
    for name, lim in (('single', 32 << 30), ('two', 1 << 20)):
        eng.set_workspace_limit(lim)
        try:
            out[name] = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d,
                                                          return_gof=True, save_fits=False, verbose=False)
        finally:
            eng.set_workspace_limit(32 << 30)
    (p1, (lm1, le1)), (p2, (lm2, le2)) = out['single'], out['two']
    close(lm1, lm2, rtol=1e-13, atol=0); close(le1, le2, **EVID)
    close(p1, p2, rtol=1e-10, atol=1e-16)
    rp, rlm, rle = fo.bruteforce_fit_predict(X[:40].copy(), Xe[:40].copy(), Xm[:40].copy(), Y, Ye, Ym, z, ze,
                                             label_dict=od)
    close(p2[:40], rp, rtol=1e-8, atol=1e-14)


def test_cdf_rule_dropping_half_of_a_hundred_thousand_kernels_is_a_selection_not_a_loop():
    """a broad posterior with a large cdf_thresh: K ~ n / 2 exclusions over 1e5 kernels -- the arg-max rounds alone would be
    K n / 64 = 8e7 steps for this ONE row (minutes); the radix selection on the weights' bit patterns takes eight passes"""
    import time
    from frankenz_amd import pdf as hp
    d, od = dicts()
    rs = np.random.RandomState(78)
    n = 100000
    y, ys = rs.uniform(0.5, 6.5, n), rs.uniform(0.02, 0.3, n)
    wt = rs.permutation(n) + 1.0                                           # distinct
    t0 = time.perf_counter()
    got = hp.gauss_kde_dict(d, y=y, y_std=ys, y_wt=wt, wt_thresh=None, cdf_thresh=0.5)
    assert time.perf_counter() - t0 < 5.0
    close(got, fo.gauss_kde_dict(od, y=y, y_std=ys, y_wt=wt, wt_thresh=None, cdf_thresh=0.5), rtol=1e-9, atol=1e-12)


def test_cdf_rule_with_hundreds_of_exclusions():
    """pdf.py:593-597 has no limit on how many of the largest weights the CDF rule drops: a nearly flat weight row over
    4 000 kernels at cdf_thresh 0.1 / 0.5 drops ~400 / ~2 000 of them (until round 4 the kernel refused more than 64),
    with runs of EQUAL weights straddling the boundary (distinct values only, so that the reference's unstable argsort
    cannot reorder the tie the boundary falls into)."""
    from frankenz_amd import pdf as hp
    d, od = dicts()
    rs = np.random.RandomState(77)
    n = 4000
    y, ys = rs.uniform(0.5, 6.5, n), rs.uniform(0.02, 0.3, n)
    wt = 1. + 1e-3 * rs.permutation(n)                                   # distinct, nearly flat
    for cdf in (0.1, 0.5, 0.9):
        want = fo.gauss_kde_dict(od, y=y, y_std=ys, y_wt=wt, wt_thresh=None, cdf_thresh=cdf)
        close(hp.gauss_kde_dict(d, y=y, y_std=ys, y_wt=wt, wt_thresh=None, cdf_thresh=cdf), want, atol=1e-13)
    grid = np.arange(0, 7 + 1e-5, .01)
    close(hp.gauss_kde(y, ys, grid, y_wt=wt, wt_thresh=None, cdf_thresh=0.3),
          fo.gauss_kde(y, ys, grid, y_wt=wt, wt_thresh=None, cdf_thresh=0.3), atol=1e-13)
    # whole tie groups beyond the boundary: the PDF is independent of which members of a group are taken only when the
    # members are the same kernel, so the tied weights share one (y, y_std)
    wt2 = np.repeat(np.arange(1., 41.), 100); y2 = np.repeat(rs.uniform(1, 6, 40), 100); ys2 = np.repeat(rs.uniform(.05, .2, 40), 100)
    close(hp.gauss_kde_dict(d, y=y2, y_std=ys2, y_wt=wt2, wt_thresh=None, cdf_thresh=0.37),
          fo.gauss_kde_dict(od, y=y2, y_std=ys2, y_wt=wt2, wt_thresh=None, cdf_thresh=0.37), rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize('kw', [{}, {'free_scale': True, 'ignore_model_err': True},
                                {'free_scale': True, 'ignore_model_err': False}])
def test_cdf_threshold_rule_through_the_classes(kw):
    """kde_kwargs={'wt_thresh': None}: BruteForce fused / predict routes and the k-NN variant."""
    from frankenz_amd import BruteForce, NearestNeighbors
    d, od = dicts()
    rs = np.random.RandomState(21)
    M, N, B = 900, 30, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 5; Ye = 0.05 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = rs.uniform(0.02, 0.08, M)
    kk = {'wt_thresh': None, 'cdf_thresh': 0.01}
    bf = BruteForce(Y, Ye, Ym)
    p, (lm, le) = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw, kde_kwargs=kk,
                                 return_gof=True, verbose=False, save_fits=True)
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od,
                                             kde_kwargs=kk, **kw)
    tol = dict(rtol=1e-7, atol=1e-13)
    close(p, rp, **tol); close(lm, rlm, rtol=1e-9); close(le, rle, **EVID64)      # materialised rows: all fp64
    close(bf.predict(z, ze, label_dict=d, kde_kwargs=kk, verbose=False), rp, **tol)
    if kw.get('free_scale') and not kw.get('ignore_model_err'):
        return
    nn = NearestNeighbors(Y, Ye, Ym, K=4, feature_map='identity', rstate=np.random.RandomState(5), verbose=False)
    p, (lm, le) = nn.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, rstate=np.random.RandomState(6), k=8,
                                 label_dict=d, lprob_kwargs=kw, kde_kwargs=kk, return_gof=True, verbose=False)
    feats = fo.knn_train(Y, Ye, 4, 'identity', np.random.RandomState(5))
    q = fo.knn_query_features(X, Xe, 'identity', np.random.RandomState(6))
    tab = fo.knn_neighbors_exact(feats, q, 8)
    rp = fo.knn_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, tab, z, ze, label_dict=od, kde_kwargs=kk, **kw)[0]
    close(p, rp, **tol)
    close(nn.predict(z, ze, label_dict=d, kde_kwargs=kk, verbose=False), rp, **tol)


@pytest.mark.parametrize('B', [17, 32])
@pytest.mark.parametrize('kw', [{}, {'free_scale': True, 'ignore_model_err': True},
                                {'free_scale': True}, {'dim_prior': False}])
def test_wide_band_sets_unmasked(B, kw):
    """17-32 bands (the reference's COSMOS filter list holds 32) run the 32-band
    instantiation: fused fit_predict, the planes of fit() and the mode C loop, unmasked."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(400 + B)
    M, N = 900, 21
    sig = rs.uniform(0.3, 2.0, B)
    Y = rs.lognormal(1., 1., size=(M, 1)) * rs.lognormal(0., .5, size=(M, B)); Ye = 0.04 * Y
    Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .3, N)[:, None] + sig * rs.randn(N, B)
    Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = rs.uniform(0.01, 0.2, M)
    bf = BruteForce(Y, Ye, Ym)
    p, (lm, le) = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d,
                                 lprob_kwargs=kw, return_gof=True, verbose=False, save_fits=False)
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze,
                                             label_dict=od, **kw)
    # 17-32 bands with per-model errors (no room in the register file), without the dimensionality prior, or mode C: the all-fp64
    # ln-space bodies; with the free scale: the one-pass kernel (fp32 remainder in the evidence)
    modeB = kw.get('free_scale') and kw.get('ignore_model_err')
    close(p, rp, rtol=1e-7, atol=1e-13); close(lm, rlm, rtol=1e-9); close(le, rle, **(EVID if modeB else EVID64))
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_kwargs=kw, verbose=False)
    rf = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, **kw)
    close(bf.fit_lnprob, rf['lnlike'], rtol=1e-8, atol=1e-8)
    close(bf.fit_chi2, rf['chi2'], rtol=1e-8, atol=1e-8)
    np.testing.assert_array_equal(bf.fit_Ndim, rf['Ndim'])


def test_more_than_32_bands_is_refused():
    from frankenz_amd import BruteForce
    Y = np.ones((10, 33))
    with pytest.raises(Exception, match='bands unsupported'):
        BruteForce(Y, 0.1 * Y, np.ones_like(Y)).fit(Y[:2].copy(), Y[:2].copy(), np.ones((2, 33)), verbose=False)


@pytest.mark.parametrize('N,M', [(1, 1), (3, 2), (5, 63), (2, 64), (4, 256), (3, 257), (0, 10)])
def test_tiny_and_boundary_shapes(N, M):
    """one object / one model, model counts around the wave (64) and tile (256) sizes, and an
    empty object set -- fused, planes and predict routes."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(1000 + 7 * N + M)
    B = 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.05 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + 0.3 * rs.randn(N, B) if N else np.zeros((0, B))
    Xe = np.full((N, B), 0.3); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    for kw in ({}, {'free_scale': True, 'ignore_model_err': True}, {'free_scale': True}):
        bf = BruteForce(Y, Ye, Ym)
        p, (lm, le) = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                     return_gof=True, verbose=False, save_fits=False)
        assert p.shape == (N, d.Ngrid) and lm.shape == (N,) and le.shape == (N,)
        if N == 0:
            continue
        rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
        ok = np.isfinite(rle)                 # M == 1 with the free scale: chi2 == 0 exactly -> -inf / nan rows
        close(p[ok], rp[ok], rtol=1e-8, atol=1e-14); close(lm[ok], rlm[ok]); close(le[ok], rle[ok], **EVID)
        assert np.isnan(p[~ok]).all() == np.isnan(rp[~ok]).all()
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_kwargs=kw, verbose=False)
        rf = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, **kw)
        fin = np.isfinite(rf['lnlike'])
        close(bf.fit_lnlike[fin], rf['lnlike'][fin], rtol=1e-8, atol=1e-8)
        close(bf.predict(z, ze, label_dict=d, verbose=False)[ok], rp[ok], rtol=1e-8, atol=1e-14)


@pytest.mark.parametrize('kw', [{}, {'dim_prior': False}])
@pytest.mark.parametrize('errs', ['band_constants', 'zeros', 'one_band_inf'])
def test_band_constant_model_errors_take_the_hoisted_path(kw, errs, monkeypatch):
    """model errors that are the same for every model (per band) are folded into the object's
    variances and mode A runs on the mode Ai kernels: same results as the general kernels
    (FZ_NO_ERRCONST=1) and as the oracle; masks and the unmasked log-variance sum included."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(88)
    M, N, B = 900, 70, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3
    Ye = np.tile({'band_constants': np.array([0.3, 0.1, 0.25, 0.6, 1.1]), 'zeros': np.zeros(B),
                  'one_band_inf': np.array([0.3, np.inf, 0.25, 0.6, 1.1])}[errs], (M, 1))
    Ym = np.ones((M, B)); Ym[rs.rand(M, B) < 0.05] = 0
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    Xm[rs.rand(N, B) < 0.1] = 0; X[3, 2] = np.nan
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)

    def run():
        bf = BruteForce(Y, Ye, Ym)
        p, (lm, le) = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw, return_gof=True,
                                     verbose=False, save_fits=True)
        return p, lm, le, bf.fit_lnlike, bf.fit_chi2, bf.fit_Ndim
    a = run()
    monkeypatch.setenv('FZ_NO_ERRCONST', '1')
    b = run()
    monkeypatch.delenv('FZ_NO_ERRCONST')
    for u, v in zip(a, b):
        np.testing.assert_allclose(u, v, rtol=1e-9, atol=1e-12, equal_nan=True)
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    rf = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, **kw)
    close(a[0], rp, rtol=1e-8, atol=1e-13); close(a[1], rlm); close(a[2], rle)
    close(a[3], rf['lnlike'], rtol=1e-9, atol=1e-9); close(a[4], rf['chi2'], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(a[5], rf['Ndim'])


@pytest.mark.parametrize('env', [{'FZ_HIST': '0', 'FZ_FUSED_CFG': '4,8'}, {'FZ_HIST': '0', 'FZ_FUSED_CFG': '2,8'}, {'FZ_HIST': '0', 'FZ_FUSED_CFG': '2,16'},
                                 {'FZ_HIST': '0', 'FZ_FUSED_CFG': '1,4'}, {'FZ_HIST': '0', 'FZ_NO_WSPACE': '1'}, {'FZ_CHUNK': '5000'},
                                 {'FZ_HIST': '0', 'FZ_NO_WSPACE': '1', 'FZ_FUSED_CFG': '2,16'}, {'FZ_HIST': '0'},
                                 {'FZ_HIST': '0', 'FZ_FUSED_CFG': '2,12'}, {'FZ_NOLIST': '1'}, {'FZ_EXACT_EVIDENCE': '1'},
                                 {'FZ_HIST_AMBCAP': '3'}, {'FZ_HIST_AMBCAP': '3', 'FZ_NOLIST': '1'}])      # ambiguous lists of 3 entries: (nearly) every object overflows and is re-run by the exact sweep
def test_tuning_switches_do_not_change_results(env, monkeypatch):
    """every launch geometry / kernel body / chunking reachable through the diagnostic
    environment switches gives the same PDFs (summation order aside)."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(123)
    M, N, B = 777, 16500, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = Y * rs.uniform(0.02, 0.08, size=(M, B)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    out = {}
    for kw in ({}, {'free_scale': True, 'ignore_model_err': True}):
        run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                        return_gof=True, save_fits=False, verbose=False)
        p0, (lm0, le0) = run()
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        p1, (lm1, le1) = run()
        for k in env:
            monkeypatch.delenv(k)
        close(p1, p0, rtol=1e-9, atol=1e-15); close(lm1, lm0, rtol=1e-12); close(le1, le0, **EVID)
    rp, rlm, rle = fo.bruteforce_fit_predict(X[:30].copy(), Xe[:30].copy(), Xm[:30].copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    close(p1[:30], rp, rtol=1e-8, atol=1e-14)


def test_fused_cfg_that_is_not_instantiated_is_refused(monkeypatch):
    """FZ_FUSED_CFG names a geometry that was not compiled: the call is refused with that text as a Python exception, and the
    next call on the same engine runs as if nothing had happened (same shape as test_tuning_switches_do_not_change_results)."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(123)
    M, N, B = 777, 16500, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = Y * rs.uniform(0.02, 0.08, size=(M, B)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, return_gof=True,
                                                    save_fits=False, verbose=False)
    p0, (lm0, le0) = run()
    monkeypatch.setenv('FZ_HIST', '0')
    monkeypatch.setenv('FZ_FUSED_CFG', '3,3')
    with pytest.raises(RuntimeError, match=r'FZ_FUSED_CFG=3,3 is not an instantiated configuration'):
        run()
    monkeypatch.delenv('FZ_FUSED_CFG')
    p1, (lm1, le1) = run()                                       # k_fused at its own geometry
    monkeypatch.delenv('FZ_HIST')
    p2, (lm2, le2) = run()                                       # the default form again
    close(p1, p0, rtol=1e-9, atol=1e-15); close(lm1, lm0, rtol=1e-12); close(le1, le0, **EVID)
    close(p2, p0, rtol=1e-9, atol=1e-15); close(lm2, lm0, rtol=1e-12); close(le2, le0, rtol=1e-12)


@pytest.mark.parametrize('kw', [{}, {'ignore_model_err': True}, {'free_scale': True, 'ignore_model_err': True}])
@pytest.mark.parametrize('err', ['const', 'varying'])
def test_default_fused_evidence_is_the_fp64_logsumexp(kw, err):
    """The DEFAULT fused path (k_hist) forms and sums every weight in fp64 -- the fp32 quantity only classifies which pairs can
    matter at all (below 2^-(55 + log2 M) of the best: dropped) -- so its ln-evidence is the reference's fp64 logsumexp
    (bruteforce.py:619) to rounding: 1e-12 here, against the oracle, on data whose sub-threshold pairs carry a large share of the
    evidence (broad noise) and on narrow likelihoods; ln-max and PDFs likewise."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    for noise in (1.0, 4.0):
        rs = np.random.RandomState(int(77 + 10 * noise))
        M, N, B = 9000, 120, 5
        sig = SDSS5 * noise
        Y = rs.lognormal(1., 1., size=(M, B)); Ym = np.ones((M, B))
        Ye = np.tile(sig, (M, 1)) if err == 'const' else sig * rs.uniform(0.5, 1.5, size=(M, B))
        X = Y[rs.choice(M, N)] + sig * rs.randn(N, B); Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, B))
        z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
        p, (lm, le) = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                        return_gof=True, save_fits=False, verbose=False)
        assert get_engine().last_form().startswith('k_hist<')
        rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
        close(le, rle, rtol=1e-12, atol=1e-12)
        close(lm, rlm, rtol=1e-12, atol=1e-12)
        close(p, rp, rtol=1e-9, atol=1e-14)


@pytest.mark.parametrize('kw', [{}, {'ignore_model_err': True}, {'free_scale': True, 'ignore_model_err': True}])
def test_exact_evidence_switch(kw, monkeypatch):
    """The default weight-space body sums the sub-threshold weights in fp32 (EVID); FZ_NO_WSPACE=1
    selects the all-fp64 ln-space body, whose ln-evidence is held to 1e-9 here, and the two bodies
    give the same ln-max and PDFs.  Objects include exact self matches, a bright object (S/N 1e5)
    and one whose only good model comes last (the reference jumps by thousands in one step)."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(909)
    M, N, B = 2100, 260, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = np.tile(0.5 * SDSS5, (M, 1)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    X[:8] = Y[:8]                                           # chi2 == 0 against their own model
    Y[-1] = 1e5 * SDSS5; X[8] = Y[-1] + SDSS5 * rs.randn(B)  # bright: every other model is off by chi2 ~ 1e10, the match is the last model
    X[9] = Y[M // 2 + 7] + 1e-3 * SDSS5                     # a near-exact match (chi2 ~ 5e-6, far below the mode)
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                    return_gof=True, save_fits=False, verbose=False)
    p0, (lm0, le0) = run()
    monkeypatch.setenv('FZ_NO_WSPACE', '1')
    p1, (lm1, le1) = run()
    monkeypatch.delenv('FZ_NO_WSPACE')
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    close(le1, rle, rtol=1e-9, atol=1e-10); close(lm1, rlm, rtol=1e-9); close(p1, rp, rtol=1e-8, atol=1e-14)
    close(le0, rle, **EVID); close(lm0, rlm, rtol=1e-9); close(p0, rp, rtol=1e-8, atol=1e-14)
    close(p0, p1, rtol=1e-9, atol=1e-15); close(lm0, lm1, rtol=1e-12)


@pytest.mark.parametrize('kw', [{}, {'free_scale': True, 'ignore_model_err': True}, {'dim_prior': False}])
def test_masked_and_unmasked_objects_split_across_kernels(kw, monkeypatch):
    """a chunk that mixes fully observed objects with objects missing bands is run as two
    launches (mask-free kernels + masked kernels): same results as the single masked launch
    (FZ_NO_SPLIT=1) and as the oracle, for objects of both kinds."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(321)
    M, N, B = 650, 9000, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = Y * rs.uniform(0.02, 0.08, size=(M, B)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    Xm[rs.rand(N, B) < 0.04] = 0
    X[17, 1] = np.nan                              # cleaned in place -> becomes a masked object
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                    return_gof=True, save_fits=False, verbose=False)
    p0, (lm0, le0) = run()
    monkeypatch.setenv('FZ_NO_SPLIT', '1')
    p1, (lm1, le1) = run()
    monkeypatch.delenv('FZ_NO_SPLIT')
    close(p0, p1, rtol=1e-9, atol=1e-15); close(lm0, lm1, rtol=1e-12); close(le0, le1, **EVID)
    masked = np.where((Xm == 0).any(axis=1))[0][:25]; full = np.where((Xm == 1).all(axis=1))[0][:25]
    pick = np.concatenate([masked, full, [17]])
    rp, rlm, rle = fo.bruteforce_fit_predict(X[pick].copy(), Xe[pick].copy(), Xm[pick].copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    close(p0[pick], rp, rtol=1e-8, atol=1e-14); close(lm0[pick], rlm); close(le0[pick], rle, **EVID)


def test_split_chunk_falls_back_as_a_whole_when_the_workspace_is_too_small():
    """object subsets exist only for the single-pass kernel: without room for its candidate lists
    the whole mixed chunk takes the two-pass route, masked variant."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(322)
    M, N, B = 500, 6000, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = 0.05 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    Xm[rs.rand(N, B) < 0.05] = 0
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    eng = get_engine()
    out = {}
    for name, lim in (('fused', 32 << 30), ('twopass', 1 << 20)):
        eng.set_workspace_limit(lim)
        try:
            out[name] = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d,
                                                          return_gof=True, save_fits=False, verbose=False)
        finally:
            eng.set_workspace_limit(32 << 30)
    (p1, (lm1, le1)), (p2, (lm2, le2)) = out['fused'], out['twopass']
    close(p1, p2, rtol=1e-9, atol=1e-15); close(lm1, lm2, rtol=1e-12); close(le1, le2, **EVID)
    rp, rlm, rle = fo.bruteforce_fit_predict(X[:40].copy(), Xe[:40].copy(), Xm[:40].copy(), Y, Ye, Ym, z, ze, label_dict=od)
    close(p2[:40], rp, rtol=1e-8, atol=1e-14)


def test_all_zero_model_poisons_free_scale_like_the_reference():
    """a model whose fluxes are all zero has shape == 0: the free-scale solve is 0/0, its ln-like is
    nan, and with it every object's evidence and PDF (bruteforce.py:619-620) -- not silently dropped."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(99)
    M, N, B = 300, 20, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Y[7] = 0.0
    Ye = 0.05 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(np.arange(10, M), N)] + 0.3 * rs.randn(N, B); Xe = np.full((N, B), 0.3); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    for kw in ({'free_scale': True, 'ignore_model_err': True}, {}):
        p, (lm, le) = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                        return_gof=True, save_fits=False, verbose=False)
        rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
        np.testing.assert_array_equal(np.isnan(p), np.isnan(rp)); np.testing.assert_array_equal(np.isnan(le), np.isnan(rle))
        ok = np.isfinite(rle)
        close(p[ok], rp[ok], rtol=1e-8, atol=1e-14); close(le[ok], rle[ok], **EVID)
        if kw:
            assert np.isnan(rle).all() and np.isnan(le).all()


@pytest.mark.parametrize('masked', [False, True])
def test_host_pdf_pipeline_matches_the_serial_copy_out(masked, monkeypatch):
    """calls with host PDFs and >= 3*2^17 objects run as a pipeline (2^18-object chunks, two
    staging buffers, rows of chunk k copied out while chunk k+1 is computed, gof rows copied once
    at the end): the same results as the serial path (FZ_NO_PIPELINE=1) and equal to the oracle on
    rows of the first, a middle and the last (ragged) chunk."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(77)
    M, N, B = 230, (1 << 18) * 2 + 12345, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = Y * rs.uniform(0.02, 0.08, size=(M, B)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    if masked:
        Xm[rs.rand(N, B) < 0.02] = 0.
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d,
                                                    return_gof=True, save_fits=False, verbose=False)
    p1, (lm1, le1) = run()
    monkeypatch.setenv('FZ_NO_PIPELINE', '1')
    p0, (lm0, le0) = run()
    monkeypatch.delenv('FZ_NO_PIPELINE')
    if not masked:      # same launches per object either way (a split chunk's partition differs with the chunking)
        # (the ragged last chunk runs with another launch geometry than the same objects inside one big chunk: the
        # weight-space body's fp32 reference then differs in the last bit, and PDFs / ln-evidence with it at rounding level)
        close(p1, p0, rtol=1e-12, atol=1e-16); np.testing.assert_array_equal(lm1, lm0); close(le1, le0, **EVID)
    else:
        close(p1, p0, rtol=1e-9, atol=1e-15); close(lm1, lm0, rtol=1e-12); close(le1, le0, **EVID)
    for sl in (slice(0, 20), slice((1 << 18) - 10, (1 << 18) + 10), slice(N - 20, N)):
        rp, rlm, rle = fo.bruteforce_fit_predict(X[sl].copy(), Xe[sl].copy(), Xm[sl].copy(), Y, Ye, Ym, z, ze, label_dict=od)
        close(p1[sl], rp, rtol=1e-8, atol=1e-14); close(lm1[sl], rlm); close(le1[sl], rle, **EVID)


@pytest.mark.parametrize('M', [4096, 1501])                 # even: 16-B row loads; odd: rows start on 8-B boundaries
@pytest.mark.parametrize('single_class', [True, False])
def test_predict_from_stored_plane_single_pass(M, single_class, monkeypatch):
    """BruteForce.predict(logwt=...) (bruteforce.py:303-372) reads each stored row once
    (k_plane_fused); same PDFs, lmap, levid as the two-pass kernels (FZ_PLANE_TWOPASS=1) and as
    the oracle, including rows with -inf entries, a nan (first / not first), a +inf and an all -inf row."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(4242 + M)
    N, B = 700, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.05 * Y; Ym = np.ones((M, B))
    z = rs.uniform(0, 6, M)
    ze = np.full(M, 0.05) if single_class else rs.uniform(0.01, 0.1, M)
    # ln-weights shaped like posterior rows: a few dominant entries over a long negligible tail
    lw = -0.5 * rs.chisquare(3, size=(N, M)) * rs.choice([1.0, 30.0, 3000.0], size=(N, 1))
    lw[5, 10:20] = -np.inf
    lw[6, 0] = np.nan                                        # builtin max: nan only if first
    lw[7, 77] = np.nan
    lw[8, 3] = np.inf
    lw[9, :] = -np.inf
    lw[10, :] = lw[10, 0]                                    # all equal: every entry selected
    lw[11, :] += 1e6                                         # huge offsets: the threshold offset is absorbed
    bf = BruteForce(Y, Ye, Ym)
    run = lambda **kk: bf.predict(z, ze, label_dict=d, logwt=lw.copy(), return_gof=True, verbose=False, **kk)
    with np.errstate(all='ignore'):
        p0, (lm0, le0) = run()                                  # default: the sub-threshold weights in fp32 (conftest.EVID)
        p1, (lm1, le1) = run(kde_kwargs={'exact_evidence': True})
        monkeypatch.setenv('FZ_PLANE_TWOPASS', '1')
        p2, (lm2, le2) = run()
        monkeypatch.delenv('FZ_PLANE_TWOPASS')
        rp, rlm, rle = fo.bruteforce_predict(lw, z, ze, label_dict=od)
    close(lm1, lm2, rtol=0, atol=0); close(le1, le2, rtol=1e-13, atol=1e-12)
    close(p1, p2, rtol=1e-10, atol=1e-16)
    close(lm1, rlm, rtol=0, atol=0); close(le1, rle, rtol=1e-12, atol=1e-11)
    close(p1, rp, rtol=1e-8, atol=1e-14)
    close(lm0, lm1, rtol=0, atol=0); close(p0, p1, rtol=1e-10, atol=1e-16)
    big = np.abs(rle) > 1e5                                     # (rows offset by 1e6: a relative tolerance is the meaningful one there)
    close(le0[~big], rle[~big], **EVID); close(le0[big], rle[big], rtol=1e-12, atol=0)
    # wt_thresh = 0 keeps every entry with a non-zero weight; a large threshold keeps only the best
    for wt in (0.0, 0.5):
        with np.errstate(all='ignore'):
            q1 = bf.predict(z, ze, label_dict=d, logwt=lw[:40].copy(), kde_kwargs={'wt_thresh': wt}, verbose=False)
            rq, _, _ = fo.bruteforce_predict(lw[:40], z, ze, label_dict=od, wt_thresh=wt)
        close(q1, rq, rtol=1e-8, atol=1e-14)


@pytest.mark.parametrize('M', [1000, 1001])                 # even: two models per thread, 16-B stores; odd: one, 8-B stores
@pytest.mark.parametrize('kw', [{}, {'free_scale': True, 'ignore_model_err': True}])
def test_fit_planes_store_width_does_not_change_results(M, kw, monkeypatch):
    """BruteForce.fit (bruteforce.py:182-203): the seven planes are bit-identical whether a thread
    owns two adjacent models (16-B non-temporal stores) or one (FZ_PLANES_MPT=1), and match the oracle."""
    from frankenz_amd import BruteForce
    rs = np.random.RandomState(808 + M)
    N, B = 300, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = Y * rs.uniform(0.02, 0.08, size=(M, B)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1)); Xm = np.ones((N, B))
    Xm[rs.rand(N, B) < 0.03] = 0
    def run():
        bf = BruteForce(Y, Ye, Ym)
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_kwargs=kw, track_scale=True, verbose=False)
        return [bf.fit_lnprior, bf.fit_lnlike, bf.fit_lnprob, bf.fit_Ndim, bf.fit_chi2, bf.fit_scale, bf.fit_scale_err]
    with np.errstate(all='ignore'):
        a = run()
        monkeypatch.setenv('FZ_PLANES_MPT', '1')
        b = run()
        monkeypatch.delenv('FZ_PLANES_MPT')
        rf = fo.bruteforce_fit(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, **kw)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    close(a[1], rf['lnlike'], rtol=1e-9, atol=1e-9); close(a[4], rf['chi2'], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(a[3], rf['Ndim'])


@pytest.mark.parametrize('kde', ['dict_many_classes', 'grid'])
def test_window_scatter_by_lane_or_by_wave(kde, monkeypatch):
    """gauss_kde_dict with many kernel widths (pdf.py:599-620) and the direct gauss_kde
    (pdf.py:519-524): a selected model's window is added by its own lane (up to 160 grid points) or
    by the whole wave (FZ_LANE_WINDOW=0); same PDFs either way, and the oracle's."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(515)
    M, N, B = 3000, 400, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.1 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + 0.5 * rs.randn(N, B); Xe = np.full((N, B), 0.5); Xm = np.ones((N, B))
    z = rs.uniform(-0.2, 7.2, M)                                   # some labels at / beyond the grid edges
    ze = rs.uniform(0.01, 0.1, M); ze[::97] = 0.4                  # a few windows wider than 160 points
    z[::131] = np.clip(z[::131], 0.1, 6.9)
    if kde == 'grid':
        lab = dict(label_grid=d.grid); olab = dict(label_grid=od.grid)
        z = np.clip(z, 0.0, 7.0)
    else:
        lab = dict(label_dict=d); olab = dict(label_dict=od)
        z = np.clip(z, 0.0, 7.0)
    run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, return_gof=True,
                                                    save_fits=False, verbose=False, **lab)
    p0, (lm0, le0) = run()
    monkeypatch.setenv('FZ_LANE_WINDOW', '0')
    p1, (lm1, le1) = run()
    monkeypatch.delenv('FZ_LANE_WINDOW')
    close(p0, p1, rtol=1e-10, atol=1e-16); close(lm0, lm1, rtol=0, atol=0); close(le0, le1, rtol=0, atol=0)
    rp, rlm, rle = fo.bruteforce_fit_predict(X[:30].copy(), Xe[:30].copy(), Xm[:30].copy(), Y, Ye, Ym, z, ze, **olab)
    close(p0[:30], rp, rtol=1e-8, atol=1e-14)


def test_grid_kde_labels_above_the_grid_contribute_nothing():
    """pdf.py:499-524: a label whose window lies wholly above the grid gives an empty slice, a zero sum,
    and is skipped -- a valid reference input (model redshifts beyond the top of ``label_grid``), not an
    error; a window that pokes in from above contributes its overlap.  Only windows wholly BELOW the
    grid (negative upper bound: Python slicing wraps) stay refused."""
    from frankenz_amd import pdf as hp
    grid = np.arange(0, 7 + 1e-5, .01)
    rs = np.random.RandomState(31)
    y = np.concatenate([rs.uniform(0.2, 6.8, 40), [7.4, 9.0, 7.04, 25.0]])
    ys = np.concatenate([rs.uniform(0.02, 0.2, 40), [0.05, 0.3, 0.03, 1.0]])
    wt = rs.uniform(0.1, 1.0, len(y))
    for kw in ({}, {'wt_thresh': 0.25}, {'sig_thresh': 3.}):
        close(hp.gauss_kde(y, ys, grid, y_wt=wt, **kw), fo.gauss_kde(y, ys, grid, y_wt=wt, **kw), atol=1e-14)
    with pytest.raises(IndexError):
        hp.gauss_kde(np.array([-3.0, 1.0]), np.array([0.05, 0.05]), grid)


@pytest.mark.parametrize('kw', [{}, {'ignore_model_err': True}, {'free_scale': True, 'ignore_model_err': True}])
@pytest.mark.parametrize('N', [300, 20000])                        # one object per wave (1, 4) / the 12-wave geometry
def test_class_sorted_stack_of_many_kernel_widths(kw, N, monkeypatch):
    """gauss_kde_dict with many kernel widths on the weight-space body: model records ordered by dictionary class,
    one histogram per class present and one convolution per class (pdf_stage_mc) -- same PDFs as the per-model
    window adds (FZ_NO_MC=1) and as the oracle; labels at both grid edges (truncated kernel masses), classes with a
    single model, a class boundary inside a 64-entry block."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(616 + N % 7)
    M, B = 2500, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.1 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + 0.5 * rs.randn(N, B); Xe = np.full((N, B), 0.5); Xm = np.ones((N, B))
    z = np.clip(rs.uniform(-0.3, 7.3, M), 0.0, 7.0)                 # piles at both edges of the grid
    ze = rs.uniform(0.01, 0.12, M)                                 # ~28 classes, half-widths 5..60
    ze[7] = 0.125; ze[8] = 0.006                                   # classes of one model (widest: 63; narrowest)
    run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                    return_gof=True, save_fits=False, verbose=False)
    p0, (lm0, le0) = run()
    monkeypatch.setenv('FZ_NO_MC', '1')
    p1, (lm1, le1) = run()
    monkeypatch.delenv('FZ_NO_MC')
    assert np.isfinite(p0).all()
    close(p0, p1, rtol=1e-9, atol=1e-15); close(lm0, lm1, rtol=1e-14, atol=0); close(le0, le1, **EVID)
    np.testing.assert_allclose(p0.sum(axis=1), 1.0, rtol=1e-12)
    rp, rlm, rle = fo.bruteforce_fit_predict(X[:25].copy(), Xe[:25].copy(), Xm[:25].copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    close(p0[:25], rp, rtol=1e-8, atol=1e-14); close(lm0[:25], rlm); close(le0[:25], rle, **EVID)


@pytest.mark.parametrize('kw', [{}, {'ignore_model_err': True}, {'free_scale': True, 'ignore_model_err': True}])
@pytest.mark.parametrize('force', [None, '1'])
def test_list_free_form_for_broad_likelihoods(kw, force, monkeypatch):
    """faint objects (most models within wt_thresh of the best): the launcher measures the share of pairs within the
    threshold on a sample and runs the form of k_hist that weighs every pair directly instead of classifying it first -- same
    PDFs / lmap / evidence as the classifier form (FZ_NOLIST=0) and as the oracle; forced (FZ_NOLIST=1) on bright objects too, where a handful
    of models carry the whole posterior, a training-set self match (chi2 == 0) sits among the models and one object
    matches nothing (every chi2 far above the mode)."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(717)
    M, N, B = 1500, 17000, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = Y * rs.uniform(0.02, 0.08, size=(M, B)); Ym = np.ones((M, B))
    noise = 6.0 * SDSS5 if force is None else 0.3 * SDSS5
    X = Y[rs.choice(M, N)] + noise * rs.randn(N, B); Xe = np.tile(noise, (N, 1)); Xm = np.ones((N, B))
    X[5] = Y[11]                                                   # exact self match
    X[6] = 1e4                                                     # matches nothing
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    run = lambda: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                    return_gof=True, save_fits=False, verbose=False)
    if force:
        monkeypatch.setenv('FZ_NOLIST', force)
    p1, (lm1, le1) = run()
    monkeypatch.setenv('FZ_NOLIST', '0')
    p0, (lm0, le0) = run()
    monkeypatch.delenv('FZ_NOLIST')
    close(p1, p0, rtol=1e-9, atol=1e-15); close(lm1, lm0, rtol=1e-12); close(le1, le0, **EVID)
    rp, rlm, rle = fo.bruteforce_fit_predict(X[:25].copy(), Xe[:25].copy(), Xm[:25].copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    close(p1[:25], rp, rtol=1e-8, atol=1e-14); close(lm1[:25], rlm); close(le1[:25], rle, **EVID)


@pytest.mark.parametrize('case', ['plain', 'free_scale', 'per_model_err', 'masked', 'prior', 'chunked', 'broad'])
def test_exact_evidence_option_is_fp64_everywhere(case, monkeypatch):
    """``lprob_kwargs={'exact_evidence': True}`` (fz_like_opts.exact_evidence) / ``kde_kwargs={'exact_evidence': True}``
    (predict): every weight of the ln-evidence formed and summed in fp64, on every route -- k_hist<exact>, the masked
    and ln-prior bodies, chunked and unchunked launches (which must then agree to rounding), predict from the stored
    plane -- held to 1e-9 against the oracle (the default bodies: conftest.EVID)."""
    from frankenz_amd import BruteForce
    from frankenz_amd.pdf import logprob_prior
    d, od = dicts()
    rs = np.random.RandomState(4242)
    M, N, B = 2600, 17000 if case == 'chunked' else 400, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = np.tile(0.5 * SDSS5, (M, 1)); Ym = np.ones((M, B))
    noise = SDSS5 * (6.0 if case == 'broad' else 1.0)
    X = Y[rs.choice(M, N)] + noise * rs.randn(N, B); Xe = np.tile(noise, (N, 1)); Xm = np.ones((N, B))
    X[:4] = Y[:4]                                            # self matches
    kw = {}
    if case == 'free_scale':
        kw = {'free_scale': True, 'ignore_model_err': True}
    if case == 'per_model_err':
        Ye = Ye * rs.uniform(0.5, 1.5, size=Ye.shape)
    if case == 'masked':
        Xm[rs.rand(N, B) < 0.1] = 0
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    kwx = dict(kw, exact_evidence=True)
    extra = {}
    if case == 'prior':
        tab = np.log(rs.dirichlet(np.ones(M), size=3)); rows = rs.randint(0, 3, N)
        extra = dict(lprob_func=logprob_prior(tab, rows))
    run = lambda k: BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=k,
                                                      return_gof=True, save_fits=False, verbose=False, **extra)
    p0, (lm0, le0) = run(kw)
    p1, (lm1, le1) = run(kwx)
    sel = slice(0, 120)
    if case == 'prior':
        lnp = fo.bruteforce_fit(X[sel].copy(), Xe[sel].copy(), Xm[sel].copy(), Y, Ye, Ym)['lnlike'] + tab[rows[sel]]
        from scipy.special import logsumexp
        rle = logsumexp(lnp, axis=1); rlm = lnp.max(axis=1)
    else:
        rp, rlm, rle = fo.bruteforce_fit_predict(X[sel].copy(), Xe[sel].copy(), Xm[sel].copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
        close(p1[sel], rp, rtol=1e-8, atol=1e-14)
    close(le1[sel], rle, **EVID64); close(lm1[sel], rlm, rtol=1e-9)
    close(le0[sel], rle, **EVID)
    close(p0, p1, rtol=1e-9, atol=1e-15); close(lm0, lm1, rtol=1e-12)
    if case == 'chunked':
        monkeypatch.setenv('FZ_CHUNK', '5000')
        p2, (lm2, le2) = run(kwx)
        monkeypatch.delenv('FZ_CHUNK')
        np.testing.assert_array_equal(lm2, lm1)
        close(le2, le1, rtol=1e-13, atol=1e-13); close(p2, p1, rtol=1e-12, atol=1e-16)        # summation order of the atomics aside
    if case in ('plain', 'free_scale'):
        # predict from the stored ln-prob plane: default (fp32 remainder) and exact
        bf = BruteForce(Y, Ye, Ym)
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_kwargs=kw, verbose=False)
        pa, (lma, lea) = bf.predict(z, ze, label_dict=d, return_gof=True, verbose=False)
        pb, (lmb, leb) = bf.predict(z, ze, label_dict=d, kde_kwargs={'exact_evidence': True}, return_gof=True, verbose=False)
        close(leb[sel], rle, **EVID64); close(lea[sel], rle, **EVID)
        np.testing.assert_array_equal(lma, lmb); close(pa, pb, rtol=1e-10, atol=1e-16)
        close(pb[sel], rp, rtol=1e-8, atol=1e-14)


def test_positional_kde_args_reach_the_kde_as_in_the_reference():
    """``kde_args`` (bruteforce.py:207-209, 361-369): the grid KDE takes its first positional as ``dx``; the dictionary KDE
    ignores up to two (they land on ``y`` / ``y_std`` next to the given indices)."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(31)
    M, N, B = 400, 12, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.1 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + 0.3 * rs.randn(N, B); Xe = np.full((N, B), 0.3); Xm = np.ones((N, B))
    z = rs.uniform(0.5, 5.5, M); ze = rs.uniform(0.02, 0.1, M)
    grid = np.arange(0, 7 + 1e-5, .01)
    bf = BruteForce(Y, Ye, Ym)
    a = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_grid=grid, kde_args=(0.02,), save_fits=False, verbose=False)
    b = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_grid=grid, kde_kwargs={'dx': 0.02}, save_fits=False, verbose=False)
    np.testing.assert_array_equal(a, b)
    c = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, kde_args=(None, None), save_fits=False, verbose=False)
    e = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, save_fits=False, verbose=False)
    np.testing.assert_array_equal(c, e)
    with pytest.raises(TypeError):
        bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_grid=grid, kde_args=(0.02, None), save_fits=False, verbose=False)


def test_uploads_are_remembered_by_content_and_in_place_edits_are_seen():
    """The engine skips uploads of what the device already holds, keyed on a content hash -- the reference keeps REFERENCES to
    the caller's model arrays (bruteforce.py:54-56), so an in-place edit between two calls must change the answer."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(77)
    M, N, B = 900, 40, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.1 * Y; Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + 0.3 * rs.randn(N, B); Xe = np.full((N, B), 0.3); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    bf = BruteForce(Y, Ye, Ym)
    run = lambda: bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, return_gof=True, save_fits=False, verbose=False)
    p0, (lm0, le0) = run()
    eng = get_engine()
    k_models, k_labels = eng._models_key, eng._labels_key
    p1, (lm1, le1) = run()
    assert eng._models_key == k_models and eng._labels_key == k_labels            # nothing changed: nothing re-sent
    np.testing.assert_array_equal(lm1, lm0)
    Y[::7] *= 1.5                                                               # in place: same array object, new content
    z[::5] = 6.0 - z[::5]
    p2, (lm2, le2) = run()
    assert eng._models_key != k_models and eng._labels_key != k_labels
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od)
    close(p2, rp, rtol=1e-8, atol=1e-14); close(lm2, rlm, rtol=1e-10); close(le2, rle, **EVID)
    assert np.abs(p2 - p0).max() > 1e-3


@pytest.mark.parametrize('B', [9, 12, 16, 20, 32])
@pytest.mark.parametrize('kw', [{}, {'free_scale': True, 'ignore_model_err': True}, {'ignore_model_err': True}])
@pytest.mark.parametrize('err', ['const', 'varying'])
def test_wide_band_sets_on_the_one_pass_kernel(B, kw, err, monkeypatch):
    """9-32 real bands without masks (the reference's COSMOS list holds 32 filters): the one-pass histogram kernel in its mask-free
    form on the 16- / 32-band instantiations (pad bands are zeros; the power of chi2 is that of the real band count), one object
    per wave and eight waves per block -- against the oracle, default and all-fp64 evidence."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(900 + B)
    M, N = 2600, 150
    sig = rs.uniform(0.3, 2.0, B)
    Y = rs.lognormal(1., 1., size=(M, 1)) * rs.lognormal(0., .5, size=(M, B))
    Ye = np.tile(0.3 * sig, (M, 1)) if err == 'const' else 0.04 * Y
    Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .1, N)[:, None] + sig * rs.randn(N, B)
    Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    bf = BruteForce(Y, Ye, Ym)
    general32 = (B > 16 and err == 'varying' and not kw)           # 17-32 bands with per-model errors: no room in the register file, masked kernels
    for exact in (False, True):
        # both forms of k_hist are fp64 throughout: the classifier form (default) and the one that weighs every pair directly
        # (FZ_EXACT_EVIDENCE=1; what the free scale and broad likelihoods run anyway)
        with monkeypatch.context() as mp:
            if exact:
                mp.setenv('FZ_EXACT_EVIDENCE', '1')
            p, (lm, le) = bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw, return_gof=True,
                                         verbose=False, save_fits=False)
        form = get_engine().last_form()
        assert form == ('k_fused' if general32 else ('k_hist<exact>' if (exact or kw.get('free_scale')) else 'k_hist<screen>')), form
        close(p, rp, rtol=1e-7, atol=1e-13); close(lm, rlm, rtol=1e-9)
        close(le, rle, **EVID64)


@pytest.mark.parametrize('M', [4100, 5120, 10000, 10240, 17000, 20480])
def test_predict_rows_in_registers_with_ties_at_the_threshold(M, monkeypatch):
    """predict() from a stored plane whose rows fit one block's registers (k_plane_rows: exact maximum first, then fp64 weights
    straight into the LDS histogram; shapes of 5 120, 10 240 and 20 480 entries, used when a row fills 80 % of one).  Entries at ln(wt_thresh) below the best -- the
    threshold to within rounding, by the hundred and by the thousand -- are decided by the reference's own expression
    (pdf.py:591: wt > wt_thresh * max(wt), strict); same answers as k_plane_fused and the oracle; every output fp64."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(77 + M)
    N, B = 90, 5
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.05 * Y; Ym = np.ones((M, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    lw = -0.5 * rs.chisquare(3, size=(N, M)) * rs.choice([1.0, 30.0, 3000.0], size=(N, 1))
    lt = np.log(1e-3)
    for i, n_tie in ((3, 1), (4, 300), (5, 3000)):                  # ties: a few, hundreds, more than the block parks
        best = lw[i].max()
        where = rs.choice(M, n_tie, replace=False)
        where = where[lw[i, where] < best]
        # within 1e-12 of the threshold: far inside the kernel's 1e-9 band (so the parked path decides them), far enough outside
        # the rounding of any exp for the reference's expression to decide them the same way on every implementation
        lw[i, where] = best + lt + rs.choice([1e-13, -1e-13, 1e-12, -1e-12, 3e-11, -3e-11], len(where)) * max(1.0, abs(best))
    lw[6, 0] = np.nan; lw[7, 99] = np.nan; lw[8, 5] = np.inf; lw[9, :] = -np.inf; lw[10, :] = -3.25
    bf = BruteForce(Y, Ye, Ym)
    with np.errstate(all='ignore'):
        p1, (lm1, le1) = bf.predict(z, ze, label_dict=d, logwt=lw.copy(), return_gof=True, verbose=False)
        assert get_engine().last_form() == 'k_plane_rows'
        monkeypatch.setenv('FZ_PLANE_ROWS', '0')
        p2, (lm2, le2) = bf.predict(z, ze, label_dict=d, logwt=lw.copy(), return_gof=True, verbose=False,
                                    kde_kwargs={'exact_evidence': True})
        assert get_engine().last_form() == 'k_plane_fused'
        monkeypatch.delenv('FZ_PLANE_ROWS')
        rp, rlm, rle = fo.bruteforce_predict(lw, z, ze, label_dict=od)
    close(lm1, rlm, rtol=0, atol=0); close(le1, rle, rtol=1e-13, atol=1e-12)
    close(p1, rp, rtol=1e-9, atol=1e-15); close(p1, p2, rtol=1e-9, atol=1e-15)
    close(lm1, lm2, rtol=0, atol=0); close(le1, le2, rtol=1e-13, atol=1e-12)


def test_wide_and_grid_switches_do_not_change_results(monkeypatch):
    """FZ_HIST_WIDE=0 (12 bands back on the masked kernels) and FZ_GRID_RECUR=0 (a table exponential per window point of the
    direct gauss_kde instead of the recurrence on the evenly spaced grid): same PDFs; an uneven grid keeps the per-point form."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(321)
    M, N, B = 1500, 300, 12
    sig = rs.uniform(0.3, 2.0, B)
    Y = rs.lognormal(1., 1., size=(M, 1)) * rs.lognormal(0., .5, size=(M, B)); Ye = np.tile(0.3 * sig, (M, 1)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .1, N)[:, None] + sig * rs.randn(N, B); Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = rs.uniform(0.02, 0.3, M)
    bf = BruteForce(Y, Ye, Ym)
    run = lambda **kw: bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, np.full(M, 0.05), return_gof=True, save_fits=False, verbose=False, **kw)
    p0, (lm0, le0) = run(label_dict=d)
    assert get_engine().last_form() == 'k_hist<screen>'
    monkeypatch.setenv('FZ_HIST_WIDE', '0')
    p1, (lm1, le1) = run(label_dict=d)
    assert get_engine().last_form() == 'k_fused'
    monkeypatch.delenv('FZ_HIST_WIDE')
    close(p1, p0, rtol=1e-9, atol=1e-15); close(lm1, lm0, rtol=1e-12); close(le1, le0, **EVID)
    grid = np.arange(0., 7. + 1e-5, 0.01)
    rung = lambda g: bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_grid=g, return_gof=True, save_fits=False, verbose=False)
    q0, (qm0, qe0) = rung(grid)
    monkeypatch.setenv('FZ_GRID_RECUR', '0')
    q1, (qm1, qe1) = rung(grid)
    monkeypatch.delenv('FZ_GRID_RECUR')
    close(q1, q0, rtol=1e-10, atol=1e-15); close(qm1, qm0, rtol=1e-13); close(qe1, qe0, rtol=1e-13, atol=1e-12)
    rq, rqm, rqe = fo.bruteforce_fit_predict(X[:40].copy(), Xe[:40].copy(), Xm[:40].copy(), Y, Ye, Ym, z, ze, label_grid=grid)
    close(q0[:40], rq, rtol=1e-8, atol=1e-14)
    bent = grid.copy(); bent[300:] += 3e-4                             # not evenly spaced (3 % of a step): the recurrence is not used
    u0, _ = rung(bent)
    ru, _, _ = fo.bruteforce_fit_predict(X[:40].copy(), Xe[:40].copy(), Xm[:40].copy(), Y, Ye, Ym, z, ze, label_grid=bent)
    close(u0[:40], ru, rtol=1e-8, atol=1e-14)


@pytest.mark.parametrize('kw', [{}, {'ignore_model_err': True}, {'free_scale': True, 'ignore_model_err': True}])
@pytest.mark.parametrize('B', [5, 8, 12])
def test_objects_with_unobserved_bands_on_the_one_pass_kernel(B, kw, monkeypatch):
    """Objects with unobserved bands against unmasked models (every real catalogue), modes A with band-constant errors / Ai / B: the
    one-pass kernel runs its mask-free arithmetic with the power of chi2 taken from each object's observed band count (a masked
    band carries inverse variance 0 and adds exactly nothing); objects left with too few bands for a bounded likelihood (one
    band; two with the free scale) are swept by the masked kernels.  Against the oracle, and against the split launches."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(4000 + B)
    M, N = 2300, 420
    sig = rs.uniform(0.3, 2.0, B)
    Y = rs.lognormal(1., 1., size=(M, 1)) * rs.lognormal(0., .5, size=(M, B)); Ye = np.tile(0.3 * sig, (M, 1)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .1, N)[:, None] + sig * rs.randn(N, B); Xe = np.tile(sig, (N, 1))
    Xm = (rs.uniform(size=(N, B)) > 0.25).astype(float)
    for i, nobs in enumerate(range(B + 1)):                       # 0 ... B observed bands, explicitly
        Xm[i] = 0.0; Xm[i, :nobs] = 1.0
    X[Xm == 0] = 1e6                                              # garbage in the unobserved bands must not matter
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    bf = BruteForce(Y, Ye, Ym)
    run = lambda: bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw, return_gof=True, save_fits=False, verbose=False)
    with np.errstate(all='ignore'):
        p0, (lm0, le0) = run()
        # (the free scale runs the form that weighs every pair directly; both are fp64 throughout)
        assert get_engine().last_form() == ('k_hist<exact> (per-object band counts)' if kw.get('free_scale') else 'k_hist<screen> (per-object band counts)')
        monkeypatch.setenv('FZ_HIST_OBJMASK', '0')
        p1, (lm1, le1) = run()
        assert not get_engine().last_form().endswith('(per-object band counts)')
        monkeypatch.delenv('FZ_HIST_OBJMASK')
        rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    # one observed band with the free scale: zero degrees of freedom, ln-like = (+-inf or a rounding-sized log) - gammaln(0): nan or
    # -inf depending on whether the residual of the perfect fit rounds to exactly 0 (NumPy here: nan; the fma residual: -inf);
    # the PDF row is nan either way
    ok = np.ones(N, bool)
    if kw.get('free_scale'):
        ok[Xm.sum(axis=1) <= 1] = False
        assert np.all(~np.isfinite(lm0[~ok])) and np.all(~np.isfinite(rlm[~ok]))
    close(p0, rp, rtol=1e-7, atol=1e-13); close(lm0[ok], rlm[ok], rtol=1e-9); close(le0[ok], rle[ok], **EVID64)
    close(p0, p1, rtol=1e-7, atol=1e-13); close(lm0, lm1, rtol=1e-9); close(le0, le1, **EVID)


@pytest.mark.parametrize('kw', [{'dim_prior': False, 'ignore_model_err': True}, {'dim_prior': False, 'free_scale': True, 'ignore_model_err': True}])
def test_no_dimensionality_prior_on_the_power_zero_form(kw, monkeypatch):
    """dim_prior=False in modes Ai / B is the one-pass kernel's power-0 form (ln L = -chi2/2 - a constant of the object, pdf.py:94-98):
    same answers as k_fused's ln-space body (FZ_HIST_NODIMPRIOR=0) and the oracle, with and without unobserved bands."""
    from frankenz_amd import BruteForce
    from frankenz_amd.engine import get_engine
    d, od = dicts()
    rs = np.random.RandomState(55)
    M, N, B = 1900, 500, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 3; Ye = np.tile(0.5 * SDSS5, (M, 1)); Ym = np.ones((M, B))
    X = Y[rs.choice(M, N)] + SDSS5 * rs.randn(N, B); Xe = np.tile(SDSS5, (N, 1))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    for Xm in (np.ones((N, B)), (rs.uniform(size=(N, B)) > 0.2).astype(float)):
        bf = BruteForce(Y, Ye, Ym)
        run = lambda: bf.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw, return_gof=True, save_fits=False, verbose=False)
        with np.errstate(all='ignore'):
            p0, (lm0, le0) = run()
            assert get_engine().last_form().startswith('k_hist<exact>' if kw.get('free_scale') else 'k_hist<screen>')
            monkeypatch.setenv('FZ_HIST_NODIMPRIOR', '0'); monkeypatch.setenv('FZ_HIST_OBJMASK', '0')
            p1, (lm1, le1) = run()
            assert not get_engine().last_form().startswith('k_hist')
            monkeypatch.delenv('FZ_HIST_NODIMPRIOR'); monkeypatch.delenv('FZ_HIST_OBJMASK')
            rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
        close(p0, rp, rtol=1e-7, atol=1e-13); close(lm0, rlm, rtol=1e-9); close(le0, rle, **EVID64)
        close(p0, p1, rtol=1e-7, atol=1e-13); close(lm0, lm1, rtol=1e-9); close(le0, le1, **EVID)


@pytest.mark.parametrize('kw', [{}, {'ignore_model_err': True}])
def test_self_match_of_an_object_nothing_else_fits(kw):
    """The one-pass kernel forms chi2 as sum (xs - y s)^2 (two instructions per band: one rounding of x s instead of the exact
    difference), so a training-set SELF MATCH comes out as ~1e-24 instead of the reference's exact 0 -- and chi2 = 0 means weight 0
    under the dimensionality prior (pdf.py:88-93: (k/2 - 1) ln chi2).  Left alone, that pair would be the best fit by far of an
    object whose nearest OTHER model sits at chi2 ~ 300 (weights ~e^-150): the kernel therefore treats chi2 <= 1e-16 as zero.
    Objects copied from models, errors scaled so that the nearest other model is at chi2 = 300 / 30 / 3: PDFs, ln-max and
    ln-evidence against the oracle, which sees the exact zero."""
    from frankenz_amd import BruteForce
    d, od = dicts()
    rs = np.random.RandomState(404)
    M, B = 4000, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * 10; Ye = np.tile(0.01 * SDSS5, (M, 1)); Ym = np.ones((M, B))
    js = rs.choice(M, 12, replace=False)
    X = Y[js].copy()
    Xe = np.empty_like(X)
    for n, j in enumerate(js):
        c = np.sum(((Y[j] - Y) / SDSS5) ** 2, axis=1); c[j] = np.inf
        Xe[n] = SDSS5 * np.sqrt(c.min() / (300., 30., 3.)[n % 3])
    Xm = np.ones_like(X)
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    p, (lm, le) = BruteForce(Y, Ye, Ym).fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, lprob_kwargs=kw,
                                                    return_gof=True, save_fits=False, verbose=False)
    rp, rlm, rle = fo.bruteforce_fit_predict(X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    assert np.isfinite(rlm).all()                        # (the self match is not the reference's maximum: its ln-like is -inf)
    close(lm, rlm, rtol=1e-11); close(le, rle, rtol=1e-11)
    close(p, rp, rtol=1e-8, atol=1e-13)
    # and the stored-plane route (exact-difference chi2) agrees
    bf = BruteForce(Y, Ye, Ym)
    bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_kwargs=kw, verbose=False)
    assert np.all(np.isneginf(bf.fit_lnlike[np.arange(len(js)), js]))
    close(bf.predict(z, ze, label_dict=d, verbose=False), rp, rtol=1e-8, atol=1e-13)
