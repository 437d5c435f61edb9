"""G18: the reference's BPZ prior (priors.py) and its one documented use, ``lprob_bpz`` of demos/2 cells 43 and 69-71, recorded
for tests/test_priors_host.py and tests/test_hip_bpz_prior.py.  Run from the repository root with the reference importable (as
make_golden.py is):

    python tests/golden/make_golden_bpz.py

Models: the 125 z x 8 template grid of g7_config1 (model j = redshift j // 8, template j % 8) with the templates' types; objects:
24 of its objects with a positive reference-band flux, spread over the magnitudes present (some brighter than m = 20, where the
prior is clipped; ``pick`` holds their indices, the model photometry stays in g7_config1).  z = 0 is on the model grid and the BPZ form is 0 there: 8 columns of -inf ln-prior."""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings('ignore')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('FRANKENZ_REFERENCE', '/root/reference'))

import scipy  # noqa: E402
from frankenz import pdf as rpdf, priors as rpriors, simulate  # noqa: E402
from frankenz.fitting import BruteForce  # noqa: E402


def main():
    g7 = np.load(os.path.join(HERE, 'g7_config1.npz'))
    ms = simulate.MockSurvey()
    ms.load_survey('sdss', Npoints=50000)
    ms.set_refmag('r')
    ms.load_templates('cww+')
    ref, ttype = int(ms.ref_filter), np.array(ms.TTYPE, dtype='int')
    zgrid, mphot = g7['zgrid'], g7['mphot']
    nt = len(ttype)
    assert mphot.shape[0] == len(zgrid) * nt
    model_z, model_type = np.repeat(zgrid, nt), np.tile(ttype, len(zgrid))
    merr, mmask = np.zeros_like(mphot), np.ones_like(mphot)

    ok = np.flatnonzero(g7['obs'][:, ref] > 0)
    mags = -2.5 * np.log10(g7['obs'][ok, ref]) + 23.9
    pick = ok[np.argsort(mags)[np.linspace(0, len(ok) - 1, 24).astype(int)]]
    X, Xe = g7['obs'][pick], g7['err'][pick]
    Xm = np.ones_like(X)
    mag = -2.5 * np.log10(X[:, ref]) + 23.9
    assert (mag < 20).any() and (mag > 20).sum() >= 12

    d = rpdf.PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    ze = np.full(len(model_z), 0.03)
    out = dict(X=X, Xe=Xe, Xm=Xm, pick=pick, model_z=model_z, model_type=model_type, mag=mag, ref=np.array(ref),
               scipy_version=np.array(scipy.__version__))

    def make_hook(**likekw):
        def lprob_bpz(x, xe, xm, ys, yes, yms, mzgrid=None, ttypes=None, ref=None):
            lnlike, ndim, chi2 = rpdf.loglike(x, xe, xm, ys, yes, yms, **likekw)[:3]
            m = -2.5 * np.log10(x[ref]) + 23.9
            prior = np.array([rpriors.bpz_pz_tm(mzgrid, t, m) for t in ttypes]).T.flatten()
            lnprior = np.log(prior)
            return lnprior, lnlike, lnlike + lnprior, ndim, chi2
        return lprob_bpz

    for tag, kw in (('A', {}), ('B', {'free_scale': True, 'ignore_model_err': True})):
        args = [zgrid, ttype, ref]
        bf = BruteForce(mphot, merr, mmask)
        bf.fit(X.copy(), Xe.copy(), Xm.copy(), lprob_func=make_hook(**kw), lprob_args=args, verbose=False)
        if tag == 'A':
            out['lnprior'] = bf.fit_lnprior.copy()
        else:
            assert np.array_equal(out['lnprior'], bf.fit_lnprior)           # the prior does not depend on the likelihood mode
        assert np.array_equal(bf.fit_lnprob, bf.fit_lnlike + bf.fit_lnprior)
        assert not np.isnan(bf.fit_lnprob).any() and np.isfinite(bf.fit_lnlike).all()
        # (fit_lnprob is bit for bit lnlike + lnprior, asserted above: the tests form it from the two stored planes, which keeps
        #  the file under the size limit for a committed fixture)
        out[tag + '_lnlike'] = bf.fit_lnlike.copy()
        p, (lm, le) = bf.predict(model_z, ze, label_dict=d, return_gof=True, verbose=False)
        out[tag + '_pred'], out[tag + '_lmap'], out[tag + '_levid'] = p, lm, le
        out[tag + '_pred_like'] = bf.predict(model_z, ze, label_dict=d, logwt=bf.fit_lnlike, verbose=False)
        out[tag + '_fp'] = BruteForce(mphot, merr, mmask).fit_predict(X.copy(), Xe.copy(), Xm.copy(), model_z, ze,
                                                                     lprob_func=make_hook(**kw), lprob_args=args, label_dict=d,
                                                                     verbose=False, save_fits=False)
        assert np.isfinite(p).all() and np.isfinite(out[tag + '_fp']).all() and np.isfinite(lm).all() and np.isfinite(le).all()
    assert np.isneginf(out['lnprior'][:, model_z == 0]).all() and np.isneginf(out['lnprior']).sum() == 24 * nt

    # the host functions
    rs = np.random.RandomState(18)
    out['pmag_mag'] = np.linspace(8., 30., 50)
    out['pmag_maglim'] = np.array(25.)
    out['pmag'] = rpriors.pmag(out['pmag_mag'], 25.)
    out['pmag_b'] = rpriors.pmag(out['pmag_mag'], 26.5, mbounds=(12., 29.), alpha=10., beta=1.5, gamma=0.5, Npoints=300)
    out['raw_m'] = np.array([15., 20., 23.37, 31.9, 40.])
    out['raw_zgrid'] = np.linspace(0., 16., 41)
    raw = [rpriors._bpz_prior(m, out['raw_zgrid']) for m in out['raw_m']]
    out['raw_p'], out['raw_f'] = np.array([r[0] for r in raw]), np.array([r[1] for r in raw])
    n = 200
    z, t, m = rs.uniform(0., 16., n), rs.randint(0, 3, n), rs.uniform(18., 34., n)
    z[:6] = [0., 0., 15., 20., 7.5, 15. / 999 * 400]
    m[:6] = [15., 20., 32., 40., 20. + 12. / 999 * 17, 25.]
    assert (m < 20).any() and (m > 32).any() and (z > 15).any()
    out['fn_z'], out['fn_t'], out['fn_m'] = z, t, m
    out['bpz_pt_m'] = np.array([float(rpriors.bpz_pt_m(int(ti), mi)) for ti, mi in zip(t, m)])
    out['bpz_pz_tm'] = np.array([float(rpriors.bpz_pz_tm(zi, int(ti), mi)) for zi, ti, mi in zip(z, t, m)])
    base = rpriors.bpz_pztm.values
    idx = np.stack([rs.randint(0, s, 2000) for s in base.shape], axis=1)
    idx[:3] = [[0, 0, 0], [999, 999, 2], [500, 0, 1]]
    out['base_idx'], out['base_val'] = idx, base[idx[:, 0], idx[:, 1], idx[:, 2]]
    out['ptm_idx'] = idx[:200, [0, 2]]
    out['ptm_val'] = rpriors.bpz_ptm.values[idx[:200, 0], idx[:200, 2]]

    path = os.path.join(HERE, 'g18_bpz_prior.npz')
    np.savez_compressed(path, **out)
    print('g18_bpz_prior %8.1f KB' % (os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
