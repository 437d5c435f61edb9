"""G22: the reference's hierarchical_sampler (samplers.py:311-535) on dense pdfs = exp(lnlike), lnlike the reference's own `loglike`
on a small mock (400 objects x 24 models x 5 bands), recorded for tests/test_mw_host.py and tests/test_hip_mw.py: the law that
`frankenz_amd.samplers.model_weight_sampler` follows with the models in the place of the label grid.  Data only.  Run from the
repository root with the reference importable (as make_golden.py is):

    python tests/golden/make_golden_mw.py

Two chains, alpha = 1 and alpha = 0.3, 400 saved samples at thin = 5 each.  Stored: the mock, lnlike, and per chain `samples`,
`samples_lnp`."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('FRANKENZ_REFERENCE', '/root/reference'))

from frankenz import pdf as rpdf  # noqa: E402
from frankenz import samplers as rsamp  # noqa: E402

N, M, B, NITER, THIN = 400, 24, 5, 400, 5


def main():
    rs = np.random.RandomState(2200)
    Y = rs.lognormal(1., 0.6, size=(M, B)); Ye = 0.05 * Y; Ym = np.ones((M, B))
    w_true = rs.dirichlet(np.full(M, 0.7))
    truth = rs.choice(M, N, p=w_true)
    sig = rs.uniform(0.5, 1.5, B)
    X = Y[truth] + sig * rs.randn(N, B); Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, B))
    lnlike = np.array([rpdf.loglike(X[i].copy(), Xe[i].copy(), Xm[i].copy(), Y, Ye, Ym)[0] for i in range(N)])
    out = dict(X=X, Xe=Xe, Xm=Xm, Y=Y, Ye=Ye, Ym=Ym, w_true=w_true, truth=truth.astype(np.int64), lnlike=lnlike)
    pdfs = np.exp(lnlike)
    for tag, a in (('a1', 1.), ('a03', 0.3)):
        t0 = time.time()
        s = rsamp.hierarchical_sampler(pdfs)
        s.run_mcmc(NITER, alpha=np.full(M, a), thin=THIN, rstate=np.random.RandomState(2201 + int(10 * a)), verbose=False)
        smp, lnp = s.results
        print('%s: reference chain of %d samples in %.1f s' % (tag, len(smp), time.time() - t0))
        out[tag + '_alpha'] = np.full(M, a)
        out[tag + '_samples'], out[tag + '_samples_lnp'] = smp, lnp
    path = os.path.join(HERE, 'g22_model_weights')
    np.savez_compressed(path, **out)
    print('wrote', path + '.npz', os.path.getsize(path + '.npz'))


if __name__ == '__main__':
    main()
