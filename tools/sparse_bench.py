"""Sparse fits (docs/sparse_fits.md): seconds of the selection stage alone on a ln-posterior plane chunk already in device memory
(fz_sparsify_logwt) and of the whole fit_sparse (fz_fit_sparse, neighbours / counts / ln-like / ln-prob rows left on the device), mode A,
5 bands, inputs and results device-resident, at Nkeep 256 and 1024 with wt_thresh 1e-3 and 0 -- against the existing consumer of the
same materialised rows: fz_draw_logwt at S = 1 on the same plane chunk and fz_fit_draw at S = 1 on the same objects.  With
--baseline-only only those two are run, through calls that predate the sparse fits, so the same file measures an older checkout.
Then the median cover() -- the share of each object's posterior its sparse row holds -- and, for comparison, the cover of
NearestNeighbors.fit at K = 25, k = 20 on the first --cover-objects objects: logsumexp of its fit_lnprob row minus the exact levid.
The data are bench.py's generator (make_problem: lognormal model fluxes, SDSS-depth noise), restated here from its arguments.
Prints one JSON line; `*_timing` holds the library's per-family kernel milliseconds of the last timed run.

    timeout -k 10 900 python tools/sparse_bench.py [--nobj 200000] [--nmodel 100000] [--repeat 3] [--baseline-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SDSS_SIGMA = np.array([0.873, 0.348, 0.418, 0.873, 3.476])


def make_problem(n_obj, n_model, seed, B=5, noise=1.0):
    """bench.py's make_problem"""
    rs = np.random.RandomState(seed)
    sig = np.resize(SDSS_SIGMA, B) * noise
    Y = rs.lognormal(mean=1.0, sigma=1.0, size=(n_model, B))
    Ye = np.tile(sig, (n_model, 1)); Ym = np.ones((n_model, B))
    pick = rs.randint(0, n_model, size=n_obj)
    X = Y[pick] + sig * rs.standard_normal((n_obj, B))
    return Y, Ye, Ym, X, np.tile(sig, (n_obj, 1)), np.ones((n_obj, B))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nobj', type=int, default=200000)
    ap.add_argument('--nmodel', type=int, default=100000)
    ap.add_argument('--seed', type=int, default=20260101)
    ap.add_argument('--nband', type=int, default=5)
    ap.add_argument('--noise-scale', type=float, default=1.0)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--plane-gb', type=float, default=8., help='most device memory the stage-alone plane chunk may take')
    ap.add_argument('--cover-objects', type=int, default=4096, help='objects of the k-NN cover comparison')
    ap.add_argument('--baseline-only', action='store_true')
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd.engine import get_engine, like_opts
    eng = get_engine(None)
    opts = like_opts({})
    N, M, B = args.nobj, args.nmodel, args.nband

    def timed(f):
        ts, fam = [], {}
        f()                                                         # warm-up (allocations, code objects)
        for _ in range(args.repeat):
            eng.sync(); eng.timing_reset()
            t0 = time.perf_counter()
            f()
            eng.sync()
            ts.append(time.perf_counter() - t0)
            fam = {k: round(v, 3) for k, v in eng.timing().items() if k.startswith('ms_') and v > 0}
        return float(np.median(ts)), fam

    Y, Ye, Ym, X, Xe, Xm = make_problem(N, M, args.seed, B, args.noise_scale)
    eng.upload_models(Y, Ye, Ym)
    dX, dXe, dXm = (eng.device_array(a) for a in (X, Xe, Xm))
    Np = int(min(N, args.plane_gb * 1e9 // (M * 8)))
    plane = eng.device_empty((Np, M))
    eng.fit(dX, dXe, dXm, opts, lnlike=plane, n=Np)                 # (no prior: the ln-posterior plane is the ln-likelihood plane)
    d_lm, d_le = eng.device_empty(N), eng.device_empty(N)
    res = {'metric': 'sparse_fits', 'objects': N, 'models': M, 'bands': B, 'mode': 'A', 'plane_objects': Np, 'plane_gb': 8e-9 * Np * M}
    d_idx = eng.device_empty((N, 1), np.int64)
    key = (0x243F6A88, 0x85A308D3)
    t, fam = timed(lambda: eng.draw_logwt(plane, 1, d_idx, key=key, lmap=d_lm, levid=d_le, n=Np, W=M))
    res.update(draw_logwt_s1_s=t, draw_logwt_s1_timing=fam, draw_plane_tb_per_s=8e-12 * Np * M / t)
    t, fam = timed(lambda: eng.fit_draw(dX, dXe, dXm, opts, None, 1, d_idx, key=key, lmap=d_lm, levid=d_le, n=N))
    res.update(fit_draw_s1_s=t, fit_draw_s1_timing=fam)
    del d_idx
    if not args.baseline_only:
        d_lk = eng.device_empty(N)
        for W in (256, 1024):
            d_nb, d_nn = eng.device_empty((N, W), np.int64), eng.device_empty(N, np.int64)
            d_lnl, d_lpb = eng.device_empty((N, W)), eng.device_empty((N, W))
            for wt in (1e-3, 0.):
                lncut = float(np.log(wt)) if wt else -np.inf
                tag = 'W%d_wt%g' % (W, wt)
                t, fam = timed(lambda: eng.sparsify_logwt(plane, W, lncut, d_nb, d_nn, vals=d_lpb, lmap=d_lm, levid=d_le, lnkept=d_lk, n=Np, M=M))
                res['select_%s_s' % tag] = t
                res['select_%s_over_draw' % tag] = t / res['draw_logwt_s1_s']
                res['select_%s_timing' % tag] = fam
                t, fam = timed(lambda: eng.fit_sparse(dX, dXe, dXm, opts, None, W, lncut, d_nb, d_nn, lnlike=d_lnl, lnprob=d_lpb, lmap=d_lm,
                                                      levid=d_le, lnkept=d_lk, n=N))
                res['fit_sparse_%s_s' % tag] = t
                res['fit_sparse_%s_over_fit_draw' % tag] = t / res['fit_draw_s1_s']
                res['fit_sparse_%s_timing' % tag] = fam
                with np.errstate(invalid='ignore'):
                    cover = np.exp(d_lk.numpy() - d_le.numpy())
                res['cover_median_%s' % tag] = float(np.median(cover))
                res['cover_p01_%s' % tag] = float(np.percentile(cover, 1))
                res['nneighbors_median_%s' % tag] = float(np.median(d_nn.numpy()))
            del d_nb, d_nn, d_lnl, d_lpb
        # the recall of the Monte-Carlo k-NN fit, against the exact evidence of the same objects
        from frankenz_amd import NearestNeighbors
        n = min(N, args.cover_objects)
        levid = d_le.numpy()[:n]
        fk = dict(skynoise=np.resize(SDSS_SIGMA, B) * args.noise_scale, zeropoints=10 ** (0.4 * 23.9))
        nn = NearestNeighbors(Y, Ye, Ym, K=25, feature_map='luptitude', fmap_kwargs=fk, rstate=np.random.RandomState(1), verbose=False)
        nn.fit(X[:n].copy(), Xe[:n].copy(), Xm[:n].copy(), rstate=np.random.RandomState(2), k=20, verbose=False)
        rows = np.where(np.arange(nn.fit_lnprob.shape[1])[None, :] < nn.Nneighbors[:, None], nn.fit_lnprob, -np.inf)
        mx = rows.max(axis=1)
        with np.errstate(invalid='ignore', divide='ignore'):
            lk = mx + np.log(np.exp(rows - mx[:, None]).sum(axis=1))
            kcov = np.exp(lk - levid)
        res.update(knn_cover_objects=n, knn_cover_median=float(np.median(kcov)), knn_cover_p01=float(np.percentile(kcov, 1)),
                   knn_nneighbors_median=float(np.median(nn.Nneighbors)))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
