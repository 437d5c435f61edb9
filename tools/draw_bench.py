"""Posterior draws over the model set (docs/draws.md): seconds of the draw stage alone on a ln-likelihood plane already in device
memory (fz_draw_logwt) and of the whole fit_sample (fz_fit_draw), S = 16 draws per object, mode A, 5 bands, inputs and results
device-resident -- against the two existing consumers of the same materialised rows: fz_predict_logwt on the same plane (the
weight-threshold KDE onto the demo's 701-point grid) and the CDF-rule fit_predict (kde_kwargs={'wt_thresh': None}) at the same shape.
With --baseline-only only those two are run, through calls that predate the draws, so the same file measures an older checkout.
The plane of the stage-alone figures holds at most --plane-gb of rows (the first objects of the shape); the whole-call figures
run the full shape.  Prints one JSON line per shape; `timing` holds the library's per-family kernel milliseconds of the timed runs.

    timeout -k 10 900 python tools/draw_bench.py [--shapes 100000x10000 1000000x100000] [--samples 16] [--repeat 3] [--baseline-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SDSS_SIGMA = np.array([0.873, 0.348, 0.418, 0.873, 3.476])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['100000x10000', '1000000x100000'], help='objects x models')
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--plane-gb', type=float, default=80., help='most device memory the stage-alone plane may take')
    ap.add_argument('--baseline-only', action='store_true')
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd import PDFDict
    from frankenz_amd.engine import get_engine, kde_opts, like_opts
    eng = get_engine(None)
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    opts = like_opts({})
    ko_wt, ko_cdf = kde_opts({}), kde_opts({'wt_thresh': None})
    S, B = args.samples, 5

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

    for shape in args.shapes:
        N, M = (int(v) for v in shape.split('x'))
        rs = np.random.RandomState(271)
        Y = rs.lognormal(1., 1., size=(M, B)); Ye = 0.05 * Y; Ym = np.ones((M, B))
        X = Y[rs.choice(M, N)] + SDSS_SIGMA * rs.randn(N, B); Xe = np.tile(SDSS_SIGMA, (N, 1)); Xm = np.ones((N, B))
        z, ze = rs.uniform(0, 6, M), np.full(M, 0.05)
        eng.upload_models(Y, Ye, Ym)
        G = eng.set_labels(z, ze, label_dict=pd)
        dX, dXe, dXm = (eng.device_array(a) for a in (X, Xe, Xm))
        Np = int(min(N, args.plane_gb * 1e9 // (M * 8)))
        plane = eng.device_empty((Np, M))
        eng.fit(dX, dXe, dXm, opts, lnlike=plane, n=Np)
        d_pdf = eng.device_empty((N, G))
        d_lm, d_le = eng.device_empty(N), eng.device_empty(N)
        res = {'metric': 'posterior_draws', 'objects': N, 'models': M, 'bands': B, 'mode': 'A', 'samples': S, 'plane_objects': Np,
               'plane_gb': 8e-9 * Np * M}
        t, fam = timed(lambda: eng.predict_logwt(plane, ko_wt, d_pdf, d_lm, d_le, n=Np))
        res.update(predict_logwt_s=t, predict_logwt_timing=fam, predict_logwt_form=eng.last_form())
        t, fam = timed(lambda: eng.fit_predict(dX, dXe, dXm, opts, ko_cdf, d_pdf, d_lm, d_le, n=N))
        res.update(fit_predict_cdf_s=t, fit_predict_cdf_timing=fam)
        if not args.baseline_only:
            d_idx = eng.device_empty((N, S), np.int64)
            key = (0x243F6A88, 0x85A308D3)
            t, fam = timed(lambda: eng.draw_logwt(plane, S, d_idx, key=key, lmap=d_lm, levid=d_le, n=Np, W=M))
            res.update(draw_logwt_s=t, draw_logwt_timing=fam, draw_over_predict=t / res['predict_logwt_s'],
                       draw_plane_tb_per_s=8e-12 * Np * M / t)
            t, fam = timed(lambda: eng.fit_draw(dX, dXe, dXm, opts, None, S, d_idx, key=key, lmap=d_lm, levid=d_le, n=N))
            res.update(fit_sample_s=t, fit_sample_timing=fam, fit_sample_over_fit_predict_cdf=t / res['fit_predict_cdf_s'])
            drawn = d_idx.numpy()[:4096]
            res['distinct_models_drawn_first_4096_objects'] = int(len(np.unique(drawn)))
            assert drawn.min() >= 0 and drawn.max() < M
            del d_idx
        print(json.dumps(res), flush=True)
        del plane, d_pdf, dX, dXe, dXm


if __name__ == '__main__':
    main()
