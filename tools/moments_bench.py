"""Posterior moments (docs/predictive.md): kernel and wall seconds of `fz_row_moments` on sparse k-NN-shaped rows -- 1e6 objects,
K k = 500 entries per row of which about 400 count, 1e5 models x 5 bands, everything device-resident -- against `fz_mw_loglike` on
the same rows, a call that predates the moments (so that --baseline-only measures an older checkout with the same file).

  baseline        fz_mw_loglike: 24 bytes per counted entry (row value, index, gathered ln-weight)
  moments         fz_row_moments with scales, errors and masks, mean + var + share: 16 + 8 + 8 L 3 bytes per counted entry
  moments_mean    ... the mean alone (no second walk), without scale, errors and mask: 16 + 8 L bytes
  target          moments_kernel_ms <= (bytes ratio) x baseline_kernel_ms
  --zeropoint N   one whole `calibrate.zeropoint_offsets` iteration at N objects against the `fit_sparse` call it contains

Prints one JSON line; `*_kernel_ms` are the library's own event timings.

    timeout -k 10 900 python tools/moments_bench.py [--objects 1000000] [--width 500] [--models 100000] [--bands 5] [--baseline-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=1000000)
    ap.add_argument('--width', type=int, default=500, help='K k: entries per row')
    ap.add_argument('--models', type=int, default=100000)
    ap.add_argument('--bands', type=int, default=5)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--zeropoint', type=int, default=0, help='objects of the zero-point iteration (0: not run)')
    ap.add_argument('--baseline-only', action='store_true')
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd.engine import get_engine
    eng = get_engine(None)
    N, W, M, L = args.objects, args.width, args.models, args.bands
    rng = np.random.default_rng(2900)
    rows = rng.random((N, W)); rows *= -12.
    nbr = rng.integers(0, M, size=(N, W), dtype=np.int64)
    nnbr = rng.integers(max(1, (3 * W) // 5), W + 1, size=N, dtype=np.int64)          # about 0.8 W count
    lnw = np.log(np.random.RandomState(2901).dirichlet(np.ones(M)))
    d_rows, d_nbr, d_nn = eng.device_array(rows), eng.device_array(nbr), eng.device_array(nnbr)
    E = int(nnbr.sum())
    res = {'metric': 'row_moments', 'objects': N, 'width': W, 'models': M, 'bands': L, 'valid_per_row': float(nnbr.mean()), 'entries': E}
    del nbr

    def timed(f, repeat):
        ts, ms = [], []
        f()                                                         # warm-up (allocations, code objects)
        for _ in range(repeat):
            eng.sync(); eng.timing_reset()
            t0 = time.perf_counter()
            f()
            eng.sync()
            ts.append(time.perf_counter() - t0)
            ms.append(eng.timing()['ms_other'])
        return float(np.median(ts)), float(np.median(ms))

    d_lnw = eng.device_array(lnw)
    t, ms = timed(lambda: eng.mw_loglike(d_rows, N, W, M, d_lnw, neighbors=d_nbr, nnbr=d_nn), args.repeat)
    res.update(baseline_s=t, baseline_kernel_ms=ms, baseline_tb_per_s=24e-12 * E / (1e-3 * ms))

    if not args.baseline_only:
        from frankenz_amd.engine import DeviceArray
        rows *= -1. / 12.; rows += 0.5                                # the scales: uniform in [0.5, 1.5)
        d_sc = eng.device_array(rows)
        del rows
        V = rng.lognormal(1., 1., size=(M, L))
        d_V, d_Ve, d_Vm = eng.device_array(V), eng.device_array(0.05 * V), eng.device_array((rng.random((M, L)) > 0.05).astype(np.float64))
        mean, var, share = (DeviceArray(eng, (N, L), np.float64) for _ in range(3))
        full = lambda: eng.row_moments(d_rows, N, W, M, L, d_V, mean, var=var, share=share, value_errs=d_Ve, value_mask=d_Vm, scale=d_sc,
                                       neighbors=d_nbr, nnbr=d_nn)
        t, ms = timed(full, args.repeat)
        ratio = (16 + 8 + 8 * L * 3) / 24.
        res.update(moments_s=t, moments_kernel_ms=ms, bytes_ratio=ratio, moments_over_baseline=ms / res['baseline_kernel_ms'],
                   target_ms=ratio * res['baseline_kernel_ms'], met=bool(ms <= ratio * res['baseline_kernel_ms']),
                   moments_tb_per_s=(16 + 8 + 8 * L * 3) * 1e-12 * E / (1e-3 * ms))
        lean = lambda: eng.row_moments(d_rows, N, W, M, L, d_V, mean, neighbors=d_nbr, nnbr=d_nn)
        t, ms = timed(lean, args.repeat)
        res.update(moments_mean_s=t, moments_mean_kernel_ms=ms, moments_mean_bytes_ratio=(16 + 8 * L) / 24.,
                   moments_mean_over_baseline=ms / res['baseline_kernel_ms'])
        m = mean.numpy()
        assert np.isfinite(m).all() and (m > 0).all()

        if args.zeropoint:
            from frankenz_amd import BruteForce, calibrate
            Nz = args.zeropoint
            Y = V; Ye = 0.02 * Y; Ym = np.ones_like(Y)
            X = Y[rng.integers(0, M, Nz)]; Xe = 0.05 * X
            X = (X + Xe * rng.standard_normal(X.shape)) * np.linspace(0.95, 1.05, L); Xm = np.ones_like(X)
            bf = BruteForce(Y, Ye, Ym)
            fit = lambda: bf.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), Nkeep=256, track_scale=True, verbose=False)
            fit()
            t0 = time.perf_counter(); fit(); t_fit = time.perf_counter() - t0
            t0 = time.perf_counter()
            calibrate.zeropoint_offsets(bf, X, Xe, Xm, Niter=1, ref_band=0, Nkeep=256, verbose=False)
            t_it = time.perf_counter() - t0
            res.update(zeropoint_objects=Nz, zeropoint_iteration_s=t_it, zeropoint_fit_sparse_s=t_fit, zeropoint_over_fit=t_it / t_fit)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
