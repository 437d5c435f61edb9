"""Posterior quantiles (docs/quantiles.md): kernel and wall seconds of `fz_row_quantiles` on the workload of tools/bins_bench.py -- 1e6
objects, K k = 500 entries per row of which about 400 count, 1e5 models, wt_thresh = 1e-3, everything device-resident -- at
q = (0.16, 0.5, 0.84) and at the five-point default, one line with label_errs = 0, and two yardsticks made of calls that predate it,
timed in the same run:

  cdf             fz_row_cdf at the same number of shared points: the cost of ONE evaluation of the solve.  The ratio stands beside
                  the measured mean number of evaluations per (row, p)
  grid route      what gives the same three numbers today: fz_knn_predict_logwt onto the 701-point dictionary grid (5.6 GB of PDFs
                  at 1e6 objects), then fz_pdfs_summarize (median and credible bounds among its 21 statistics)
  target          quant3 wall <= grid route wall

Prints one JSON line; `*_kernel_ms` are the library's own event timings, `*_s` wall seconds between synchronisations (median).

    timeout -k 10 900 python tools/quantile_bench.py [--objects 1000000] [--width 500] [--models 100000] [--repeat 5]
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
    ap.add_argument('--repeat', type=int, default=5)
    args = ap.parse_args()
    import torch                                                    # before the library is loaded: one HIP runtime in the process
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd import PDFDict
    from frankenz_amd.engine import DeviceArray, get_engine, kde_opts
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    eng = get_engine(None)
    N, W, M = args.objects, args.width, args.models
    rng = np.random.default_rng(2900)                               # tools/bins_bench.py's rows, neighbours, counts and labels
    rows = rng.random((N, W)); rows *= -12.
    nbr = rng.integers(0, M, size=(N, W), dtype=np.int64)
    nnbr = rng.integers(max(1, (3 * W) // 5), W + 1, size=N, dtype=np.int64)
    d_rows, d_nbr, d_nn = eng.device_array(rows), eng.device_array(nbr), eng.device_array(nnbr)
    E = int(nnbr.sum())
    del rows, nbr
    z = rng.uniform(0., 7., M); ze = rng.uniform(0.02, 0.2, M)
    d_z, d_ze, d_zero = eng.device_array(z), eng.device_array(ze), eng.device_array(np.zeros(M))
    lncut = np.log(1e-3)
    res = {'metric': 'row_quantiles', 'objects': N, 'width': W, 'models': M, 'valid_per_row': float(nnbr.mean()), 'entries': E}

    def timed(f):
        ts, ms = [], []
        f()                                                         # warm-up (allocations, code objects)
        for _ in range(args.repeat):
            eng.sync(); torch.cuda.synchronize(); eng.timing_reset()
            t0 = time.perf_counter()
            f()
            eng.sync(); torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
            t = eng.timing()
            ms.append(sum(v for k, v in t.items() if k.startswith('ms_')))
        return float(np.median(ts)), float(np.median(ms))

    probs = {3: np.array([0.16, 0.5, 0.84]), 5: np.array([0.025, 0.16, 0.5, 0.84, 0.975])}
    for Q, p in probs.items():
        d_p = eng.device_array(p)
        out = DeviceArray(eng, (N, Q), np.float64)
        # yardstick (a): one evaluation
        pts = eng.device_array(np.linspace(1., 6., Q))
        t, ms = timed(lambda: eng.row_cdf(d_rows, N, W, M, d_z, d_ze, pts, Q, out, per_object=False, lncut=lncut, neighbors=d_nbr, nnbr=d_nn))
        res.update({'cdf%d_s' % Q: t, 'cdf%d_kernel_ms' % Q: ms})
        cnt = []
        f = lambda: cnt.append(eng.row_quantiles(d_rows, N, W, M, d_z, d_ze, d_p, Q, out, lncut=lncut, neighbors=d_nbr, nnbr=d_nn))
        t, ms = timed(f)
        nskip, nfail, niter = cnt[-1]
        res.update({'quant%d_s' % Q: t, 'quant%d_kernel_ms' % Q: ms, 'quant%d_over_cdf%d' % (Q, Q): ms / res['cdf%d_kernel_ms' % Q],
                    'quant%d_mean_evaluations' % Q: niter / float((N - nskip) * Q), 'quant%d_nfail' % Q: nfail})
        if Q == 3:                                                  # every label a point mass: bisection to the resolution in x
            cnt = []
            f = lambda: cnt.append(eng.row_quantiles(d_rows, N, W, M, d_z, d_zero, d_p, Q, out, lncut=lncut, neighbors=d_nbr, nnbr=d_nn))
            t, ms = timed(f)
            nskip, nfail, niter = cnt[-1]
            res.update(quant3_zero_errs_s=t, quant3_zero_errs_kernel_ms=ms, quant3_zero_errs_mean_evaluations=niter / float((N - nskip) * Q),
                       quant3_zero_errs_nfail=nfail)
        del out

    # yardstick (b): the grid route
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    eng.set_labels(z, ze, label_dict=pd)
    ko = kde_opts({})
    G = pd.Ngrid
    pdfs = torch.empty((N, G), dtype=torch.float64, device=dev)
    stats = torch.empty((21, N), dtype=torch.float64, device=dev)
    urand = torch.from_numpy(rng.random(N)).to(dev)
    pt, pg = pd.grid.reshape(G, 1), pd.grid.reshape(1, G)
    loss = np.ascontiguousarray(1. - 1. / (1. + np.square((pt - pg) / ((1. + pt) * 0.15))))      # pdfs_summarize's default kernel
    predict_ms = []

    def grid_route():
        eng.knn_predict_logwt(d_rows, d_nbr, d_nn, W, ko, pdfs, n=N)
        predict_ms.append(sum(v for k, v in eng.timing().items() if k.startswith('ms_')))
        eng.pdfs_summarize(pdfs, pd.grid, True, urand, loss, None, 0.03, stats, n=N)

    t, ms = timed(grid_route)
    res.update(grid_s=t, grid_kernel_ms=ms, grid_predict_kernel_ms=float(np.median(predict_ms[1:])), quant3_over_grid=res['quant3_s'] / t,
               quant5_over_grid=res['quant5_s'] / t)
    res['target'] = 'quant3_s <= grid_s'
    res['met'] = bool(res['quant3_s'] <= t)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
