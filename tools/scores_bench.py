"""Posterior scoring rules (docs/scores.md): kernel and wall seconds of `fz_row_scores` on the workload of tools/bins_bench.py -- 1e6
objects, K k = 500 entries per row of which about 400 count, 1e5 models, wt_thresh = 1e-3, everything device-resident -- with one truth
per object: the whole call (lnpdf, crps, sqnorm), the stage kernel alone (want = lnpdf), the distribution of the included counts and
the pair evaluations per second, and two yardsticks made of calls that predate it, timed in the same run:

  cdf             fz_row_cdf at one per-object point on the same rows: ONE gather walk with one erfc.  The stage kernel makes three
                  walks; the ratio is reported
  grid route      what gives the same scores today: fz_knn_predict_logwt onto the 701-point dictionary grid (5.6 GB of PDFs at 1e6
                  objects), then CRPS and the integral of p^2 by cumulative sums on the device

For context, not as a bar: how far the grid route's CRPS lies from the closed form on the first 1e5 objects when every label error is
below the grid step (0.001 .. 0.005 against 0.01).

Prints one JSON line; `*_kernel_ms` are the library's own event timings, `*_s` wall seconds between synchronisations (median).

    timeout -k 10 900 python tools/scores_bench.py [--objects 1000000] [--width 500] [--models 100000] [--repeat 5]
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
    del rows, nbr
    z = rng.uniform(0., 7., M); ze = rng.uniform(0.02, 0.2, M)
    truth = rng.uniform(0., 7., N)
    d_z, d_ze, d_x = eng.device_array(z), eng.device_array(ze), eng.device_array(truth)
    lncut = np.log(1e-3)
    res = {'metric': 'row_scores', 'objects': N, 'width': W, 'models': M, 'valid_per_row': float(nnbr.mean())}

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

    one = lambda: DeviceArray(eng, (N, 1), np.float64)
    lnpdf, crps, sqnorm, cdf = one(), one(), DeviceArray(eng, (N,), np.float64), one()
    ninc = DeviceArray(eng, (N,), np.int64)
    kw = dict(per_object=True, lncut=lncut, neighbors=d_nbr, nnbr=d_nn)

    # yardstick (a): one gather walk with one erfc
    t, ms = timed(lambda: eng.row_cdf(d_rows, N, W, M, d_z, d_ze, d_x, 1, cdf, **kw))
    res.update(cdf_s=t, cdf_kernel_ms=ms)
    t, ms = timed(lambda: eng.row_scores(d_rows, N, W, M, d_z, d_ze, d_x, 1, lnpdf=lnpdf, ninc=ninc, **kw))
    res.update(stage_s=t, stage_kernel_ms=ms, stage_over_cdf=ms / res['cdf_kernel_ms'])
    t, ms = timed(lambda: eng.row_scores(d_rows, N, W, M, d_z, d_ze, d_x, 1, lnpdf=lnpdf, crps=crps, sqnorm=sqnorm, ninc=ninc, **kw))
    n = ninc.numpy().astype(np.float64)
    pairs = float((n * (n + 1.) / 2.).sum())
    res.update(scores_s=t, scores_kernel_ms=ms, pairs=pairs, pairs_per_s=pairs / max(1e-9, (ms - res['stage_kernel_ms']) * 1e-3),
               included={k: float(v) for k, v in zip(('min', 'p05', 'median', 'p95', 'max'), np.percentile(n, [0, 5, 50, 95, 100]))},
               included_mean=float(n.mean()))
    closed = crps.numpy()[:, 0]

    # yardstick (b): the grid route
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    ko = kde_opts({})
    G = pd.Ngrid
    dz = float(pd.grid[1] - pd.grid[0])
    grid = torch.from_numpy(np.ascontiguousarray(pd.grid)).to(dev)
    t_x = torch.from_numpy(truth).to(dev)
    pdfs = torch.empty((N, G), dtype=torch.float64, device=dev)
    predict_ms, keep = [], {}

    def grid_scores(p, x):
        p = p / (p.sum(dim=1, keepdim=True) * dz)
        c = torch.cumsum(p, dim=1).mul_(dz)
        c.sub_((grid[None, :] >= x[:, None]).to(torch.float64))
        return c.square_().sum(dim=1).mul_(dz), p.square().sum(dim=1).mul_(dz)

    def grid_route(n=N):
        eng.knn_predict_logwt(d_rows, d_nbr, d_nn, W, ko, pdfs, n=n)
        predict_ms.append(sum(v for k, v in eng.timing().items() if k.startswith('ms_')))
        keep['crps'], keep['sqnorm'] = grid_scores(pdfs[:n], t_x[:n])

    eng.set_labels(z, ze, label_dict=pd)
    t, ms = timed(grid_route)
    res.update(grid_s=t, grid_predict_kernel_ms=float(np.median(predict_ms[1:])), scores_over_grid=res['scores_s'] / t)
    res['grid_crps_minus_closed_median_abs'] = float(np.median(np.abs(keep['crps'].cpu().numpy() - closed)))

    # context: label errors below the grid step, the first 1e5 objects
    n1 = min(N, 100000)
    ze1 = rng.uniform(0.001, 0.005, M)
    eng.row_scores(d_rows, n1, W, M, d_z, eng.device_array(ze1), d_x, 1, crps=crps, **kw)
    closed = crps.numpy()[:n1, 0]
    eng.set_labels(z, ze1, label_dict=pd)
    grid_route(n1)
    d = np.abs(keep['crps'].cpu().numpy() - closed)
    res.update(narrow_closed_crps_median=float(np.median(closed)), narrow_grid_crps_abs_diff_median=float(np.median(d)),
               narrow_grid_crps_abs_diff_p95=float(np.percentile(d, 95)), narrow_grid_crps_abs_diff_max=float(d.max()))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
