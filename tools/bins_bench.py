"""Posterior bin masses (docs/bins.md): kernel and wall seconds of `fz_row_bins` on sparse k-NN-shaped rows -- 1e6 objects, K k = 500
entries per row of which about 400 count, 1e5 models, everything device-resident -- at 8 unequal tomographic bins and at 70 bins of
0.1, against two routes made of calls that predate it, timed in the same run:

  moments_mean    fz_row_moments, the mean alone of a 5-band table, on the same rows (tools/moments_bench.py's lean call): the byte
                  yardstick, 16 + 40 bytes per counted entry
  grid route      fz_knn_predict_logwt onto the 701-point dictionary grid (5.6 GB of PDFs at 1e6 objects) followed by a device-side
                  sum of the grid points of every bin (one fp64 matrix product with the (701, Nbins) membership matrix)
  target          bins8 wall <= grid8 wall: the new path reads the same rows, writes 1 / 88 of the bytes and evaluates 9 erfc per
                  included entry

Prints one JSON line; `*_kernel_ms` are the library's own event timings, `*_s` wall seconds between synchronisations (median).

    timeout -k 10 900 python tools/bins_bench.py [--objects 1000000] [--width 500] [--models 100000] [--repeat 5]
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
    rng = np.random.default_rng(2900)
    rows = rng.random((N, W)); rows *= -12.
    nbr = rng.integers(0, M, size=(N, W), dtype=np.int64)
    nnbr = rng.integers(max(1, (3 * W) // 5), W + 1, size=N, dtype=np.int64)          # about 0.8 W count
    d_rows, d_nbr, d_nn = eng.device_array(rows), eng.device_array(nbr), eng.device_array(nnbr)
    E = int(nnbr.sum())
    del rows, nbr
    z = rng.uniform(0., 7., M); ze = rng.uniform(0.02, 0.2, M)
    d_z, d_ze = eng.device_array(z), eng.device_array(ze)
    edges = {8: np.array([0., 0.3, 0.5, 0.7, 0.9, 1.2, 1.6, 2.5, 7.]), 70: np.arange(71) * 0.1}
    res = {'metric': 'row_bins', 'objects': N, 'width': W, 'models': M, 'valid_per_row': float(nnbr.mean()), 'entries': E}

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

    # the byte yardstick
    d_V = eng.device_array(rng.lognormal(1., 1., size=(M, 5)))
    mean = DeviceArray(eng, (N, 5), np.float64)
    t, ms = timed(lambda: eng.row_moments(d_rows, N, W, M, 5, d_V, mean, neighbors=d_nbr, nnbr=d_nn))
    del mean, d_V
    res.update(moments_mean_s=t, moments_mean_kernel_ms=ms)

    # the new path
    for NB, e in edges.items():
        out = DeviceArray(eng, (N, NB), np.float64)
        d_e = eng.device_array(e)
        f = lambda: eng.row_bins(d_rows, N, W, M, d_z, d_ze, d_e, NB + 1, out, lncut=np.log(1e-3), normalize=True, neighbors=d_nbr, nnbr=d_nn)
        t, ms = timed(f)
        res.update({'bins%d_s' % NB: t, 'bins%d_kernel_ms' % NB: ms, 'bins%d_over_moments_mean' % NB: ms / res['moments_mean_kernel_ms']})
        if NB == 8:
            p8 = out.numpy()
        del out

    # the grid route
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    eng.set_labels(z, ze, label_dict=pd)
    ko = kde_opts({})
    pdfs = torch.empty((N, pd.Ngrid), dtype=torch.float64, device=dev)
    for NB, e in edges.items():
        k = np.searchsorted(e, pd.grid, side='right') - 1           # the bin with e_k <= grid point < e_k+1
        A = np.zeros((pd.Ngrid, NB))
        ok = (k >= 0) & (k < NB)
        A[np.arange(pd.Ngrid)[ok], k[ok]] = 1.
        d_A = torch.from_numpy(A).to(dev)
        got = torch.empty((N, NB), dtype=torch.float64, device=dev)

        def grid_route():
            eng.knn_predict_logwt(d_rows, d_nbr, d_nn, W, ko, pdfs, n=N)
            torch.matmul(pdfs, d_A, out=got)
            got.div_(got.sum(dim=1, keepdim=True))

        t, ms = timed(grid_route)
        res.update({'grid%d_s' % NB: t, 'grid%d_predict_kernel_ms' % NB: ms, 'bins%d_over_grid' % NB: res['bins%d_s' % NB] / t})
        if NB == 8:
            res['grid8_max_abs_diff'] = float(np.nanmax(np.abs(got.cpu().numpy() - p8)))     # (a Riemann sum of a discretised kernel)
    res['target'] = 'bins8_s <= grid8_s'
    res['met'] = bool(res['bins8_s'] <= res['grid8_s'])
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
