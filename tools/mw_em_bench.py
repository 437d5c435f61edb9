"""EM over model weights (docs/model_weights.md, "EM"): wall and kernel seconds per iteration of `fz_mw_em` on sparse k-NN-shaped rows
-- 1e6 objects, K k = 500 entries per row of which about 400 count, 1e5 models, device-resident -- against the Gibbs sweep of
`fz_mw_chain` on the same rows, timed through calls that predate the iteration (so that --baseline-only measures an older checkout
with the same file), and the time of the index build, once.

  baseline        fz_mw_chain: sweeps back to back on resident rows
  em              fz_mw_em: iterations back to back on resident rows and index
  em_rows / em_cols / em_weights   the iteration's kernel time by family, from the library's events (FZ_MW_EM_STAGES = 1, 2 stop every
                  iteration after the row pass / the column pass; differences of the totals)

Prints one JSON line; `*_kernel_ms` are the library's own event timings per sweep / iteration.

    timeout -k 10 900 python tools/mw_em_bench.py [--objects 1000000] [--width 500] [--models 100000] [--sweeps 10] [--baseline-only]
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
    ap.add_argument('--sweeps', type=int, default=10, help='sweeps / iterations per timed run')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--baseline-only', action='store_true')
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd.engine import get_engine
    eng = get_engine(None)
    N, W, M = args.objects, args.width, args.models
    rng = np.random.default_rng(2900)
    rs = np.random.RandomState(2901)
    rows = rng.random((N, W)); rows *= -12.
    nbr = rng.integers(0, M, size=(N, W), dtype=np.int64)
    # a popular model in a share of the rows: column lengths are heavy-tailed in practice
    nbr[rng.random(N) < 0.3, 0] = 0
    nnbr = rng.integers(max(1, (3 * W) // 5), W + 1, size=N, dtype=np.int64)          # about 0.8 W count
    alpha = np.ones(M)
    lnw = np.log(rs.dirichlet(alpha))
    key = (0x243F6A88, 0x85A308D3)
    d_rows, d_nbr, d_nn = eng.device_array(rows), eng.device_array(nbr), eng.device_array(nnbr)
    E = int(nnbr.sum())
    res = {'metric': 'model_weight_em', 'objects': N, 'width': W, 'models': M, 'valid_per_row': float(nnbr.mean()), 'rows_gb': 8e-9 * N * W,
           'entries': E}
    del rows, nbr

    def timed(f, n, repeat):
        ts, ms = [], 0.
        f()                                                         # warm-up (allocations, code objects)
        for _ in range(repeat):
            eng.sync(); eng.timing_reset()
            t0 = time.perf_counter()
            f()
            eng.sync()
            ts.append(time.perf_counter() - t0)
            ms = eng.timing()['ms_other']
        return float(np.median(ts)) / n, ms / n

    d_alpha = eng.device_array(alpha)
    counts, pos = np.zeros(M, dtype=np.int64), np.empty(M)

    def chain():
        d_lnw = eng.device_array(lnw)
        eng.mw_chain(d_rows, N, W, M, d_alpha, d_lnw, key, 0, args.sweeps, counts, pos, neighbors=d_nbr, nnbr=d_nn)
    t, ms = timed(chain, args.sweeps, args.repeat)
    res.update(baseline_sweep_s=t, baseline_kernel_ms=ms, baseline_tb_per_s=16e-12 * E / (1e-3 * ms))

    if not args.baseline_only:
        from frankenz_amd.engine import DeviceArray
        E2, nbytes = eng.mw_em_index_bytes(N, W, M, d_nn)
        assert E2 == E
        index = (DeviceArray(eng, (M + 1,), np.int64), DeviceArray(eng, (E,), np.int32), DeviceArray(eng, (E,), np.float64))
        eng.sync(); eng.timing_reset()
        t0 = time.perf_counter()
        eng.mw_em_index(d_rows, N, W, M, d_nbr, d_nn, E, *index)
        eng.sync()
        res.update(index_build_s=time.perf_counter() - t0, index_build_kernel_ms=eng.timing()['ms_other'], index_gb=1e-9 * nbytes)
        c, trace, nskip = np.empty(M), np.empty(args.sweeps), np.empty(args.sweeps, dtype=np.int64)

        def em():
            d_lnw = eng.device_array(lnw)
            eng.mw_em(d_rows, N, W, M, d_alpha, d_lnw, args.sweeps, pos, c, trace, nskip, neighbors=d_nbr, nnbr=d_nn, index=index, entries=E)
        t, ms = timed(em, args.sweeps, args.repeat)
        assert abs(pos.sum() - 1.) < 1e-9 and abs(c.sum() - (N - nskip[-1])) < 1e-6 * N and np.diff(trace).min() > -1e-6
        res.update(em_iter_s=t, em_kernel_ms=ms, em_over_baseline=t / res['baseline_sweep_s'], em_kernel_over_baseline_kernel=ms / res['baseline_kernel_ms'],
                   em_tb_per_s=28e-12 * E / (1e-3 * ms), lnpost_first=float(trace[0]), lnpost_last=float(trace[-1]))
        stage = {}
        for k in ('1', '2'):
            os.environ['FZ_MW_EM_STAGES'] = k
            stage[k] = timed(em, args.sweeps, 1)[1]
        del os.environ['FZ_MW_EM_STAGES']
        res.update(em_rows_kernel_ms=stage['1'], em_cols_kernel_ms=stage['2'] - stage['1'], em_weights_kernel_ms=ms - stage['2'])
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
