"""Gibbs over model weights (docs/model_weights.md): wall and kernel seconds per sweep of `model_weight_sampler`'s two modes on sparse
k-NN-shaped rows -- 1e6 objects, K k = 500 entries per row of which about 400 count, 1e5 models -- against what a user writes
without it, through calls that predate it (so that --baseline-only measures an older checkout with the same file):

  baseline_device   the draw alone: fz_draw_logwt with S = 1 on PRE-ADDED rows `lnlike + lnw[neighbors]` already in device memory
                    (forming them is not counted: it is the bound the sweep is held against)
  baseline_host     the loop itself: the rows formed on the host, `draw_logwt` from host memory (what `sample(1, logwt=)` calls),
                    np.bincount, rstate.dirichlet

  device_mode       fz_mw_chain: sweeps back to back on resident rows, every random number made on the device
  host_mode         per sweep rstate.rand(N), fz_mw_sweep on resident rows, rstate.dirichlet and np.log on the host

Prints one JSON line; `*_kernel_ms` are the library's own event timings per sweep.

    timeout -k 10 900 python tools/mw_sampler_bench.py [--objects 1000000] [--width 500] [--models 100000] [--sweeps 10] [--baseline-only]
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
    ap.add_argument('--sweeps', type=int, default=10, help='sweeps per timed device-side run')
    ap.add_argument('--host-sweeps', type=int, default=2, help='sweeps per timed run of the loops that go through the host')
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
    nnbr = rng.integers(max(1, (3 * W) // 5), W + 1, size=N, dtype=np.int64)          # about 0.8 W count
    alpha = np.ones(M)
    lnw = np.log(rs.dirichlet(alpha))
    key = (0x243F6A88, 0x85A308D3)
    d_rows, d_nbr, d_nn = eng.device_array(rows), eng.device_array(nbr), eng.device_array(nnbr)
    res = {'metric': 'model_weight_sweep', 'objects': N, 'width': W, 'models': M, 'valid_per_row': float(nnbr.mean()),
           'rows_gb': 8e-9 * N * W}

    def timed(f, nsweeps, repeat):
        ts, ms = [], 0.
        f()                                                         # warm-up (allocations, code objects)
        for _ in range(repeat):
            eng.sync(); eng.timing_reset()
            t0 = time.perf_counter()
            f()
            eng.sync()
            ts.append(time.perf_counter() - t0)
            ms = eng.timing()['ms_other']
        return float(np.median(ts)) / nsweeps, ms / nsweeps

    def pre_added(lw):
        t = lw[nbr]; t += rows
        return t

    # ---- baselines: calls the parent commit has ----
    d_t = eng.device_array(pre_added(lnw))
    d_idx = eng.device_empty((N, 1), np.int64)
    state = {'s': 0}

    def base_device():
        for _ in range(args.sweeps):
            state['s'] += 1
            eng.draw_logwt(d_t, 1, d_idx, key=(key[0], key[1] + state['s']), neighbors=d_nbr, nnbr=d_nn, n=N, W=W)
    t, ms = timed(base_device, args.sweeps, args.repeat)
    res.update(baseline_device_sweep_s=t, baseline_device_kernel_ms=ms, baseline_device_tb_per_s=8e-12 * float(nnbr.sum()) / (1e-3 * ms))
    del d_t, d_idx

    def base_host():
        lw = lnw
        idx = np.empty((N, 1), dtype=np.int64)
        for _ in range(args.host_sweeps):
            eng.draw_logwt(pre_added(lw), 1, idx, u=rs.rand(N, 1), neighbors=nbr, nnbr=nnbr, n=N, W=W)
            counts = np.bincount(idx[idx >= 0], minlength=M)
            lw = np.log(rs.dirichlet(alpha + counts))
    t, ms = timed(base_host, args.host_sweeps, 1)
    res.update(baseline_host_sweep_s=t, baseline_host_kernel_ms=ms)

    if not args.baseline_only:
        d_alpha = eng.device_array(alpha)
        counts, pos = np.zeros(M, dtype=np.int64), np.empty(M)

        def device_mode():
            d_lnw = eng.device_array(lnw)
            eng.mw_chain(d_rows, N, W, M, d_alpha, d_lnw, key, 0, args.sweeps, counts, pos, neighbors=d_nbr, nnbr=d_nn)
        t, ms = timed(device_mode, args.sweeps, args.repeat)
        res.update(device_mode_sweep_s=t, device_mode_kernel_ms=ms, device_mode_over_baseline_device=t / res['baseline_device_sweep_s'],
                   device_mode_kernel_over_baseline_kernel=ms / res['baseline_device_kernel_ms'],
                   device_mode_tb_per_s=16e-12 * float(nnbr.sum()) / (1e-3 * ms))
        assert counts.sum() == N and abs(pos.sum() - 1.) < 1e-9

        def host_mode():
            lw = lnw
            for _ in range(args.host_sweeps):
                eng.mw_sweep(d_rows, N, W, M, lw, counts, u=rs.rand(N), neighbors=d_nbr, nnbr=d_nn)
                lw = np.log(rs.dirichlet(alpha + counts))
        t, ms = timed(host_mode, args.host_sweeps, args.repeat)
        res.update(host_mode_sweep_s=t, host_mode_kernel_ms=ms, host_mode_over_baseline_host=t / res['baseline_host_sweep_s'])
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
