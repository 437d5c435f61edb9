"""Steps per second of SelfOrganizingMap.train_network at the reference's default size (nside 50 -> 2 500 nodes, nproj 2,
niter 2000 x nbatch 50 = 1e5 steps) on 20 000 models x 5 bands.  Prints one JSON line: wall-clock steps/s of train_network (host
tables, uploads and the per-step generator included) and of the training kernel alone (device time of its launches).

    timeout -k 10 300 python tools/som_bench.py [--repeat 3]
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
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--nside', type=int, default=50)
    ap.add_argument('--niter', type=int, default=2000)
    ap.add_argument('--nbatch', type=int, default=50)
    ap.add_argument('--models', type=int, default=20000)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd.engine import get_engine
    from frankenz_amd.networks import SelfOrganizingMap
    rs = np.random.RandomState(157)
    M, B = args.models, 5
    Y = rs.lognormal(1., 1., size=(M, B)) * rs.uniform(0.5, 2., size=(M, 1))
    Ye = 0.05 * Y + 0.01
    Ym = (rs.uniform(size=(M, B)) > 0.02).astype(np.float64)
    eng = get_engine(None)
    T = args.niter * args.nbatch
    kw = dict(nside=args.nside, niter=args.niter, nbatch=args.nbatch, verbose=False)
    SelfOrganizingMap(Y, Ye, Ym).train_network(rstate=np.random.RandomState(0), **dict(kw, niter=2, nbatch=2))      # warm-up
    walls, kern = [], []
    for r in range(args.repeat):
        som = SelfOrganizingMap(Y, Ye, Ym)
        eng.timing_reset()
        t0 = time.perf_counter()
        som.train_network(rstate=np.random.RandomState(r), **kw)
        walls.append(time.perf_counter() - t0)
        kern.append(eng.timing()['ms_other'] * 1e-3)
    w, k = float(np.median(walls)), float(np.median(kern))
    print(json.dumps({'metric': 'som_train_steps_per_s', 'nodes': args.nside**2, 'steps': T, 'models': M, 'bands': B,
                      'wall_s': w, 'steps_per_s': T / w, 'kernel_s': k, 'kernel_steps_per_s': T / k if k > 0 else None,
                      'us_per_step_kernel': 1e6 * k / T, 'walls': walls, 'kernels': kern}))


if __name__ == '__main__':
    main()
