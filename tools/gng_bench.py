"""Steps per second of GrowingNeuralGas.train_network at the reference's default size (niter 5000 x nbatch 50 = 2.5e5 steps,
max_nodes 2500) on the 20 000 models x 5 bands of golden case G17-g.  Prints one JSON line: wall-clock steps/s of train_network
(host tables, uploads, the per-step generator and the network read back after every launch included) and of the training kernel
alone (device time of its launches), each the median over the repeats.

    timeout -k 10 300 python tools/gng_bench.py [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def models(M, B=5):
    """tests/golden/make_golden_som.py's som_models(177, M, B, bad='err')"""
    rs = np.random.RandomState(177)
    Y = rs.lognormal(1., 1., size=(M, B)) * rs.uniform(0.5, 2., size=(M, 1))
    Ye = 0.05 * Y + 0.01
    Ym = (rs.uniform(size=(M, B)) > 0.02).astype(np.float64)
    k = max(4, M // 500)
    r, c = rs.randint(0, M, k), rs.randint(0, B, k)
    Ye[r[k // 2:], c[k // 2:]] = rs.choice([0., -1., np.inf], size=k - k // 2)
    return Y, Ye, Ym


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--niter', type=int, default=5000)
    ap.add_argument('--nbatch', type=int, default=50)
    ap.add_argument('--max-nodes', type=int, default=2500)
    ap.add_argument('--models', type=int, default=20000)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd.engine import get_engine
    from frankenz_amd.networks import GrowingNeuralGas
    eng = get_engine(None)
    T = args.niter * args.nbatch
    kw = dict(niter=args.niter, nbatch=args.nbatch, max_nodes=args.max_nodes, verbose=False)
    Y, Ye, Ym = models(args.models)
    GrowingNeuralGas(Y, Ye, Ym).train_network(rstate=np.random.RandomState(0), **dict(kw, niter=4, nbatch=2))      # warm-up
    walls, kern, nodes = [], [], []
    for r in range(args.repeat):
        Y, Ye, Ym = models(args.models)
        gng = GrowingNeuralGas(Y, Ye, Ym)
        eng.timing_reset()
        t0 = time.perf_counter()
        gng.train_network(rstate=np.random.RandomState(1707 + r), **kw)
        walls.append(time.perf_counter() - t0)
        kern.append(eng.timing()['ms_other'] * 1e-3)
        nodes.append(int(gng.NNODE))
    w, k = float(np.median(walls)), float(np.median(kern))
    print(json.dumps({'metric': 'gng_train_steps_per_s', 'nodes': nodes, 'steps': T, 'models': args.models, 'bands': 5,
                      'wall_s': w, 'steps_per_s': T / w, 'kernel_s': k, 'kernel_steps_per_s': T / k if k > 0 else None,
                      'us_per_step_kernel': 1e6 * k / T, 'walls': walls, 'kernels': kern}))


if __name__ == '__main__':
    main()
