"""Monte-Carlo draws of the k-NN fitter on the device (docs/knn.md, "Monte-Carlo draws on the device") at the benchmark's k-NN shape:
1e6 objects x 1e5 models, 5 bands, K = 25 feature sets, k = 20.  Three measurements, the two versions of each alternated within this
one process after a warm-up of both, wall clock around calls that end in a device synchronise, medians of --repeat runs:

  (a) the device-resident step  prep.run(dX, dXe, dXm, out=, query_features=dQ)  (features drawn beforehand: what bench.py times)
      against  prep.run(dX, dXe, dXm, out=, query_draws='device')  (the draw inside the step);
  (b) NumPy in -> NumPy out  fit_predict(save_fits=False)  with query_draws='host' against 'device', and the host's time in
      ``_query_features`` alone;
  (c) the constructor with feature_draws='host' (plus the upload of its sets, which the first fit pays) against 'device' (draw, copy-out
      and installation in one), and the time of installing given sets alone -- copy, SoA pack, the host-side k-d ordering, the
      matrix-pipe operands -- which both versions pay.

Prints one JSON line.

    timeout -k 10 900 python tools/knn_mc_bench.py [--objects 1000000] [--models 100000] [--repeat 3] [--skip-numpy]
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
    ap.add_argument('--objects', type=int, default=1000000)
    ap.add_argument('--models', type=int, default=100000)
    ap.add_argument('--K', type=int, default=25)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--skip-numpy', action='store_true', help='leave out (b): it returns (objects, 701) float64 arrays on the host')
    args = ap.parse_args()
    import torch                                                    # before the library is loaded: one HIP runtime in the process (as bench.py)
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd import NearestNeighbors, PDFDict
    from frankenz_amd.engine import get_engine
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    eng = get_engine(0)
    N, M, K, k, B = args.objects, args.models, args.K, args.k, 5
    rs = np.random.RandomState(20260101)
    Y = rs.lognormal(1., 1., size=(M, B)); Ye = np.tile(SDSS_SIGMA, (M, 1)); Ym = np.ones((M, B))
    X = Y[rs.randint(0, M, size=N)] + SDSS_SIGMA * rs.standard_normal((N, B)); Xe = np.tile(SDSS_SIGMA, (N, 1)); Xm = np.ones((N, B))
    z, ze = rs.uniform(0, 6, M), np.full(M, 0.05)
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    fk = dict(skynoise=SDSS_SIGMA, zeropoints=10 ** (0.4 * 23.9))
    res = {'metric': 'knn_mc_draws', 'objects': N, 'models': M, 'bands': B, 'K': K, 'k': k, 'repeat': args.repeat}

    def clock(f):
        eng.sync(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        eng.sync(); torch.cuda.synchronize()
        return time.perf_counter() - t0

    def alternated(fa, fb):
        fa(); fb()                                                  # warm-up of both (allocations, code objects, page-locked blocks)
        ta, tb = [], []
        for _ in range(args.repeat):
            ta.append(clock(fa)); tb.append(clock(fb))
        return float(np.median(ta)), float(np.median(tb)), ta, tb

    # ---- (c) the constructor --------------------------------------------------------------------------------------------------
    mk = lambda draws: NearestNeighbors(Y, Ye, Ym, K=K, feature_map='luptitude', fmap_kwargs=fk, rstate=np.random.RandomState(1), verbose=False,
                                        device=0, feature_draws=draws)
    made = {}

    def ctor_host():
        made['host'] = mk('host')
        eng._trees_key = None
        made['host']._engine()                                      # the upload and installation the first fit would pay

    def ctor_device():
        made['device'] = mk('device')

    th, td, _, _ = alternated(ctor_host, ctor_device)
    feats = made['device']._feats

    def install():
        eng._trees_key = None
        eng.knn_upload_trees(feats, key=made['device']._feats_key)

    ti = float(np.median([clock(install) for _ in range(args.repeat)]))
    tdraw = float(np.median([clock(lambda: mk('host')) for _ in range(max(1, args.repeat - 1))]))
    res['constructor'] = {'host_draw_plus_install_s': th, 'device_draw_install_copyout_s': td, 'host_draw_alone_s': tdraw,
                          'install_given_sets_s': ti, 'install_share_of_device_constructor': ti / td, 'speedup': th / td}

    # ---- (a) the device-resident step -------------------------------------------------------------------------------------------
    nn = made['device']
    prep = nn.prepare_fit_predict(z, ze, label_dict=pd, kde_kwargs={'wt_thresh': 1e-3}, lprob_kwargs={}, k=k)
    dX, dXe, dXm = (torch.from_numpy(a).to(dev) for a in (X, Xe, Xm))
    out = (torch.empty((N, pd.Ngrid), dtype=torch.float64, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
           torch.empty(N, dtype=torch.float64, device=dev))
    key = np.random.RandomState(2).randint(0, 2**32, size=2, dtype=np.uint32)
    dQ = nn.query_features(dX, dXe, draws='device', key=key)        # the same features on both sides: the searches do the same work
    t_given, t_drawn, ta, tb = alternated(lambda: prep.run(dX, dXe, dXm, out=out, query_features=dQ),
                                          lambda: prep.run(dX, dXe, dXm, out=out, rstate=np.random.RandomState(2), query_draws='device'))
    t_draw = float(np.median([clock(lambda: nn.query_features(dX, dXe, draws='device', key=key)) for _ in range(args.repeat + 2)][2:]))
    res['device_step'] = {'features_given_s': t_given, 'features_drawn_in_step_s': t_drawn, 'added': t_drawn / t_given - 1.,
                          'draw_call_alone_s': t_draw, 'runs_given_s': ta, 'runs_drawn_s': tb}
    del out, dQ

    # ---- (b) NumPy in -> NumPy out --------------------------------------------------------------------------------------------
    if not args.skip_numpy:
        kw = dict(label_dict=pd, kde_kwargs={'wt_thresh': 1e-3}, k=k, save_fits=False, verbose=False)
        t_host, t_dev, ta, tb = alternated(
            lambda: nn.fit_predict(X, Xe, Xm, z, ze, rstate=np.random.RandomState(2), query_draws='host', **kw),
            lambda: nn.fit_predict(X, Xe, Xm, z, ze, rstate=np.random.RandomState(2), query_draws='device', **kw))
        t_q = float(np.median([clock(lambda: nn._query_features(X, Xe, np.random.RandomState(2))) for _ in range(args.repeat)]))
        t_qd = float(np.median([clock(lambda: nn.query_features(X, Xe, draws='device', key=key)) for _ in range(args.repeat)]))
        res['numpy_call'] = {'query_draws_host_s': t_host, 'query_draws_device_s': t_dev, 'host_query_features_alone_s': t_q,
                             'device_query_features_numpy_round_trip_s': t_qd, 'runs_host_s': ta, 'runs_device_s': tb}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
