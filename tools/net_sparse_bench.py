"""Network fits as sparse rows (docs/network.md, "Sparse rows"): seconds of the union stage alone (fz_net_union: the counting call, and
counting + emitting the table) on a selection already in device memory, of fz_net_table on the same selection (the stage of
Network.fit it replaces: the concatenated lists, repeats and all), of the subset likelihood inside fit_sparse (the library's ms_knn
timer), of the whole Network.fit_sparse(resident=True) and of Network.fit on the same inputs -- medians of --repeat runs after one
warm-up.  Mode A for the objects, 5 bands, bench.py's generator (make_problem: lognormal model fluxes, SDSS-depth noise), restated
here from its arguments.  The network: --nnode model rows as nodes, populated as usual.  The objects are the first --nobj that select
at most --nsel-max nodes, and every node's list is then cut to its first L models, L the largest length at which no object's summed
list length exceeds --rawlen-max (4 096: the most Network.fit takes), so that both routes run on the same inputs.  With --skip-fit Network.fit is left out (it holds eight (n, rawlen) host arrays per chunk of
65 536 objects).  Prints one JSON line; `*_timing` holds the library's per-family kernel milliseconds of the last timed run.

    timeout -k 10 1100 python tools/net_sparse_bench.py [--nobj 100000] [--nmodel 100000] [--nnode 1000] [--repeat 5] [--skip-fit]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SDSS_SIGMA = np.array([0.873, 0.348, 0.418, 0.873, 3.476])


def make_problem(n_obj, n_model, seed, B=5, noise=1.0):
    """bench.py's make_problem"""
    rs = np.random.RandomState(seed)
    sig = np.resize(SDSS_SIGMA, B) * noise
    Y = rs.lognormal(mean=1.0, sigma=1.0, size=(n_model, B))
    Ye = np.tile(sig, (n_model, 1)); Ym = np.ones((n_model, B))
    pick = rs.randint(0, n_model, size=n_obj)
    X = Y[pick] + sig * rs.standard_normal((n_obj, B))
    return Y, Ye, Ym, X, np.tile(sig, (n_obj, 1)), np.ones((n_obj, B))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nobj', type=int, default=100000)
    ap.add_argument('--nmodel', type=int, default=100000)
    ap.add_argument('--nnode', type=int, default=1000)
    ap.add_argument('--seed', type=int, default=20260101)
    ap.add_argument('--nband', type=int, default=5)
    ap.add_argument('--wt-thresh', type=float, default=1e-3, help='the selection rule of the objects (weight rule)')
    ap.add_argument('--nsel-max', type=int, default=64, help='objects that select more nodes than this are left out')
    ap.add_argument('--rawlen-max', type=int, default=4096)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--skip-fit', action='store_true')
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd.engine import get_engine, like_opts
    from frankenz_amd.networks import Network, _csr
    eng = get_engine(None)
    N, M, B = args.nobj, args.nmodel, args.nband

    def timed(f, repeat=args.repeat):
        ts, fam = [], {}
        f()                                                         # warm-up (allocations, code objects)
        for _ in range(repeat):
            eng.sync(); eng.timing_reset()
            t0 = time.perf_counter()
            f()
            eng.sync()
            ts.append(time.perf_counter() - t0)
            fam = {k: round(v, 3) for k, v in eng.timing().items() if k.startswith('ms_') and v > 0}
        return float(np.median(ts)), fam

    Y, Ye, Ym, X, Xe, Xm = make_problem(2 * N, M, args.seed, B)      # (twice the objects: those that select too many nodes are left out)
    rs = np.random.RandomState(args.seed + 1)
    net = Network(Y, Ye, Ym)
    net.set_nodes(Y[rs.choice(M, args.nnode, replace=False)].copy())
    t0 = time.perf_counter()
    net.populate_network(verbose=False)
    res = {'metric': 'net_sparse', 'objects': N, 'models': M, 'bands': B, 'nodes': args.nnode, 'populate_s': time.perf_counter() - t0}

    # the selection of the objects, on the device (what fit and fit_sparse both form first)
    match_sel = np.arange(net.NNODE)[net.nodes_Nmatch > 0]
    y = np.ascontiguousarray(net.nodes[match_sel]); Nn = len(y)
    eng.upload_models(y, np.zeros_like(y), np.ones_like(y))

    def select(X, Xe, Xm):
        n = len(X)
        plane = eng.device_empty((n, Nn))
        eng.fit(X.copy(), Xe.copy(), Xm.copy(), like_opts(net.lpnet_kwargs), plane, n=n)
        d_nsel, d_sel = eng.device_empty((n,), np.int32), eng.device_empty((n, Nn), np.int32)
        eng.net_select(plane, True, args.wt_thresh, 0.5, None, None, d_nsel, d_sel)
        return d_nsel, d_sel

    # the first N objects that select at most --nsel-max nodes (an object far from every node selects them all), then the lists cut
    # to L entries: rawlen <= nsel_max * L <= rawlen_max for every object
    nsel_all = select(X, Xe, Xm)[0].numpy()
    few = np.flatnonzero(nsel_all <= args.nsel_max)[:N]
    if len(few) < N:
        raise SystemExit("only %d of %d objects select at most %d nodes" % (len(few), 2 * N, args.nsel_max))
    X, Xe, Xm = X[few], Xe[few], Xm[few]
    d_nsel, d_sel = select(X, Xe, Xm)
    nsel = d_nsel.numpy()
    res.update(objects_left_out_share=float((nsel_all[:few[-1] + 1] > args.nsel_max).mean()))
    L = max(1, args.rawlen_max // max(int(nsel.max()), 1))
    net.nodes_idxs = [v[:L] for v in net.nodes_idxs]
    net.nodes_Nmatch = np.array([len(v) for v in net.nodes_idxs], dtype='int')
    off, items = _csr(net.nodes_idxs)
    lens = np.diff(off)
    d_match, d_off, d_items = eng.device_array(match_sel.astype(np.int32)), eng.device_array(off), eng.device_array(items)
    res.update(matched_nodes=Nn, list_cut=L, list_len_median=float(np.median(lens[lens > 0])), nsel_median=float(np.median(nsel)),
               nsel_max=int(nsel.max()))

    d_nu = eng.device_empty((N,), np.int64)
    t, fam = timed(lambda: eng.net_union(d_nsel, d_sel, d_match, d_off, d_items, M, d_nu, n=N, nn=Nn))
    res.update(union_count_s=t, union_count_timing=fam)
    nuniq = d_nu.numpy()
    W = int(nuniq.max())
    d_idx = eng.device_empty((N, W), np.int64)
    t, fam = timed(lambda: eng.net_union(d_nsel, d_sel, d_match, d_off, d_items, M, d_nu, W, d_idx, n=N, nn=Nn))
    res.update(union_emit_s=t, union_emit_timing=fam, union_count_and_emit_s=res['union_count_s'] + t, width=W,
               nuniq_median=float(np.median(nuniq)))
    del d_idx
    # the stage of Network.fit it replaces: the concatenated lists at the width of the longest
    sel_h = d_sel.numpy()
    rawlen = np.array([lens[match_sel[sel_h[i, :nsel[i]]]].sum() for i in range(N)], dtype=np.int64)
    Wraw = int(rawlen.max())
    d_tab = eng.device_empty((N, Wraw), np.int64)
    t, fam = timed(lambda: eng.net_table(d_nsel, d_sel, d_match, d_off, d_items, Wraw, d_tab))
    res.update(net_table_s=t, net_table_timing=fam, rawlen_max=Wraw, rawlen_median=float(np.median(rawlen)))
    del d_tab, d_nsel, d_sel, d_nu

    kw = dict(wt_thresh=args.wt_thresh, verbose=False)
    t, fam = timed(lambda: net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), resident=True, **kw))
    res.update(fit_sparse_resident_s=t, fit_sparse_timing=fam, subset_likelihood_s=fam.get('ms_knn', 0.) * 1e-3,
               union_below_subset_likelihood=bool(res['union_count_and_emit_s'] < fam.get('ms_knn', 0.) * 1e-3))
    if not args.skip_fit:
        t, fam = timed(lambda: net.fit(X.copy(), Xe.copy(), Xm.copy(), **kw))
        res.update(network_fit_s=t, network_fit_timing=fam, fit_sparse_over_network_fit=res['fit_sparse_resident_s'] / t)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
