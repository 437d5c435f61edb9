"""G17: GrowingNeuralGas.train_network of the reference (networks.py:1870-2260), recorded for tests/test_gng_host.py and
tests/test_hip_gng.py.  Run from the repository root with the reference importable (as make_golden_som.py is):

    python tests/golden/make_golden_gng.py [--cases abcdefhg] [--out FILE]

Recorded per case: the two initial rows and the draw stream (a recording stand-in for the RandomState), every step's BMU, NNODE and
nprune of every batch, the final node ids, positions, errors, the adjacency in neighbour order (CSR) with the edge ages, which
entries of the caller's arrays changed and what the two aliased rows hold afterwards.  The reference's graph class is replaced by a
logging subclass for the run, so that the script sees every edge and node removal.  It asserts the margins that make an exact
comparison fair -- the smallest relative gap between the best, second and third node ln-prob of any step, and between the two
largest unequal errors wherever the insertion takes an arg-max -- and that the cases together cover a removed node, a duplicate
prune entry, a pruned edge whose age had been reset, and a draw of an aliased row.  Case g (the default size) takes minutes."""
import argparse
import hashlib
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('FRANKENZ_REFERENCE', '/root/reference'))

import networkx as nx  # noqa: E402
from frankenz import networks as rnet  # noqa: E402

sys.path.insert(0, HERE)
from make_golden_som import som_models, lp_foreign, changed  # noqa: E402

LOG = None


class ProbeGraph(nx.Graph):
    """logs what the batch ends do to the graph: the state of every edge handed to remove_edge, and every node removal"""

    def add_node(self, n, **attr):
        if LOG is not None and 'pos' in attr and n not in self:
            LOG['inserting'] = True                                # the insertion: its remove_edge(e1, e2) is not a prune entry
        super(ProbeGraph, self).add_node(n, **attr)

    def remove_edge(self, u, v):
        if LOG is not None:
            if LOG['inserting']:
                LOG['inserting'] = False
            else:
                key = (min(u, v), max(u, v))
                if self.has_edge(u, v):
                    LOG['pruned'] += 1
                    if self.edges[u, v]['age'] < LOG['max_age']:
                        LOG['reset'] += 1
                elif key in LOG['batch']:
                    LOG['dup'] += 1
                else:
                    LOG['stale'] += 1
                LOG['batch'].add(key)
        super(ProbeGraph, self).remove_edge(u, v)

    def remove_node(self, n):
        if LOG is not None:
            LOG['removed'] += 1
        super(ProbeGraph, self).remove_node(n)


class Recorder(object):
    """RandomState stand-in: records the initial pair and every scalar choice (the per-step draws)"""
    def __init__(self, seed):
        self.rs = np.random.RandomState(seed); self.draws = []; self.init = None

    def choice(self, a, size=None, replace=True, p=None):
        out = self.rs.choice(a, size=size, replace=replace, p=p)
        if size is None:
            self.draws.append(int(out))
        else:
            self.init = np.array(out, dtype=np.int64)
        return out


def rel_gap(hi, lo):
    return (hi - lo) / max(1., abs(hi))


def top_unequal_gap(vals):
    """relative gap (hi - lo) / hi between the largest value and the largest one below it (inf if all are equal).  Accumulated
    errors are sums and products of non-negative terms that decay by 0.5 % per step, down to 1e-30 and below for a node that is
    never the BMU: another summation order moves each by a relative amount, so the gap is taken relative to the larger value itself
    (the ln-prob gaps above are relative to max(1, |ln-prob|), as in make_golden_som.py)."""
    vals = np.asarray(vals, dtype=np.float64)
    top = vals.max()
    rest = vals[vals < top]
    return (top - rest.max()) / abs(top) if len(rest) and top != 0. else np.inf


def run(tag, Y, Ye, Ym, seed, err_kernel=None, **kw):
    global LOG
    gng = rnet.GrowingNeuralGas(Y, Ye, Ym)
    rec = Recorder(seed)
    models_err = Ye if err_kernel is None else np.sqrt(Ye**2 + err_kernel**2)
    nbatch, max_age, max_nodes = kw.get('nbatch', 50), kw.get('max_age', 15), kw.get('max_nodes', 2500)
    LOG = {'inserting': False, 'pruned': 0, 'reset': 0, 'dup': 0, 'stale': 0, 'removed': 0, 'batch': set(), 'max_age': max_age}
    saved = rnet.nx
    rnet.nx = types.SimpleNamespace(Graph=ProbeGraph, get_node_attributes=nx.get_node_attributes)
    bmus, nnode, nprune = [], [], []
    gap12 = gap23 = gap_e1 = gap_e2 = np.inf
    t0 = time.time()
    try:
        steps = gng._train_network(Y, models_err, Ym, rstate=rec, **kw)
        prev_err, prev_order = None, None
        if kw.get('graph_init') is not None:
            prev_order = list(kw['graph_init'].nodes())
            prev_err = {n: kw['graph_init'].nodes[n]['error'] for n in prev_order}
        i = -1
        while True:
            batch_end = (i + 1) % nbatch == 0
            if batch_end and i >= 0:
                # the state the coming batch end starts from: node order and errors after the previous step
                prev_order = list(gng.graph.nodes())
                prev_err = {n: gng.graph.nodes[n]['error'] for n in prev_order}
            try:
                res, bmu, nn, npr = next(steps)
            except StopIteration:
                break
            i += 1
            lp = np.asarray(res[2], dtype=np.float64)
            bmus.append(int(bmu))
            if len(lp) >= 3:
                t3 = np.partition(lp, -3)[-3:]
                gap12, gap23 = min(gap12, rel_gap(t3[2], t3[1])), min(gap23, rel_gap(t3[1], t3[0]))
            else:
                t2 = np.sort(lp)
                gap12 = min(gap12, rel_gap(t2[1], t2[0]))
            if i % nbatch == 0:
                nnode.append(int(nn)); nprune.append(int(npr))
                LOG['batch'] = set()
                g = gng.graph
                # (step 0 of a fresh network is left out: its errors are all zero but the BMU's)
                inserted = [n for n in g.nodes() if n not in prev_err] if prev_err is not None else []
                if inserted:
                    new = inserted[0]
                    e1, e2 = list(g.neighbors(new))
                    # errors the arg-max saw: the previous step's, plus this step's chi2 on the BMU, on the nodes that survived
                    err = dict(prev_err)
                    err[bmu] += np.asarray(res[4])[prev_order.index(bmu)]
                    live = [n for n in g.nodes() if n != new]
                    gap_e1 = min(gap_e1, top_unequal_gap([err[n] for n in live]))
                    assert e1 == live[int(np.argmax([err[n] for n in live]))], (tag, i)
                    nb1 = [n for n in g.neighbors(e1) if n != new] + [e2]
                    gap_e2 = min(gap_e2, top_unequal_gap([err[n] for n in nb1]))
    finally:
        rnet.nx = saved
        log, LOG = LOG, None
    g = gng.graph
    ids = np.array(list(g.nodes()), dtype=np.int64)
    count = {int(n): k for k, n in enumerate(ids)}
    assert [g.nodes[n]['count'] for n in g.nodes()] == list(range(len(ids)))
    off = np.zeros(len(ids) + 1, dtype=np.int32)
    nbr, age = [], []
    for k, n in enumerate(ids):
        for m in g.neighbors(int(n)):
            nbr.append(count[int(m)]); age.append(g.edges[int(n), m]['age'])
        off[k + 1] = len(nbr)
    draws = np.array(rec.draws, dtype=np.int64)
    alias = 0 if rec.init is None else int(np.isin(draws, rec.init).sum())
    out = {'draws': draws, 'bmus': np.array(bmus, dtype=np.int16), 'nnode': np.array(nnode, dtype=np.int16),
           'nprune': np.array(nprune, dtype=np.int32), 'ids': ids.astype(np.int32),
           'pos': np.array([g.nodes[int(n)]['pos'] for n in ids]), 'err': np.array([g.nodes[int(n)]['error'] for n in ids]),
           'adj_off': off, 'adj_nbr': np.array(nbr, dtype=np.int32), 'adj_age': np.array(age, dtype=np.int32),
           'nodes': np.asarray(gng.nodes), 'init': np.zeros(0, dtype=np.int64) if rec.init is None else rec.init,
           'gaps': np.array([gap12, gap23, gap_e1, gap_e2]),
           'cover': np.array([log['removed'], log['dup'], log['reset'], alias, log['pruned'], log['stale']], dtype=np.int64)}
    assert np.array_equal(out['nodes'], out['pos']) or kw.get('track_scale', False)
    print('%s: %d steps in %.1f s, NNODE %d, gaps (bmu 1-2, 2-3, e1, e2) %s, removed %d dup %d reset %d alias %d pruned %d stale %d'
          % (tag, len(bmus), time.time() - t0, len(ids), np.array2string(out['gaps'], precision=3), log['removed'], log['dup'],
             log['reset'], alias, log['pruned'], log['stale']))
    if kw.get('lprob_func') is None:
        assert min(gap12, gap23, gap_e1, gap_e2) > 1e-9, tag
    return gng, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='abcdefhg')
    ap.add_argument('--g-seed', type=int, default=1707, help='RandomState seed of case g (kept in the file)')
    ap.add_argument('--out', default=os.path.join(HERE, 'g17_gng_train.npz'))
    args = ap.parse_args()
    out = dict(np.load(args.out)) if os.path.exists(args.out) else {}

    def inputs(tag, Y, Ye, Ym):
        out[tag + '_in_sums'] = np.array([np.sum(np.where(np.isfinite(Y), Y, 0)), np.sum(np.where(np.isfinite(Ye), Ye, 0)), Ym.sum()])
        out[tag + '_in_bad'] = np.flatnonzero(~(np.isfinite(Y) & np.isfinite(Ye) & (Ye > 0))).astype(np.int32)

    def case(tag, mseed, M, B, bad, rseed, small_draws=True, **kw):
        if tag not in args.cases:
            return
        for k in [k for k in out if k.startswith(tag + '_')]:
            del out[k]
        Y, Ye, Ym = som_models(mseed, M, B, bad)
        inputs(tag, Y, Ye, Ym)
        Y0, Ye0, Ym0 = Y.copy(), Ye.copy(), Ym.copy()
        gng, res = run(tag, Y, Ye, Ym, rseed, **kw)
        if len(res['init']):
            # the device path needs the two initial rows clean (a clean would reach into a node's position mid-run)
            assert not np.isin(out[tag + '_in_bad'] // B, res['init']).any() or kw.get('lprob_func') is not None, tag
            res['rows_after'] = Y[res['init']].copy()
        res['out_changed'] = np.stack([changed(Y, Y0), changed(Ye, Ye0), changed(Ym, Ym0)])
        if tag == 'g':
            res['bmus_sha1'] = np.frombuffer(hashlib.sha1(res['bmus'].astype(np.int64).tobytes()).digest(), dtype=np.uint8)
            res['draws_head'] = res['draws'][:1000]
            del res['bmus'], res['draws'], res['nodes']
        else:
            res['draws'] = res['draws'].astype(np.int16 if M < 32768 else np.int32)
        for k, v in res.items():
            out[tag + '_' + k] = v
        return gng

    dflt = {'free_scale': True, 'ignore_model_err': True}
    # a: defaults at a small size, bad errors that the likelihood cleans
    case('a', 171, 3000, 5, 'err', 1701, niter=300, nbatch=20, max_nodes=120, max_age=8)
    # b: 8 bands, heavy pruning
    case('b', 172, 400, 8, False, 1702, niter=300, nbatch=10, max_nodes=60, max_age=4)
    # c: track_scale with the scale returned
    case('c', 173, 2000, 5, 'err', 1703, niter=200, nbatch=20, max_nodes=100, max_age=8, track_scale=True,
         lprob_kwargs=dict(dflt, return_scale=True))
    # d: fixed scale, model errors kept (dim_prior on), err_kernel; short max_age (duplicate prune entries)
    case('d', 174, 2000, 5, 'err', 1704, niter=200, nbatch=20, max_nodes=100, max_age=6, err_kernel=0.02,
         lprob_kwargs={'free_scale': False, 'ignore_model_err': False})
    if 'd' in args.cases:
        out['d_err_kernel'] = np.array(0.02)
    # e: graph_init with 6 nodes, labels out of order, ring edges of several ages
    if 'e' in args.cases:
        Y, _, _ = som_models(175, 2000, 5, 'err')
        rs = np.random.RandomState(1755)
        labels = [3, 0, 5, 1, 4, 2]
        g0 = nx.Graph()
        rows = rs.choice(2000, 6, replace=False)
        e_pos = Y[rows] * rs.uniform(0.8, 1.2, size=(6, 1))
        e_err = rs.uniform(0., 30., size=6)
        for k, n in enumerate(labels):
            g0.add_node(n, pos=e_pos[k].copy(), error=float(e_err[k]))
        e_edges = [(3, 0, 2), (0, 5, 0), (5, 1, 5), (1, 4, 1), (4, 2, 3), (2, 3, 0), (3, 1, 4)]
        for u, v, a in e_edges:
            g0.add_edge(u, v, age=a)
        gng = case('e', 175, 2000, 5, 'err', 1705, niter=200, nbatch=20, max_nodes=100, max_age=8, graph_init=g0)
        assert gng.graph is g0
        out['e_init_labels'], out['e_init_pos'], out['e_init_err'] = np.array(labels), e_pos, e_err
        out['e_init_edges'] = np.array(e_edges)
    # f: a foreign lprob_func (host loop)
    case('f', 176, 500, 5, False, 1706, niter=30, nbatch=10, max_nodes=40, max_age=8, lprob_func=lp_foreign)
    # h: every step is a batch end; the network grows past 64 and past 1 024 slots
    case('h', 178, 3000, 5, 'err', 1708, niter=1300, nbatch=1, max_nodes=1200)
    if all(t + '_cover' in out for t in 'abcdh'):
        cover = sum(out[t + '_cover'] for t in 'abcdh')
        print('coverage over a-d, h: removed %d, duplicate entries %d, pruned after reset %d, aliased draws %d' % tuple(cover[:4]))
        assert (cover[:4] > 0).all()
    # g: the default size on 20 000 models
    case('g', 177, 20000, 5, 'err', args.g_seed)
    if 'g' in args.cases:
        out['g_seed'] = np.array(args.g_seed)
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out))


if __name__ == '__main__':
    main()
