"""GrowingNeuralGas training, host side (no GPU): the draw stream, and the package's host loop -- the reference's step loop
restated on plain ordered dictionaries, without networkx -- driven by a NumPy likelihood, against G17
(tests/golden/g17_gng_train.npz, made by tests/golden/make_golden_gng.py from the reference): every BMU, NNODE and nprune, the
final labels, positions, errors, adjacency order and edge ages, and the caller's arrays afterwards, bit for bit."""
import math
import os

import numpy as np
import pytest

from frankenz_amd import networks as net

G17 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g17_gng_train.npz')
DFLT = {'free_scale': True, 'ignore_model_err': True}
MODELS = {'a': (171, 3000, 5, 'err'), 'b': (172, 400, 8, False), 'c': (173, 2000, 5, 'err'), 'd': (174, 2000, 5, 'err'),
          'e': (175, 2000, 5, 'err'), 'f': (176, 500, 5, False), 'h': (178, 3000, 5, 'err'), 'g': (177, 20000, 5, 'err')}
SEED = {'a': 1701, 'b': 1702, 'c': 1703, 'd': 1704, 'e': 1705, 'f': 1706, 'h': 1708, 'g': 1707}
KW = {
    'a': dict(niter=300, nbatch=20, max_nodes=120, max_age=8),
    'b': dict(niter=300, nbatch=10, max_nodes=60, max_age=4),
    'c': dict(niter=200, nbatch=20, max_nodes=100, max_age=8, track_scale=True, lprob_kwargs=dict(DFLT, return_scale=True)),
    'd': dict(niter=200, nbatch=20, max_nodes=100, max_age=6, lprob_kwargs={'free_scale': False, 'ignore_model_err': False}),
    'e': dict(niter=200, nbatch=20, max_nodes=100, max_age=8),
    'f': dict(niter=30, nbatch=10, max_nodes=40, max_age=8),
    'h': dict(niter=1300, nbatch=1, max_nodes=1200),
    'g': dict(),
}


def som_models(seed, M, B, bad=True):
    """tests/golden/make_golden_som.py's models: G17 keeps their sums and which entries are bad, the tests regenerate them"""
    rs = np.random.RandomState(seed)
    Y = rs.lognormal(1., 1., size=(M, B)) * rs.uniform(0.5, 2., size=(M, 1))
    Ye = 0.05 * Y + 0.01
    Ym = (rs.uniform(size=(M, B)) > 0.02).astype(np.float64)
    if bad:
        k = max(4, M // 500)
        r, c = rs.randint(0, M, k), rs.randint(0, B, k)
        if bad is True:
            Y[r[:k // 2], c[:k // 2]] = np.nan
        Ye[r[k // 2:], c[k // 2:]] = rs.choice([0., -1., np.inf], size=k - k // 2)
    return Y, Ye, Ym


def case_models(g, tag):
    """the case's models, checked against what G17 recorded of them"""
    Y, Ye, Ym = som_models(*MODELS[tag])
    np.testing.assert_allclose([np.sum(np.where(np.isfinite(Y), Y, 0)), np.sum(np.where(np.isfinite(Ye), Ye, 0)), Ym.sum()],
                               g[tag + '_in_sums'], rtol=1e-13)
    np.testing.assert_array_equal(np.flatnonzero(~(np.isfinite(Y) & np.isfinite(Ye) & (Ye > 0))), g[tag + '_in_bad'])
    return Y, Ye, Ym


def case_kwargs(g, tag):
    """the keywords of the case; case e's initial graph as a FakeGraph or (networkx=True) an nx.Graph"""
    kw = dict(KW[tag])
    if tag == 'd':
        kw['err_kernel'] = float(g['d_err_kernel'])
    return kw


class FakeGraph(object):
    """the few members of a networkx.Graph the package reads from ``graph_init`` and writes back to (so that the tests need no
    networkx): ordered nodes with attributes, ordered adjacency with shared edge attributes"""

    def __init__(self):
        self._node, self._adj = {}, {}

    def add_node(self, n, **attr):
        if n not in self._node:
            self._node[n] = {}; self._adj[n] = {}
        self._node[n].update(attr)

    def add_edge(self, u, v, **attr):
        d = self._adj[u].get(v, {})
        d.update(attr)
        self._adj[u][v] = self._adj[v][u] = d

    def clear(self):
        self._node.clear(); self._adj.clear()

    def number_of_nodes(self):
        return len(self._node)

    @property
    def nodes(self):
        g = self

        class View(dict):
            def __call__(self):
                return list(g._node)
        return View(self._node)

    def neighbors(self, n):
        return iter(self._adj[n])

    @property
    def edges(self):
        g = self

        class View(object):
            def __getitem__(self, uv):
                return g._adj[uv[0]][uv[1]]
        return View()


def init_graph(g, graph=None):
    """case e's initial graph (6 nodes, labels out of order, a ring and a chord, several ages)"""
    graph = FakeGraph() if graph is None else graph
    for n, p, e in zip(g['e_init_labels'], g['e_init_pos'], g['e_init_err']):
        graph.add_node(int(n), pos=p.copy(), error=float(e))
    for u, v, a in g['e_init_edges']:
        graph.add_edge(int(u), int(v), age=int(a))
    return graph


def expected_arrays(g, tag, Y, Ye, Ym):
    """the caller's arrays after training: the entries G17 saw change are cleaned (pdf.py:309-311) or, in the two rows the initial
    nodes are views of, hold the nodes' positions"""
    ch = g[tag + '_out_changed']
    out = []
    for a, k, v in zip((Y, Ye, Ym), range(3), (0., 1., 0.)):
        a = a.copy(); a.ravel()[ch[k]] = v; out.append(a)
    if len(g[tag + '_init']):
        out[0][g[tag + '_init']] = g[tag + '_rows_after']
    return out


def numpy_logprob(x, xe, xm, y, ye, ym, free_scale=False, ignore_model_err=False, dim_prior=True, return_scale=False, **kw):
    """pdf.py:76-98 / 171-235 / 309-311 for one row against noiseless, unmasked nodes, in NumPy (the package's own logprob runs on
    the device): cleans the row in place, returns the reference's tuple"""
    bad = ~(np.isfinite(x) & np.isfinite(xe) & (xe > 0.))
    x[bad], xe[bad], xm[bad] = 0., 1., False
    tot_var = np.square(xe) + np.zeros_like(y)
    tot_mask = xm * np.ones_like(y)
    Ndim = np.sum(tot_mask, axis=1)
    scale = np.ones(len(y))
    if free_scale:
        inter = np.sum(tot_mask * y * x[None, :] / tot_var, axis=1)
        shape = np.sum(tot_mask * np.square(y) / tot_var, axis=1)
        scale = inter / shape
        chi2 = np.sum(tot_mask * np.square(x - scale[:, None] * y) / tot_var, axis=1)
    else:
        chi2 = np.sum(tot_mask * np.square(x - y) / tot_var, axis=1)
    if dim_prior:
        a = 0.5 * (Ndim - 1) if free_scale else 0.5 * Ndim
        with np.errstate(all='ignore'):
            xl = np.where(a - 1. == 0, np.where(np.isnan(chi2), chi2, 0.), (a - 1.) * np.log(chi2))
        lnl = xl - chi2 / 2. - np.array([math.lgamma(v) for v in a]) - np.log(2.) * a
    else:
        lnl = -0.5 * chi2 - 0.5 * (Ndim * np.log(2. * np.pi) + np.sum(np.log(tot_var), axis=1))
    out = (np.zeros_like(lnl), lnl, lnl, Ndim, chi2)
    return out + (scale, np.zeros_like(scale)) if return_scale else out


def lp_foreign(x, xe, xm, y, ye, ym, *args, **kwargs):
    """case f's user likelihood: a plain chi2 without cleaning or priors"""
    chi2 = np.sum(xm * (x - y)**2 / xe**2, axis=1)
    lnl = -0.5 * chi2
    return np.zeros_like(lnl), lnl, lnl, np.sum(xm * ym, axis=1), chi2


def check_network(gng, g, tag, exact=True, rtol=0.):
    """the trained network against G17: structure equal, positions and errors equal (exact) or within rtol"""
    np.testing.assert_array_equal(gng.graph_ids, g[tag + '_ids'])
    np.testing.assert_array_equal(gng.graph_adj_off, g[tag + '_adj_off'])
    np.testing.assert_array_equal(gng.graph_adj_nbr, g[tag + '_adj_nbr'])
    np.testing.assert_array_equal(gng.graph_adj_age, g[tag + '_adj_age'])
    assert gng.NNODE == len(g[tag + '_ids'])
    fit = g[tag + '_nodes'] if tag + '_nodes' in g else g[tag + '_pos']
    if exact:
        np.testing.assert_array_equal(gng.graph_pos, g[tag + '_pos'])
        np.testing.assert_array_equal(gng.graph_errors, g[tag + '_err'])
        np.testing.assert_array_equal(gng.nodes, fit)
    else:
        np.testing.assert_allclose(gng.graph_pos, g[tag + '_pos'], rtol=rtol)
        np.testing.assert_allclose(gng.graph_errors, g[tag + '_err'], rtol=rtol)
        np.testing.assert_allclose(gng.nodes, fit, rtol=rtol)


def check_graph(graph, gng, g, tag):
    """``graph`` (networkx or FakeGraph) holds the same network, in the reference's node and adjacency order"""
    ids = [int(v) for v in g[tag + '_ids']]
    assert list(graph.nodes()) == ids
    off, nbr, age = g[tag + '_adj_off'], g[tag + '_adj_nbr'], g[tag + '_adj_age']
    for k, n in enumerate(ids):
        assert graph.nodes[n]['count'] == k
        assert graph.nodes[n]['error'] == gng.graph_errors[k]
        np.testing.assert_array_equal(graph.nodes[n]['pos'], gng.graph_pos[k])
        assert list(graph.neighbors(n)) == [ids[j] for j in nbr[off[k]:off[k + 1]]]
        assert [graph.edges[n, m]['age'] for m in graph.neighbors(n)] == list(age[off[k]:off[k + 1]])


def run_steps(gng, Y, Ye, Ym, seed, lprob_func=None, **kw):
    """(bmu, NNODE, nprune) of every step of the _train_network generator, as train_network would drive it"""
    ek = kw.pop('err_kernel', None)
    err = Ye if ek is None else np.sqrt(Ye**2 + ek**2)
    out = [s[1:] for s in gng._train_network(Y, err, Ym, rstate=np.random.RandomState(seed), lprob_func=lprob_func, **kw)]
    return np.array(out, dtype=np.int64)


def check_steps(steps, g, tag, nbatch):
    np.testing.assert_array_equal(steps[:, 0], g[tag + '_bmus'])
    np.testing.assert_array_equal(steps[::nbatch, 1], g[tag + '_nnode'])
    np.testing.assert_array_equal(steps[::nbatch, 2], g[tag + '_nprune'])
    np.testing.assert_array_equal(steps[:, 1], np.repeat(g[tag + '_nnode'], nbatch)[:len(steps)])
    np.testing.assert_array_equal(steps[:, 2], np.repeat(g[tag + '_nprune'], nbatch)[:len(steps)])


@pytest.fixture(scope='module')
def g():
    return dict(np.load(G17))


def test_draw_stream_is_one_choice_pair_and_one_randint_call(g):
    """rstate.choice(Nmodel, size=2, replace=False), then rstate.choice(Nmodel) once per step == one randint call of size T"""
    a, b = np.random.RandomState(1701), np.random.RandomState(1701)
    ia = a.choice(3000, size=2, replace=False)
    per_step = np.array([a.choice(3000) for _ in range(6000)])
    ib = b.choice(3000, size=2, replace=False)
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(net._draw_stream(b, 3000, 6000), per_step)
    np.testing.assert_array_equal(ia, g['a_init'])
    np.testing.assert_array_equal(per_step, g['a_draws'])


def test_golden_margins_and_coverage(g):
    """what make_golden_gng.py asserted when it recorded G17, re-read from the file"""
    for tag in 'abcdehg':
        assert (g[tag + '_gaps'] > 1e-9).all(), tag
    cover = sum(g[t + '_cover'] for t in 'abcdh')
    assert (cover[:4] > 0).all()           # removed nodes, duplicate prune entries, edges pruned after a reset, aliased draws


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd', 'e', 'h'])
def test_host_loop_reproduces_g17(g, tag):
    Y, Ye, Ym = case_models(g, tag)
    Y0, Ye0, Ym0 = Y.copy(), Ye.copy(), Ym.copy()
    kw = case_kwargs(g, tag)
    graph0 = None
    if tag == 'e':
        graph0 = kw['graph_init'] = init_graph(g)
    gng = net.GrowingNeuralGas(Y, Ye, Ym)
    steps = run_steps(gng, Y, Ye, Ym, SEED[tag], lprob_func=numpy_logprob, **kw)
    check_steps(steps, g, tag, kw['nbatch'])
    check_network(gng, g, tag)
    for got, want in zip((Y, Ye, Ym), expected_arrays(g, tag, Y0, Ye0, Ym0)):
        np.testing.assert_array_equal(got, want)
    if graph0 is not None:
        assert gng.graph is graph0                                        # trained in place
        check_graph(graph0, gng, g, tag)
    elif gng.graph is not None:
        check_graph(gng.graph, gng, g, tag)
        for k in range(2):                                                # the two initial nodes still are the caller's rows
            if k in gng.graph.nodes():
                assert np.shares_memory(gng.graph.nodes[k]['pos'], Y)


def test_foreign_lprob_func_runs_the_host_loop(g):
    Y, Ye, Ym = case_models(g, 'f')
    gng = net.GrowingNeuralGas(Y, Ye, Ym)
    res = list(gng._train_network(Y, Ye, Ym, rstate=np.random.RandomState(SEED['f']), lprob_func=lp_foreign, **KW['f']))
    assert len(res[0][0]) == 5 and len(res[0][0][2]) == 2                   # node_results as the reference yields them
    steps = np.array([r[1:] for r in res], dtype=np.int64)
    check_steps(steps, g, 'f', KW['f']['nbatch'])
    check_network(gng, g, 'f')


def test_train_network_progress_line_and_defaults(g, capsys):
    import inspect
    sig = inspect.signature(net.GrowingNeuralGas.train_network)
    want = dict(models=None, models_err=None, models_mask=None, learn_best=0.2, learn_neighbor=0.005, max_age=15, nbatch=50,
                new_err_dec=0.5, all_err_dec=5e-3, max_nodes=2500, niter=5000, graph_init=None, err_kernel=None, lprob_func=None,
                rstate=None, lprob_args=None, lprob_kwargs=None, track_scale=False, verbose=True)
    assert {k: v.default for k, v in sig.parameters.items() if k != 'self'} == want
    Y, Ye, Ym = case_models(g, 'f')
    gng = net.GrowingNeuralGas(Y, Ye, Ym)
    gng.train_network(rstate=np.random.RandomState(SEED['f']), lprob_func=lp_foreign, **KW['f'])
    err = capsys.readouterr().err
    last = err.rstrip('\n').split('\r')[-1]
    assert last == 'Iteration 30/30 [nodes=%d, edges pruned=%d] ' % (g['f_nnode'][-1], g['f_nprune'][-1])
    check_network(gng, g, 'f')


def test_graph_init_label_collision_is_refused(g):
    Y, Ye, Ym = case_models(g, 'e')
    graph = FakeGraph()
    for n in (0, 1, 7):                                                   # 3 nodes: the insertions would be labelled 3, 4, 5, 6, 7, ...
        graph.add_node(n, pos=Y[n + 10].copy(), error=0.)
    graph.add_edge(0, 1, age=0); graph.add_edge(1, 7, age=0)
    gng = net.GrowingNeuralGas(Y, Ye, Ym)
    with pytest.raises(ValueError, match='already in the graph'):
        next(gng._train_network(Y, Ye, Ym, rstate=np.random.RandomState(1), lprob_func=lp_foreign, graph_init=graph, niter=10, nbatch=5))


def test_fitting_exports_the_four_classes():
    from frankenz_amd import fitting
    assert fitting.__all__ == ["BruteForce", "NearestNeighbors", "SelfOrganizingMap", "GrowingNeuralGas"]
    assert fitting.GrowingNeuralGas is net.GrowingNeuralGas and fitting.SelfOrganizingMap is net.SelfOrganizingMap
    assert issubclass(net.GrowingNeuralGas, net.Network)
    assert net._GNG_MAX_DEGREE == 64
