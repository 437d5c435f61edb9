"""GrowingNeuralGas.train_network on the device (fz_gng_train) against G17, the reference's own training runs
(tests/golden/make_golden_gng.py): the BMU of every step, NNODE and nprune of every batch, the final labels, adjacency order and
ages (equal), positions and errors (rtol 1e-9: chi2 may round differently from NumPy's sums), the caller's cleaned and aliased
rows; segmenting; the global-memory form; the degree limit; refusals; and a trained network end to end through
populate_network / fit_predict against the oracle."""
import hashlib
import os
import sys

import numpy as np
import pytest

from frankenz_amd import networks as net
from frankenz_amd.networks import GrowingNeuralGas
from conftest import EVID64
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gng_host import (G17, KW, SEED, FakeGraph, case_kwargs, case_models, check_graph, check_network, check_steps,  # noqa: E402
                           expected_arrays, init_graph, numpy_logprob, run_steps, som_models)

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.gpu
RTOL = 1e-9


@pytest.fixture(scope='module')
def g():
    return dict(np.load(G17))


@pytest.fixture(scope='module')
def trained_g(g):
    """case g (the default size) trained once: (network, steps, models as left by the training)"""
    Y, Ye, Ym = case_models(g, 'g')
    gng = GrowingNeuralGas(Y, Ye, Ym)
    steps = run_steps(gng, Y, Ye, Ym, int(g['g_seed']))
    return gng, steps, (Y, Ye, Ym)


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd', 'e', 'h'])
def test_cases_against_g17(g, tag):
    Y, Ye, Ym = case_models(g, tag)
    Y0, Ye0, Ym0 = Y.copy(), Ye.copy(), Ym.copy()
    kw = case_kwargs(g, tag)
    graph0 = None
    if tag == 'e':
        graph0 = kw['graph_init'] = init_graph(g)
    gng = GrowingNeuralGas(Y, Ye, Ym)
    steps = run_steps(gng, Y, Ye, Ym, SEED[tag], **kw)
    check_steps(steps, g, tag, kw['nbatch'])
    check_network(gng, g, tag, exact=False, rtol=RTOL)
    want = expected_arrays(g, tag, Y0, Ye0, Ym0)
    if len(g[tag + '_init']):
        # the two rows the initial nodes are views of hold the nodes' positions (or their last ones), the rest is equal
        np.testing.assert_allclose(Y[g[tag + '_init']], g[tag + '_rows_after'], rtol=RTOL)
        want[0][g[tag + '_init']] = Y[g[tag + '_init']]
    for got, w in zip((Y, Ye, Ym), want):
        np.testing.assert_array_equal(got, w)
    if graph0 is not None:
        assert gng.graph is graph0
    if gng.graph is not None:
        check_graph(gng.graph, gng, g, tag)


@pytest.mark.parametrize('tag', ['b', 'c'])
def test_segments_give_identical_bits(g, monkeypatch, tag):
    """1, 7 and 1 000 kernel launches: the same BMUs, structure, positions and errors, bit for bit"""
    kw = case_kwargs(g, tag)
    T = kw['niter'] * kw['nbatch']
    runs = []
    for nseg in (1, 7, 1000):
        monkeypatch.setattr(net, '_GNG_SEGMENT', -(-T // nseg))
        Y, Ye, Ym = case_models(g, tag)
        gng = GrowingNeuralGas(Y, Ye, Ym)
        steps = run_steps(gng, Y, Ye, Ym, SEED[tag], **kw)
        runs.append((steps, gng.graph_ids, gng.graph_pos, gng.graph_errors, gng.nodes, gng.graph_adj_off, gng.graph_adj_nbr,
                     gng.graph_adj_age, Y))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a, b)
    check_steps(runs[0][0], g, tag, kw['nbatch'])


def test_global_memory_form_against_the_host_loop():
    """1 100 nodes x 32 bands do not fit LDS: the nodes stay in global memory.  Against the package's host loop with the NumPy
    likelihood (tests/test_gng_host.py holds that loop to the reference bit for bit); the BMU decisions of the run are checked to
    be further apart than rounding first."""
    kw = dict(niter=1150, nbatch=1, max_nodes=1100, max_age=12)
    Y, Ye, Ym = som_models(181, 1500, 32, 'err')
    Yh, Yeh, Ymh = Y.copy(), Ye.copy(), Ym.copy()
    ref = GrowingNeuralGas(Yh, Yeh, Ymh)
    gap, want = np.inf, []
    for res, bmu, nn, npr in ref._train_network(Yh, Yeh, Ymh, rstate=np.random.RandomState(1801), lprob_func=numpy_logprob, **kw):
        lp = np.asarray(res[2])
        top = np.sort(lp)[-3:]
        gap = min(gap, np.min(np.diff(top)) / max(1., abs(top[-1])))
        want.append((bmu, nn, npr))
    assert gap > 1e-9
    assert ref.NNODE == 1100
    gng = GrowingNeuralGas(Y, Ye, Ym)
    steps = run_steps(gng, Y, Ye, Ym, 1801, **kw)
    np.testing.assert_array_equal(steps, np.array(want))
    for name in ('graph_ids', 'graph_adj_off', 'graph_adj_nbr', 'graph_adj_age'):
        np.testing.assert_array_equal(getattr(gng, name), getattr(ref, name))
    np.testing.assert_allclose(gng.graph_pos, ref.graph_pos, rtol=RTOL)
    np.testing.assert_allclose(gng.graph_errors, ref.graph_errors, rtol=RTOL)
    np.testing.assert_array_equal(Ye, Yeh)
    np.testing.assert_allclose(Y, Yh, rtol=RTOL)


def test_degree_overflow_is_refused_loudly(g, monkeypatch):
    monkeypatch.setattr(net, '_GNG_MAX_DEGREE', 2)
    Y, Ye, Ym = case_models(g, 'a')
    gng = GrowingNeuralGas(Y, Ye, Ym)
    with pytest.raises(RuntimeError, match='more than 2 neighbours'):
        gng.train_network(rstate=np.random.RandomState(SEED['a']), verbose=False, **KW['a'])


def test_refusals(g):
    Y, Ye, Ym = som_models(182, 50, 33, False)
    with pytest.raises(NotImplementedError, match='33 bands'):
        GrowingNeuralGas(Y, Ye, Ym).train_network(niter=2, nbatch=2, verbose=False)
    Y, Ye, Ym = case_models(g, 'a')
    rs = np.random.RandomState(3)
    state = rs.get_state()
    with pytest.raises(NotImplementedError, match='at most 65536'):
        GrowingNeuralGas(Y, Ye, Ym).train_network(niter=2, nbatch=2, max_nodes=65537, rstate=rs, verbose=False)
    assert all(np.array_equal(a, b) for a, b in zip(state, rs.get_state()))      # refused before anything was drawn
    with pytest.raises(ValueError, match='track_scale'):
        GrowingNeuralGas(Y, Ye, Ym).train_network(niter=2, nbatch=2, track_scale=True, verbose=False)
    clash = FakeGraph()
    for n in (0, 1, 5):                                                   # 3 nodes: the insertions would be labelled 3, 4, 5
        clash.add_node(n, pos=Y[n + 10].copy(), error=0.)
    clash.add_edge(0, 1, age=0); clash.add_edge(1, 5, age=0)
    with pytest.raises(ValueError, match='already in the graph'):
        GrowingNeuralGas(Y, Ye, Ym).train_network(niter=3, nbatch=2, graph_init=clash, verbose=False)
    # the C entry point's own limits
    from frankenz_amd.engine import get_engine, like_opts
    eng = get_engine(None)
    X = np.ones((4, 5)); dr = np.zeros(4, dtype=np.int64)
    opts = like_opts({'free_scale': True, 'ignore_model_err': True})

    def call(cap=4, md=4, B=5, max_nodes=4):
        x = np.ones((4, B))
        nf, ni = net._gng_state_sizes(cap, B, md, 8, 32)
        ist = np.zeros(ni, dtype=np.int32); ist[0] = 2
        eng.gng_train(x, x, x, dr, np.zeros(nf), ist, np.zeros(cap, dtype=np.int64), cap, md, 8, 32, 2, 15, max_nodes, 2, .2, .005, .5, .995,
                      opts, False, -1, -1, 0, 4, np.zeros(4, dtype=np.int64), np.zeros((2, 2), dtype=np.int32))
    with pytest.raises(NotImplementedError, match='degree limit'):
        call(md=65)
    with pytest.raises(NotImplementedError, match='degree limit'):
        call(md=1)
    with pytest.raises(ValueError, match='max_nodes'):
        call(max_nodes=5)
    with pytest.raises(NotImplementedError, match='bands'):
        call(B=33)


def test_full_size_against_g17(g, trained_g):
    """the reference's defaults (niter 5000 x nbatch 50, max_nodes 2500) on 20 000 models"""
    gng, steps, (Y, Ye, Ym) = trained_g
    assert hashlib.sha1(steps[:, 0].astype(np.int64).tobytes()).digest() == g['g_bmus_sha1'].tobytes()
    np.testing.assert_array_equal(steps[::50, 1], g['g_nnode'])
    np.testing.assert_array_equal(steps[::50, 2], g['g_nprune'])
    check_network(gng, g, 'g', exact=False, rtol=RTOL)
    np.testing.assert_allclose(Y[g['g_init']], g['g_rows_after'], rtol=RTOL)


def test_trained_network_end_to_end_against_the_oracle(g, trained_g):
    """train_network -> populate_network -> fit_predict on the full-size network (G17-g's, to rounding) equals the oracle applied to
    the same nodes"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
    import frankenz_oracle as fo
    from frankenz_amd import PDFDict
    gng, _, (Y, Ye, Ym) = trained_g
    M, N = 2000, 200
    keep = np.setdiff1d(np.arange(M + 2), g['g_init'])[:M]            # (not the two rows the training rewrote)
    Ys, Yes, Yms = [np.ascontiguousarray(a[keep]).copy() for a in (Y, Ye, Ym)]
    rs = np.random.RandomState(17)
    z, ze = rs.uniform(0, 6, M), np.full(M, 0.05)
    okm = np.isfinite(Ys).all(axis=1) & np.isfinite(Yes).all(axis=1) & (Yes > 0).all(axis=1)
    X = Ys[okm][rs.choice(okm.sum(), N)] * rs.lognormal(0, .2, (N, 1)); Xe = 0.1 * X; Xm = np.ones_like(X)
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    od = fo.KernelDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    small = GrowingNeuralGas(Ys, Yes, Yms)
    np.testing.assert_allclose(gng.nodes, g['g_pos'], rtol=RTOL)
    small.set_nodes(gng.nodes)
    small.populate_network(verbose=False)
    with np.errstate(all='ignore'):
        p, (lm, le) = small.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=pd, return_gof=True, verbose=False)
        onet = fo.populate_network(gng.nodes, Ys.copy(), Yes.copy(), Yms.copy())
        rp, rlm, rle, _ = fo.network_fit_predict(onet, gng.nodes, X.copy(), Xe.copy(), Xm.copy(), Ys, Yes, Yms, z, ze, label_dict=od)
    np.testing.assert_array_equal(small.nodes_Nmatch, onet['Nmatch'])
    np.testing.assert_allclose(p, rp, rtol=1e-8, atol=1e-14)
    np.testing.assert_allclose(lm, rlm, rtol=1e-8)
    np.testing.assert_allclose(le, rle, **EVID64)
