"""SelfOrganizingMap.train_network on the device (fz_som_train) against G15, the reference's own training runs
(tests/golden/make_golden_som.py): the BMU of every step, the final nodes, the cleaned caller arrays, nodes_init trained in place;
segmenting; refusals; and the trained map end to end through populate_network / fit_predict against the oracle."""
import math
import os
import sys

import numpy as np
import pytest

from frankenz_amd import networks as net
from frankenz_amd.networks import SelfOrganizingMap
from conftest import EVID64
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_som_host import case_models, expected_cleaned, restated_training, som_models  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
G15 = os.path.join(HERE, 'golden', 'g15_som_train.npz')
pytestmark = pytest.mark.gpu

KW = {
    'a': dict(nside=8, nproj=2, niter=40, nbatch=25),
    'b': dict(nside=5, nproj=3, niter=40, nbatch=25, neighbor_func=net.neighbor_lorentz, learn_func=net.learn_geometric,
              learn_kwargs={'start': .8, 'end': .05}, wt_thresh=1e-2),
    'c': dict(nside=8, nproj=2, niter=40, nbatch=25, wt_thresh=None, cdf_thresh=0.01),
    'd': dict(nside=6, nproj=2, niter=40, nbatch=25, track_scale=True,
              lprob_kwargs={'free_scale': True, 'ignore_model_err': True, 'return_scale': True}),
    'e': dict(nside=8, nproj=2, niter=40, nbatch=25, lprob_kwargs={'free_scale': False, 'ignore_model_err': False}),
    'f': dict(nside=4, nproj=2, niter=10, nbatch=10),
}
SEED = {'a': 1501, 'b': 1502, 'c': 1503, 'd': 1504, 'e': 1505, 'f': 1506, 'g': 1507}


def lp_foreign(x, xe, xm, y, ye, ym, *args, **kwargs):
    chi2 = np.sum(xm * (x - y)**2 / xe**2, axis=1)
    lnl = -0.5 * chi2
    return np.zeros_like(lnl), lnl, lnl, np.sum(xm * ym, axis=1), chi2


@pytest.fixture(scope='module')
def g():
    return dict(np.load(G15))


def inputs(g, tag):
    return case_models(g, tag)


def train(Y, Ye, Ym, seed, **kw):
    """train_network, and the BMUs of the same run from the _train_network generator"""
    som = SelfOrganizingMap(Y, Ye, Ym)
    som.train_network(rstate=np.random.RandomState(seed), verbose=False, **kw)
    return som


def steps_of(Y, Ye, Ym, seed, **kw):
    """(node_results, bmu) of every step of the _train_network generator"""
    som = SelfOrganizingMap(Y, Ye, Ym)
    ek = kw.pop('err_kernel', None)
    if ek is not None:
        Ye = np.sqrt(Ye**2 + ek**2)
    steps = [(r[0], r[1]) for r in som._train_network(Y, Ye, Ym, rstate=np.random.RandomState(seed), **kw)]
    return [r[0] for r in steps], np.array([r[1] for r in steps])


def bmus_of(Y, Ye, Ym, seed, **kw):
    return steps_of(Y, Ye, Ym, seed, **kw)[1]


@pytest.mark.parametrize('tag', list('abcdef'))
def test_cases_against_g15(g, tag):
    kw = dict(KW[tag])
    if tag == 'e':
        kw['err_kernel'] = np.full((2000, 5), float(g['e_err_kernel']))
    if tag == 'f':
        kw['lprob_func'] = lp_foreign
    init = g['d_init'].copy() if tag == 'd' else None
    Y, Ye, Ym = inputs(g, tag)
    with np.errstate(all='ignore'):
        som = train(Y, Ye, Ym, SEED[tag], nodes_init=init, **kw)
    np.testing.assert_allclose(som.nodes, g[tag + '_nodes'], rtol=1e-9)
    np.testing.assert_array_equal(som.nodes_pos, g[tag + '_nodes_pos'])
    assert (som.NSIDE, som.NNODE, som.NPROJ, som.NITER, som.NBATCH) == (kw['nside'], kw['nside']**kw['nproj'], kw['nproj'],
                                                                          kw['niter'], kw['nbatch'])
    if tag in 'ae':
        for mine, ref in zip((Y, Ye, Ym), expected_cleaned(g, tag, *inputs(g, tag))):
            np.testing.assert_array_equal(mine, ref)
    if tag == 'd':
        assert som.nodes is init
        np.testing.assert_allclose(init, g['d_init_after'], rtol=1e-9)
    init = g['d_init'].copy() if tag == 'd' else None
    with np.errstate(all='ignore'):
        fits, b = steps_of(*inputs(g, tag), SEED[tag], nodes_init=init, **kw)
    np.testing.assert_array_equal(b, g[tag + '_bmus'])
    # a-e run on the device (no per-step likelihood rows); f's foreign likelihood runs on the host and yields its results
    assert all((r is None) == (tag != 'f') for r in fits)


@pytest.fixture(scope='module')
def trained_g(g):
    Y, Ye, Ym = case_models(g, 'g')
    som = SelfOrganizingMap(Y, Ye, Ym)
    with np.errstate(all='ignore'):
        b = np.array([r[1] for r in som._train_network(Y, Ye, Ym, rstate=np.random.RandomState(1507))])
    return som, b, (Y, Ye, Ym)


def test_full_size_against_g15(g, trained_g):
    som, b, _ = trained_g
    assert som.NNODE == 2500 and len(b) == 100000
    np.testing.assert_array_equal(b, g['g_bmus'])
    np.testing.assert_allclose(som.nodes, g['g_nodes'], rtol=1e-8)


@pytest.mark.parametrize('nseg', [1, 7, 1000])
def test_segments_give_identical_nodes(g, monkeypatch, nseg):
    ref = None
    for n in (1, nseg):
        monkeypatch.setattr(net, '_SOM_SEGMENT', -(-1000 // n))
        with np.errstate(all='ignore'):
            som = train(*inputs(g, 'a'), SEED['a'], **KW['a'])
        if ref is None:
            ref = som.nodes.copy()
    np.testing.assert_array_equal(som.nodes, ref)


def test_cdf_ties_split_in_node_index_order(g):
    """a CDF threshold inside the neighbourhood: tie groups of equal weight straddle the boundary at most steps; the device splits
    them in node-index order, as a stable argsort does (tests/test_som_host.py's restatement with kind='stable')"""
    Y, Ye, Ym = inputs(g, 'c')
    kw = dict(KW['c'], cdf_thresh=0.3)
    with np.errstate(all='ignore'):
        som = train(Y.copy(), Ye.copy(), Ym.copy(), SEED['c'], **kw)
        b = bmus_of(Y.copy(), Ye.copy(), Ym.copy(), SEED['c'], **kw)
        nodes, rb, _, _ = restated_training(Y, Ye, Ym, SEED['c'], 8, 2, 'gauss', 'harmonic', {}, None, 0.3,
                                            {'free_scale': True, 'ignore_model_err': True}, False)
    np.testing.assert_array_equal(b, rb)
    np.testing.assert_allclose(som.nodes, nodes, rtol=1e-9)


@pytest.mark.parametrize('B,nside,wt_thresh,cdf_thresh', [(5, 40, None, 0.3), (32, 30, 1e-3, 2e-4), (32, 40, None, 0.3),
                                                          (5, 8, None, 1.5)])
def test_large_maps_and_cdf_edges_against_the_restatement(B, nside, wt_thresh, cdf_thresh):
    """maps past one wave and past LDS against tests/test_som_host.py's restatement (ties in node-index order):
    1 600 nodes x 5 bands (LDS form; 16 waves and two passes of nodes per thread: the cross-wave scan of the CDF rule and the
    rank of a straddling tie group across waves and passes), 900 and 1 600 nodes x 32 bands (230 / 410 KB: the global-memory
    form), and cdf_thresh > 1, where no running probability fits and no node moves"""
    Y, Ye, Ym = som_models(160 + B, 3000, B, bad='err')
    kw = dict(nside=nside, nproj=2, niter=10, nbatch=20, wt_thresh=wt_thresh, cdf_thresh=cdf_thresh)
    with np.errstate(all='ignore'):
        som = train(Y.copy(), Ye.copy(), Ym.copy(), 16, **kw)
        b = bmus_of(Y.copy(), Ye.copy(), Ym.copy(), 16, **kw)
        nodes, rb, _, _ = restated_training(Y, Ye, Ym, 16, nside, 2, 'gauss', 'harmonic', {}, wt_thresh, cdf_thresh,
                                            {'free_scale': True, 'ignore_model_err': True}, False, niter=10, nbatch=20)
    np.testing.assert_array_equal(b, rb)
    np.testing.assert_allclose(som.nodes, nodes, rtol=1e-9)
    if cdf_thresh > 1:
        rs = np.random.RandomState(16)
        np.testing.assert_array_equal(som.nodes, Y[rs.choice(3000, size=nside**2, replace=False)])


def test_refusals(g):
    from frankenz_amd.engine import get_engine, like_opts
    eng = get_engine(None)
    Y, Ye, Ym = inputs(g, 'a')
    som = SelfOrganizingMap(Y, Ye, Ym)
    with pytest.raises(ValueError, match='return_scale'):
        som.train_network(nside=4, niter=2, nbatch=2, track_scale=True, verbose=False)
    with pytest.raises(ValueError, match='nodes_init'):
        som.train_network(nside=4, niter=2, nbatch=2, nodes_init=np.ones((15, 5)), verbose=False)
    with pytest.raises(ValueError, match='rate'):
        som.train_network(nside=4, niter=2, nbatch=2, neighbor_kwargs={'rate': 'cubic'}, verbose=False)
    opts = like_opts({'free_scale': True})
    pos = np.ascontiguousarray(net.som_nodes_pos(4, 2), dtype=np.int32)
    tab = lambda: (np.zeros(4, dtype=np.int64), np.full(4, .5), np.full(4, 2.), np.zeros(4, dtype=np.int32))
    X = np.ones((10, 33)); nodes = np.ones((16, 33))
    with pytest.raises(NotImplementedError, match='bands'):
        eng.som_train(X, X, X, nodes, pos, *tab()[:3], 0, True, 1e-3, .5, opts, False, 0, 4, tab()[3])
    X = np.ones((10, 5)); nodes = np.ones((16, 5))
    with pytest.raises(ValueError, match='neighbour kind'):
        eng.som_train(X, X, X, nodes, pos, *tab()[:3], 7, True, 1e-3, .5, opts, False, 0, 4, tab()[3])
    d = tab(); d[0][2] = 10
    with pytest.raises(IndexError, match='drawn row'):
        eng.som_train(X, X, X, nodes, pos, *d[:3], 0, True, 1e-3, .5, opts, False, 0, 4, d[3])
    big = np.zeros(((1 << 22) + 1, 1), dtype=np.int32)
    with pytest.raises(NotImplementedError, match='nodes'):
        eng.som_train(X, X, X, nodes, big, *tab()[:3], 0, True, 1e-3, .5, opts, False, 0, 4, tab()[3])


def test_trained_map_end_to_end_against_the_oracle(g, trained_g):
    """train_network -> populate_network -> fit_predict on the full-size map equals the oracle applied to G15-g's nodes"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'oracle'))
    import frankenz_oracle as fo
    from frankenz_amd import PDFDict
    som, _, (Y, Ye, Ym) = trained_g
    M, N = 2000, 200
    Ys, Yes, Yms = [np.ascontiguousarray(a[:M]) for a in (Y, Ye, Ym)]
    Ys, Yes, Yms = Ys.copy(), Yes.copy(), Yms.copy()
    rs = np.random.RandomState(15)
    z, ze = rs.uniform(0, 6, M), np.full(M, 0.05)
    okm = np.isfinite(Ys).all(axis=1) & np.isfinite(Yes).all(axis=1) & (Yes > 0).all(axis=1)
    X = Ys[okm][rs.choice(okm.sum(), N)] * rs.lognormal(0, .2, (N, 1)); Xe = 0.1 * X; Xm = np.ones_like(X)
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    od = fo.KernelDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    small = SelfOrganizingMap(Ys, Yes, Yms)
    small.set_nodes(som.nodes, som.nodes_pos)
    small.populate_network(verbose=False)
    with np.errstate(all='ignore'):
        p, (lm, le) = small.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=pd, return_gof=True, verbose=False)
        onet = fo.populate_network(g['g_nodes'], Ys.copy(), Yes.copy(), Yms.copy())
        rp, rlm, rle, _ = fo.network_fit_predict(onet, g['g_nodes'], X.copy(), Xe.copy(), Xm.copy(), Ys, Yes, Yms, z, ze, label_dict=od)
    np.testing.assert_array_equal(small.nodes_Nmatch, onet['Nmatch'])
    np.testing.assert_allclose(p, rp, rtol=1e-8, atol=1e-14)
    np.testing.assert_allclose(lm, rlm, rtol=1e-8)
    np.testing.assert_allclose(le, rle, **EVID64)
    npdf, _ = small.get_pdfs(z, ze, label_dict=pd, return_gof=True, verbose=False)
    rnp, _, _ = fo.network_node_pdfs(onet, z, ze, label_dict=od)
    np.testing.assert_allclose(npdf, rnp, rtol=1e-8, atol=1e-300)
