"""Inference through a trained network: frankenz_amd.networks.Network against golden G14, generated from the reference's
_Network with hand-set nodes (networks.py:244-356, 413-560, 782-936, 938-1128, 1130-1473), and against the oracle on a larger case."""
import functools

import numpy as np
import pytest

import _net_ref as nr
import frankenz_oracle as fo
from conftest import load_golden

pytestmark = pytest.mark.gpu


def eq(a, b, rtol=1e-9, atol=1e-11):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def dicts():
    from frankenz_amd import PDFDict
    grid, sg = np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500)
    return PDFDict(grid, sg), fo.KernelDict(grid, sg)


def make_net(g, **kw):
    from frankenz_amd.networks import Network
    net = Network(g['models'].copy(), g['models_err'].copy(), g['models_mask'].copy())
    net.set_nodes(g['nodes'])
    net.populate_network(verbose=False, **kw)
    return net


def cat(lst, dt):
    return np.concatenate([np.asarray(v, dtype=dt) for v in lst])


@pytest.mark.parametrize('rule', ['wt', 'cdf'])
@pytest.mark.parametrize('nodes_only', [0, 1])
@pytest.mark.parametrize('disc', [0, 1])
def test_g14_fit_predict_through_the_network(rule, nodes_only, disc):
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    net = make_net(g)
    np.testing.assert_array_equal(net.nodes_Nmatch, g['Nmatch'])
    rk = dict(wt_thresh=1e-3) if rule == 'wt' else dict(wt_thresh=None, cdf_thresh=0.05)
    tag = '%s_n%d_d%d' % (rule, nodes_only, disc)
    X, Xe, Xm = g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy()
    with np.errstate(all='ignore'):
        pdfs, (lm, le) = net.fit_predict(X, Xe, Xm, g['labels'], g['label_errs'], label_dict=d, nodes_only=bool(nodes_only), discrete=bool(disc),
                                         return_gof=True, verbose=False, save_fits=True, track_scale=bool(nodes_only), **rk)
    np.testing.assert_array_equal(net.Nneighbors, g[tag + '_Nneighbors'])
    np.testing.assert_array_equal(cat(net.neighbors, 'int'), g[tag + '_neighbors'])       # the reference's order (pandas.unique / argsort)
    eq(cat(net.fit_lnprob, 'float'), g[tag + '_lnprob']); eq(cat(net.fit_chi2, 'float'), g[tag + '_chi2'])
    np.testing.assert_array_equal(cat(net.fit_Ndim, 'int'), g[tag + '_Ndim'])
    if nodes_only:
        eq(cat(net.fit_scale, 'float'), g[tag + '_scale'])
    eq(lm, g[tag + '_lmap']); eq(le, g[tag + '_levid'])
    eq(pdfs, g[tag + '_pdfs'], rtol=1e-8, atol=1e-14)
    # predict() from the stored fits; fit() alone stores the same
    with np.errstate(all='ignore'):
        p2, (lm2, le2) = net.predict(g['labels'], g['label_errs'], label_dict=d, return_gof=True, discrete=bool(disc), verbose=False)
    eq(p2, g[tag + '_pdfs_predict'], rtol=1e-8, atol=1e-14); eq(lm2, g[tag + '_lmap']); eq(le2, g[tag + '_levid'])
    net.fit(g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy(), nodes_only=bool(nodes_only), discrete=bool(disc), verbose=False,
            track_scale=bool(nodes_only), **rk)
    np.testing.assert_array_equal(cat(net.neighbors, 'int'), g[tag + '_neighbors'])
    eq(cat(net.fit_lnprob, 'float'), g[tag + '_lnprob'])
    # the in-place clean of the objects reached the caller's arrays (pdf.py:309-311)
    assert X[2, 3] == 0.0 and Xe[2, 3] == 1.0 and Xm[2, 3] == 0.0


@pytest.mark.parametrize('disc', [0, 1])
def test_g14_node_pdfs(disc):
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    net = make_net(g)
    p, (lm, le) = net.get_pdfs(g['labels'], g['label_errs'], label_dict=d, return_gof=True, discrete=bool(disc), verbose=False)
    eq(p, g['nodepdfs_d%d' % disc], rtol=1e-8, atol=1e-14); eq(lm, g['nodelmap_d%d' % disc]); eq(le, g['nodelevid_d%d' % disc])
    p1, gof = net.get_pdf(3, g['labels'], g['label_errs'], label_dict=d, return_gof=True, discrete=bool(disc))
    eq(p1, g['nodepdfs_d%d' % disc][3], rtol=1e-8, atol=1e-14)


@pytest.mark.parametrize('nodes_only', [0, 1])
def test_g14_nodes_without_models_are_left_out(nodes_only):
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    net = make_net(g, track_scale=False, lpnet_kwargs={'free_scale': False, 'ignore_model_err': True})
    np.testing.assert_array_equal(net.nodes_Nmatch, g['fx_Nmatch'])
    tag = 'fx_n%d' % nodes_only
    with np.errstate(all='ignore'):
        pdfs, (lm, le) = net.fit_predict(g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy(), g['labels'], g['label_errs'],
                                         label_dict=d, nodes_only=bool(nodes_only), return_gof=True, verbose=False)
    np.testing.assert_array_equal(cat(net.neighbors, 'int'), g[tag + '_neighbors'])
    eq(cat(net.fit_lnprob, 'float'), g[tag + '_lnprob']); eq(lm, g[tag + '_lmap']); eq(le, g[tag + '_levid'])
    eq(pdfs, g[tag + '_pdfs'], rtol=1e-8, atol=1e-14)


def test_g14_grid_kde_and_generators():
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    net = make_net(g)
    with np.errstate(all='ignore'):
        pdfs, (lm, le) = net.fit_predict(g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy(), g['labels'], g['label_errs'],
                                         label_grid=d.grid, return_gof=True, verbose=False)
        gen = list(net._fit_predict(g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy(), g['labels'], g['label_errs'], label_grid=d.grid))
    eq(pdfs, g['grid_pdfs'], rtol=1e-8, atol=1e-14); eq(lm, g['grid_lmap']); eq(le, g['grid_levid'])
    eq(np.array([r[0] for r in gen]), g['grid_pdfs'], rtol=1e-8, atol=1e-14)
    with pytest.raises(ValueError):
        net.fit_predict(g['data'], g['data_err'], g['data_mask'], g['labels'], g['label_errs'])
    with pytest.raises(ValueError):
        net.get_node()


def test_user_callables_run_on_the_host_and_match_the_device_path():
    """a foreign lpnet_func / lprob_func (here: thin wrappers of the package's own logprob) goes through the host loops"""
    from frankenz_amd import pdf as fpdf
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    mine = lambda *a, **k: fpdf.logprob(*a, **k)
    net = make_net(g)
    net2 = make_net(g, lpnet_func=mine)
    np.testing.assert_array_equal(net.nodes_Nmatch, net2.nodes_Nmatch)
    for a, b in zip(net.nodes_idxs, net2.nodes_idxs):
        assert a == b
    args = (g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy(), g['labels'], g['label_errs'])
    with np.errstate(all='ignore'):
        p0 = net.fit_predict(*[np.copy(a) for a in args], label_dict=d, verbose=False)
        p1 = net2.fit_predict(*[np.copy(a) for a in args], label_dict=d, lprob_func=mine, verbose=False)
    eq(p0, p1, rtol=1e-9, atol=1e-14)
    np.testing.assert_array_equal(cat(net.neighbors, 'int'), cat(net2.neighbors, 'int'))


# ---- the host layer's own paths: chunk seams, the layout of the yielded tuples, save_fits, a foreign likelihood on a label grid ------
FIT_LISTS = ('neighbors', 'fit_lnprior', 'fit_lnlike', 'fit_lnprob', 'fit_Ndim', 'fit_chi2', 'fit_scale', 'fit_scale_err')


def g14_objects(g):
    return g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy()


def stored_and_pdfs(g, d):
    """what fit_predict (nodes_only 0 / 1) and fit leave on the network and return, on the G14 objects"""
    out = {}
    for call in ('fit_predict_n0', 'fit_predict_n1', 'fit'):
        net = make_net(g)
        with np.errstate(all='ignore'):
            if call == 'fit':
                net.fit(*g14_objects(g), verbose=False)
                got = {}
            else:
                nodes_only = call.endswith('1')
                pdfs, (lm, le) = net.fit_predict(*g14_objects(g), g['labels'], g['label_errs'], label_dict=d, nodes_only=nodes_only,
                                                 track_scale=nodes_only, save_fits=True, return_gof=True, verbose=False)
                got = dict(pdfs=pdfs, lmap=lm, levid=le)
        got['Nneighbors'] = net.Nneighbors
        for k in FIT_LISTS:
            got[k] = getattr(net, k)
        out[call] = got
    return out


def test_a_chunk_seam_inside_the_objects_changes_no_bit():
    """7 objects per device call: a seam inside the 14 objects of G14; 5: two seams and a short last chunk of 4.  The stored fits and
    the PDFs are those of one chunk, bit for bit"""
    from frankenz_amd import networks
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    N = len(g['data'])
    assert N > 7 and N % 5 != 0
    whole = stored_and_pdfs(g, d)
    default = networks._NET_CHUNK
    cuts = []
    try:
        for chunk in (7, 5):
            networks._NET_CHUNK = chunk
            cuts.append(stored_and_pdfs(g, d))
    finally:
        networks._NET_CHUNK = default
    for cut, (call, want) in [(c, cw) for c in cuts for cw in whole.items()]:
        got = cut[call]
        assert got.keys() == want.keys()
        for k in want:
            if k in FIT_LISTS:
                assert len(got[k]) == len(want[k]) and len(want[k]) in (0, N), (call, k)
                for a, b in zip(got[k], want[k]):
                    np.testing.assert_array_equal(a, b, err_msg='%s %s' % (call, k))
            else:
                np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (call, k))
        assert len(want['fit_lnprob']) == N and (call != 'fit_predict_n1' or len(want['fit_scale']) == N)


def test_the_layout_of_the_yielded_tuples():
    """_fit yields (idxs, Nidx, results); results holds seven arrays where the likelihood was asked for the scale, else five
    (pdf.logprob's own rule), and with a foreign lprob_func it is the very tuple the user's function returned"""
    from frankenz_amd import pdf as fpdf
    g = load_golden('g14_network_inference')
    fixed = make_net(g, track_scale=False, lpnet_kwargs={'free_scale': False, 'ignore_model_err': True})
    cases = [(make_net(g), dict(lprob_kwargs={'free_scale': True, 'return_scale': True}), 7),
             (make_net(g), dict(), 5),
             (make_net(g), dict(nodes_only=True), 7),
             (fixed, dict(nodes_only=True), 5)]
    for net, kw, want in cases:
        with np.errstate(all='ignore'):
            res = list(net._fit(*g14_objects(g), **kw))
        assert len(res) == len(g['data'])
        for idxs, m, r in res:
            assert len(r) == want and len(idxs) == m and all(len(a) == m for a in r)
    made = []

    def mine(*a, **k):
        made.append(fpdf.logprob(*a, **k))
        return made[-1]
    with np.errstate(all='ignore'):
        res = list(make_net(g)._fit(*g14_objects(g), lprob_func=mine))
    assert len(res) == len(made) == len(g['data'])
    for r, m in zip(res, made):
        assert len(r) == 3 and r[2] is m


def test_save_fits_false_leaves_the_network_as_it_was():
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    net = make_net(g)
    with np.errstate(all='ignore'):
        res = list(net._fit_predict(*g14_objects(g), g['labels'], g['label_errs'], label_dict=d, save_fits=False))
    assert len(res) == len(g['data'])
    assert net.neighbors is None and net.Nneighbors is None
    for k in FIT_LISTS[1:]:
        assert getattr(net, k) is None, k


def test_a_foreign_lprob_func_on_a_label_grid_matches_the_device_path():
    """the union path with the user's likelihood: the PDFs come from knn_predict_logwt on the ln-posteriors it returned"""
    from frankenz_amd import pdf as fpdf
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    mine = lambda *a, **k: fpdf.logprob(*a, **k)
    net, net2 = make_net(g), make_net(g)
    args = g14_objects(g) + (g['labels'], g['label_errs'])
    with np.errstate(all='ignore'):
        p0, (lm0, le0) = net.fit_predict(*[np.copy(a) for a in args], label_grid=d.grid, return_gof=True, verbose=False)
        p1, (lm1, le1) = net2.fit_predict(*[np.copy(a) for a in args], label_grid=d.grid, lprob_func=mine, return_gof=True, verbose=False)
    eq(p0, p1, rtol=1e-9, atol=1e-14)
    eq(lm0, lm1); eq(le0, le1)
    np.testing.assert_array_equal(cat(net.neighbors, 'int'), cat(net2.neighbors, 'int'))


def test_a_larger_network_against_the_oracle():
    """2 000 models on 60 nodes, 300 objects (more than one wave's worth of nodes, unions of hundreds of models)"""
    from frankenz_amd.networks import Network
    d, od = dicts()
    rs = np.random.RandomState(8)
    M, N, Nn, B = 2000, 300, 60, 5
    sig = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
    Y = rs.lognormal(1., 1., size=(M, 1)) * rs.lognormal(0., .4, size=(M, B)) * 5; Ye = 0.05 * Y; Ym = np.ones((M, B))
    nodes = Y[rs.choice(M, Nn, replace=False)] * rs.lognormal(0, 0.05, size=(Nn, B))
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .3, N)[:, None] + sig * rs.randn(N, B); Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    net = Network(Y, Ye, Ym); net.set_nodes(nodes); net.populate_network(verbose=False)
    onet = fo.populate_network(nodes, Y.copy(), Ye.copy(), Ym.copy())
    np.testing.assert_array_equal(net.nodes_Nmatch, onet['Nmatch'])
    for kw in (dict(), dict(nodes_only=True), dict(discrete=True)):
        with np.errstate(all='ignore'):
            p, (lm, le) = net.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, return_gof=True, verbose=False, **kw)
            rp, rlm, rle, lists = fo.network_fit_predict(onet, nodes, X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
        np.testing.assert_array_equal(net.Nneighbors, [len(v) for v in lists['neighbors']])
        np.testing.assert_array_equal(cat(net.neighbors, 'int'), np.concatenate(lists['neighbors']))
        eq(lm, rlm); eq(le, rle); eq(p, rp, rtol=1e-8, atol=1e-14)


# ---- more than one wave's worth of matched nodes, both rules (the kernels themselves: tests/test_hip_net_kernels.py) -----------------
LPNET = {'free_scale': True, 'ignore_model_err': True, 'return_scale': True}
RULES = {'wt': dict(), 'cdf': dict(wt_thresh=None, cdf_thresh=0.05)}


@functools.lru_cache(maxsize=None)
def multiwave_case():
    """1 500 models on 150 nodes, 100 objects"""
    rs = np.random.RandomState(21)
    M, N, Nn, B = 1500, 100, 150, 5
    sig = np.array([0.873, 0.348, 0.418, 0.873, 3.476])
    Y = rs.lognormal(1., 1., size=(M, 1)) * rs.lognormal(0., .4, size=(M, B)) * 5; Ye = 0.05 * Y; Ym = np.ones((M, B))
    nodes = Y[rs.choice(M, Nn, replace=False)] * rs.lognormal(0, 0.05, size=(Nn, B))
    X = Y[rs.choice(M, N)] * rs.lognormal(0, .3, N)[:, None] + sig * rs.randn(N, B); Xe = np.tile(sig, (N, 1)); Xm = np.ones((N, B))
    z = rs.uniform(0, 6, M); ze = np.full(M, 0.05)
    return Y, Ye, Ym, nodes, X, Xe, Xm, z, ze


@functools.lru_cache(maxsize=None)
def multiwave_oracle(rule):
    Y, Ye, Ym, nodes, X, Xe, Xm, z, ze = multiwave_case()
    onet = fo.populate_network(nodes, Y.copy(), Ye.copy(), Ym.copy(), **RULES[rule])
    if rule == 'cdf':
        # the precondition of comparing selections under the CDF rule: no model's and no object's running probability lies within 1e-9
        # of 1 - cdf_thresh (the device's scan rounds differently from np.cumsum).  Every row, none left out.
        y = nodes; ym = np.ones_like(y, dtype='bool')
        gaps = [nr.select(fo.logprob(x, xe, xm, y, np.zeros_like(y), ym, **LPNET)[2], False, 0.0, 0.05)[1]
                for x, xe, xm in zip(Y.copy(), Ye.copy(), Ym.copy())]
        y = nodes[np.asarray(onet['Nmatch']) > 0]; ym = np.ones_like(y, dtype='bool')
        gaps += [nr.select(fo.logprob(x, xe, xm, y, np.zeros_like(y), ym, **LPNET)[2], False, 0.0, 0.05)[1]
                 for x, xe, xm in zip(X.copy(), Xe.copy(), Xm.copy())]
        assert len(gaps) == len(Y) + len(X) and min(gaps) > 1e-9, min(gaps)
    return onet


@pytest.mark.parametrize('rule', ['wt', 'cdf'])
def test_multiwave_populate_network(rule):
    from frankenz_amd.networks import Network
    Y, Ye, Ym, nodes, X, Xe, Xm, z, ze = multiwave_case()
    onet = multiwave_oracle(rule)
    net = Network(Y.copy(), Ye.copy(), Ym.copy()); net.set_nodes(nodes); net.populate_network(verbose=False, **RULES[rule])
    np.testing.assert_array_equal(net.nodes_Nmatch, onet['Nmatch'])
    assert (net.nodes_Nmatch > 0).sum() > 128                  # the objects' rows are longer than two 64-column chunks
    for a, b in zip(net.nodes_idxs, onet['idxs']):
        np.testing.assert_array_equal(np.asarray(a, dtype='int'), np.asarray(b, dtype='int'))
    for a, b in zip(net.nodes_bmus, onet['bmus']):
        np.testing.assert_array_equal(np.asarray(a, dtype='int'), np.asarray(b, dtype='int'))
    eq(net.models_lmap, onet['lmap']); eq(net.models_levid, onet['levid'])
    eq(cat(net.nodes_logwts, 'float'), cat(onet['logwts'], 'float'))


@pytest.mark.parametrize('rule', ['wt', 'cdf'])
@pytest.mark.parametrize('nodes_only', [0, 1])
def test_multiwave_fit_predict(rule, nodes_only):
    from frankenz_amd.networks import Network
    d, od = dicts()
    Y, Ye, Ym, nodes, X, Xe, Xm, z, ze = multiwave_case()
    onet = multiwave_oracle(rule)
    net = Network(Y.copy(), Ye.copy(), Ym.copy()); net.set_nodes(nodes); net.populate_network(verbose=False, **RULES[rule])
    kw = dict(nodes_only=bool(nodes_only), **RULES[rule])
    if rule == 'cdf' and not nodes_only:
        # the CDF rule keeps all but the few best nodes: their lists sum to far more than the union table holds, and the message
        # says that this limit, not the node limit, was hit; the best-matching-unit lists (one node per model) fit
        with pytest.raises(NotImplementedError, match='union table'):
            net.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, verbose=False, **kw)
        kw['discrete'] = True
    with np.errstate(all='ignore'):
        p, (lm, le) = net.fit_predict(X.copy(), Xe.copy(), Xm.copy(), z, ze, label_dict=d, return_gof=True, verbose=False, **kw)
        rp, rlm, rle, lists = fo.network_fit_predict(onet, nodes, X.copy(), Xe.copy(), Xm.copy(), Y, Ye, Ym, z, ze, label_dict=od, **kw)
    np.testing.assert_array_equal(net.Nneighbors, [len(v) for v in lists['neighbors']])
    np.testing.assert_array_equal(cat(net.neighbors, 'int'), np.concatenate(lists['neighbors']))
    eq(lm, rlm); eq(le, rle); eq(p, rp, rtol=1e-8, atol=1e-14)


def test_an_object_that_selects_no_node_is_refused():
    """a nan among an object's node ln-probabilities (here from the user's node likelihood) selects no node; the reference then fails
    in np.max of nothing.  Here the call is refused before any fit, with the object named, instead of fitting a union table padded
    with model 0 (docs/deviations.md)"""
    from frankenz_amd import pdf as fpdf
    g = load_golden('g14_network_inference')
    d, _ = dicts()
    X, Xe, Xm = g['data'].copy(), g['data_err'].copy(), g['data_mask'].copy()

    def mine(x, *a, **k):
        r = [np.array(v) for v in fpdf.logprob(x, *a, **k)]
        if np.array_equal(x, g['data'][4]):
            r[2][1] = np.nan
        return tuple(r)
    net = make_net(g, lpnet_func=mine)
    for kw in (dict(), dict(nodes_only=True), dict(wt_thresh=None, cdf_thresh=0.05)):
        with pytest.raises(ValueError, match=r'object 4 selects no node .*\(1 of %d objects' % len(X)):
            net.fit_predict(X.copy(), Xe.copy(), Xm.copy(), g['labels'], g['label_errs'], label_dict=d, verbose=False, **kw)
        with pytest.raises(ValueError, match='object 4 selects no node'):
            net.fit(X.copy(), Xe.copy(), Xm.copy(), verbose=False, **kw)
    net = make_net(g)
    with pytest.raises(ValueError, match=r'object 0 selects no node .*\(%d of %d objects' % (len(X), len(X))):
        net.fit(X.copy(), Xe.copy(), Xm.copy(), wt_thresh=1.0, verbose=False)               # strict > against the max: no node
