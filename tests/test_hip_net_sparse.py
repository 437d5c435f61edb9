"""``Network.fit_sparse`` (docs/network.md, "Sparse rows"): the fit through a trained network left as ``SparseFits`` rows over the union of
the selected nodes' lists.  On golden G14 against ``Network.fit`` (the reference-pinned path) matched by model index; on a network
whose lists overlap so much that ``Network.fit`` refuses it, against ``pdf.logprob`` on exactly the union; widths, refusals, the row
consumers, chunking and residency.

Golden G14 holds 15 nodes over 120 models; the cases that need 20 matched nodes, 319 or 4 097 models extend it: its models tiled with
a fixed jitter, its nodes plus jittered copies, populated as usual, then the lists set by hand (the lists are data)."""
import functools
import pickle

import numpy as np
import pytest

from conftest import EVID64, load_golden

pytestmark = pytest.mark.gpu

RULES = {'wt': dict(wt_thresh=1e-3), 'cdf': dict(wt_thresh=None, cdf_thresh=0.05)}
FREE = {'free_scale': True, 'ignore_model_err': True, 'return_scale': True}
# every mode like_opts takes: A, Ai, B, C (iterative), and the Gaussian form without the dimension prior
MODES = [({}, False), ({'ignore_model_err': True}, False), (FREE, True), ({'free_scale': True, 'return_scale': True}, True),
         ({'dim_prior': False}, False)]
PADS = dict(fit_lnprior=-np.inf, fit_lnlike=-np.inf, fit_lnprob=-np.inf, fit_Ndim=0, fit_chi2=np.inf, fit_scale=1.0, fit_scale_err=0.0)


def eq(a, b, rtol=1e-9, atol=1e-11):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol)


def engine():
    from frankenz_amd.engine import get_engine
    return get_engine(None)


def make_net(g):
    from frankenz_amd.networks import Network
    net = Network(g['models'].copy(), g['models_err'].copy(), g['models_mask'].copy())
    net.set_nodes(g['nodes'])
    net.populate_network(verbose=False)
    return net


def objects(g, reps=1):
    return tuple(np.tile(g[k], (reps, 1)) for k in ('data', 'data_err', 'data_mask'))


def extended_net(tiles, extra_nodes):
    """G14 extended: its models ``tiles`` times over with a fixed jitter, its nodes and ``extra_nodes`` jittered copies; populated"""
    from frankenz_amd.networks import Network
    g = load_golden('g14_network_inference')
    rs = np.random.RandomState(14)
    jit = rs.lognormal(0., 0.03, size=(tiles * len(g['models']), g['models'].shape[1]))
    Y, Ye, Ym = (np.tile(g[k], (tiles, 1)) for k in ('models', 'models_err', 'models_mask'))
    Y = Y * jit
    nodes = np.concatenate([g['nodes'], g['nodes'][:extra_nodes] * rs.lognormal(0., 0.03, size=(extra_nodes, Y.shape[1]))])
    net = Network(Y, Ye, Ym)
    net.set_nodes(nodes)
    net.populate_network(verbose=False)
    return g, net


def set_lists(net, lists):
    """the per-node lists as data; nodes beyond ``lists`` are left without a model"""
    lists = [list(v) for v in lists] + [[] for _ in range(net.NNODE - len(lists))]
    net.nodes_idxs = lists
    net.nodes_bmus = [list(v) for v in lists]
    net.nodes_Nmatch = np.array([len(v) for v in lists], dtype='int')


def check_paddings(sf, free):
    valid = np.arange(sf.NKEEP)[None, :] < np.asarray(sf.Nneighbors)[:, None]
    assert (sf.neighbors[~valid] == -99).all() and (sf.neighbors[valid] >= 0).all()
    for k, pad in PADS.items():
        a = getattr(sf, k)
        if k in ('fit_scale', 'fit_scale_err') and not free:
            assert a is None
            continue
        assert (a[~valid] == pad).all(), k
    assert (sf.fit_lnprior[valid] == 0.0).all()
    np.testing.assert_array_equal(sf.fit_lnprob, sf.fit_lnlike)


def check_evidence(sf):
    assert (sf.cover() == 1.0).all()
    np.testing.assert_array_equal(sf.lnkept, sf.levid)
    np.testing.assert_array_equal(sf.lmap, sf.fit_lnprob.max(axis=1))
    rows = sf.fit_lnprob.astype(np.longdouble)
    mx = rows.max(axis=1)
    ref = (mx + np.log(np.exp(rows - mx[:, None]).sum(axis=1))).astype(np.float64)
    np.testing.assert_allclose(sf.levid, ref, **EVID64)


@pytest.mark.parametrize('rule', ['wt', 'cdf'])
@pytest.mark.parametrize('disc', [0, 1])
def test_g14_rows_are_the_fit_matched_by_model(rule, disc):
    g = load_golden('g14_network_inference')
    net, ref = make_net(g), make_net(g)
    for kw, free in MODES:
        X, Xe, Xm = objects(g)
        before, frozen = dict(vars(net)), pickle.dumps(vars(net))
        with np.errstate(all='ignore'):
            sf = net.fit_sparse(X, Xe, Xm, lprob_kwargs=kw, track_scale=free, discrete=bool(disc), verbose=False, **RULES[rule])
            ref.fit(*objects(g), lprob_kwargs=kw, track_scale=free, discrete=bool(disc), verbose=False, **RULES[rule])
        # no attribute of the network is touched; the in-place clean of the objects reached the caller's arrays (pdf.py:309-311)
        assert vars(net).keys() == before.keys() and all(vars(net)[k] is before[k] for k in before)
        assert pickle.dumps(vars(net)) == frozen
        assert X[2, 3] == 0.0 and Xe[2, 3] == 1.0 and Xm[2, 3] == 0.0
        np.testing.assert_array_equal(sf.Nneighbors, ref.Nneighbors)
        assert sf.NKEEP == ref.Nneighbors.max() and sf.NMODEL == net.NMODEL and sf.neighbors.dtype == np.int64
        for i in range(len(X)):
            n = int(sf.Nneighbors[i])
            order = np.argsort(ref.neighbors[i], kind='stable')
            np.testing.assert_array_equal(sf.neighbors[i, :n], np.sort(ref.neighbors[i]))
            eq(sf.fit_lnprob[i, :n], np.asarray(ref.fit_lnprob[i])[order]); eq(sf.fit_lnlike[i, :n], np.asarray(ref.fit_lnlike[i])[order])
            eq(sf.fit_chi2[i, :n], np.asarray(ref.fit_chi2[i])[order])
            np.testing.assert_array_equal(sf.fit_Ndim[i, :n], np.asarray(ref.fit_Ndim[i])[order])
            if free:
                eq(sf.fit_scale[i, :n], np.asarray(ref.fit_scale[i])[order]); eq(sf.fit_scale_err[i, :n], np.asarray(ref.fit_scale_err[i])[order])
        check_paddings(sf, free)
        check_evidence(sf)
    # a fixed scale with track_scale: ones and zeros throughout, as ``fit`` leaves them
    sf = net.fit_sparse(*objects(g), track_scale=True, verbose=False, **RULES[rule])
    assert (sf.fit_scale == 1.0).all() and (sf.fit_scale_err == 0.0).all()


@functools.lru_cache(maxsize=None)
def overlap_case():
    """20 matched nodes, node c listing the models c .. c + 299: every object selects all of them (no threshold): 6 000 entries
    before repeats are removed, 319 after"""
    g, net = extended_net(3, 5)
    assert net.NNODE == 20 and net.NMODEL == 360
    set_lists(net, [np.arange(c, c + 300) for c in range(20)])
    return g, net


def test_the_overlapping_lists_the_dense_fit_refuses():
    from frankenz_amd import pdf as fpdf
    g, net = overlap_case()
    with pytest.raises(NotImplementedError, match='6000 models before repeats are removed'):
        net.fit(*objects(g), wt_thresh=None, cdf_thresh=None, verbose=False)
    for kw, free in (MODES[0], MODES[2]):
        X, Xe, Xm = objects(g)
        with np.errstate(all='ignore'):
            sf = net.fit_sparse(X, Xe, Xm, wt_thresh=None, cdf_thresh=None, lprob_kwargs=kw, track_scale=free, verbose=False)
        assert sf.NKEEP == 319 and (sf.Nneighbors == 319).all()
        np.testing.assert_array_equal(sf.neighbors, np.tile(np.arange(319), (len(X), 1)))
        ii = np.arange(319)
        for i in range(len(X)):
            with np.errstate(all='ignore'):
                r = fpdf.logprob(X[i], Xe[i], Xm[i], net.models[ii], net.models_err[ii], net.models_mask[ii], **kw)
            eq(sf.fit_lnprob[i], r[2]); eq(sf.fit_lnlike[i], r[1]); eq(sf.fit_chi2[i], r[4])
            np.testing.assert_array_equal(sf.fit_Ndim[i], r[3])
            if free:
                eq(sf.fit_scale[i], r[5]); eq(sf.fit_scale_err[i], r[6])
        check_paddings(sf, free)
        check_evidence(sf)


def test_width_at_the_limit_and_refusals():
    from frankenz_amd import pdf as fpdf
    g, net = extended_net(35, 0)
    assert net.NMODEL == 4200
    X, Xe, Xm = objects(g)
    set_lists(net, [np.arange(4096)])                           # one matched node listing 4 096 models: the widest row there is
    sf = net.fit_sparse(X[:3].copy(), Xe[:3].copy(), Xm[:3].copy(), wt_thresh=None, cdf_thresh=None, verbose=False)
    assert sf.NKEEP == 4096 and (sf.Nneighbors == 4096).all()
    np.testing.assert_array_equal(sf.neighbors[1], np.arange(4096))
    check_evidence(sf)
    set_lists(net, [np.arange(4000), np.arange(3999, 4097)])    # 4 098 entries, 4 097 different models
    with pytest.raises(NotImplementedError, match=r'object 0: .* 4097 different models.* 4096'):
        net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), wt_thresh=None, cdf_thresh=None, verbose=False)
    # an object that selects no node (strict > against the max), and one whose nodes list no model
    net = make_net(g)
    with pytest.raises(ValueError, match=r'object 0 selects no node .*\(%d of %d objects' % (len(X), len(X))):
        net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), wt_thresh=1.0, verbose=False)
    # ... in the very words of ``fit``: one expression matches both
    words = (r'^object 0 selects no node of the network \(%d of %d objects in this call do\): its node ln-probabilities hold a nan, or '
             r'none passes the threshold \(wt_thresh=1\.0, cdf_thresh=0\.0002\)$' % (len(X), len(X)))
    with pytest.raises(ValueError, match=words) as sparse:
        net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), wt_thresh=1.0, verbose=False)
    with pytest.raises(ValueError, match=words) as dense:
        net.fit(X.copy(), Xe.copy(), Xm.copy(), wt_thresh=1.0, verbose=False)
    assert str(sparse.value) == str(dense.value)
    net.nodes_bmus = [[] for _ in range(net.NNODE)]
    with pytest.raises(ValueError, match='object 0: the nodes it selects list no model'):
        net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), discrete=True, verbose=False)
    with pytest.raises(NotImplementedError, match='built-in likelihood'):
        net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), lprob_func=lambda *a, **k: fpdf.logprob(*a, **k), verbose=False)


@functools.lru_cache(maxsize=None)
def consumer_case():
    g = load_golden('g14_network_inference')
    net = make_net(g)
    with np.errstate(all='ignore'):
        sf = net.fit_sparse(*objects(g), lprob_kwargs=FREE, track_scale=True, verbose=False)
    return g, net, sf


def test_predict_is_the_network_predict():
    from frankenz_amd import PDFDict
    g, net, sf = consumer_case()
    d = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    ref = make_net(g)
    with np.errstate(all='ignore'):
        ref.fit(*objects(g), lprob_kwargs=FREE, verbose=False)
        want, (rlm, rle) = ref.predict(g['labels'], g['label_errs'], label_dict=d, return_gof=True, verbose=False)
        got, (lm, le) = sf.predict(g['labels'], g['label_errs'], label_dict=d, return_gof=True, verbose=False)
    eq(got, want, rtol=1e-8, atol=1e-14)          # the rows are summed in another order: not bit for bit
    eq(lm, rlm); eq(le, rle)


def test_row_consumers_are_the_row_functions():
    from frankenz_amd import pdf as fpdf
    g, net, sf = consumer_case()
    z, ze = g['labels'], g['label_errs']
    rows, nb, nn = sf.fit_lnprob, sf.neighbors, sf.Nneighbors

    def same(a, b):
        assert type(a) is type(b)
        for x, y in zip(a, b) if isinstance(a, tuple) else [(a, b)]:
            np.testing.assert_array_equal(x, y)

    with np.errstate(all='ignore'):
        same(sf.predict_quantiles(z, ze), fpdf.posterior_quantiles(rows, z, ze, (0.025, 0.16, 0.5, 0.84, 0.975), neighbors=nb, Nneighbors=nn))
        edges = np.linspace(0., 7., 36)
        same(sf.predict_bins(z, ze, edges), fpdf.posterior_bins(rows, z, ze, edges, neighbors=nb, Nneighbors=nn))
        pts = np.array([0.5, 1.0, 2.5])
        same(sf.predict_cdf(z, ze, pts), fpdf.posterior_cdf(rows, z, ze, pts, neighbors=nb, Nneighbors=nn))
        same(sf.moments(z, ze), fpdf.posterior_moments(rows, z, ze, neighbors=nb, Nneighbors=nn))
        same(sf.moments(z, ze, use_scale=True), fpdf.posterior_moments(rows, z, ze, scale=sf.fit_scale, neighbors=nb, Nneighbors=nn))
        mean, var, share = sf.predict_phot(net.models, net.models_err, net.models_mask)
    assert mean.shape == (sf.NDATA, net.NDIM) and np.isfinite(mean).all()
    S = 9
    idx, (lm, le) = sf.sample(S, rstate=np.random.RandomState(3), return_gof=True)
    want, wlm, wle = np.empty((sf.NDATA, S), dtype=np.int64), np.zeros(sf.NDATA), np.zeros(sf.NDATA)
    engine().draw_logwt(rows, S, want, key=sf.philox_key, neighbors=nb, nnbr=nn, lmap=wlm, levid=wle)
    np.testing.assert_array_equal(idx, want); np.testing.assert_array_equal(lm, wlm); np.testing.assert_array_equal(le, wle)
    for i in range(sf.NDATA):
        assert np.isin(idx[i], nb[i, :nn[i]]).all()
    np.testing.assert_array_equal(lm, sf.lmap)


def test_weight_sampler_and_weight_em_take_a_step():
    g, net, sf = consumer_case()
    M = sf.NMODEL
    s = sf.weight_sampler()
    assert s.NMODEL == M and s.W == sf.NKEEP
    s.run_mcmc(1, alpha=np.full(M, 0.5), thin=1, rstate=np.random.RandomState(2), verbose=False)
    w = np.asarray(s.samples[-1])
    assert w.shape == (M,) and np.isfinite(w).all()
    em = sf.weight_em()
    w1, lnp, counts = em.step(np.full(M, 1. / M))
    assert np.asarray(w1).shape == (M,) and np.isfinite(lnp) and abs(np.asarray(counts).sum() - sf.NDATA) < 1e-9


def test_chunking_and_residency_do_not_change_a_bit():
    """3 360 objects under a 1 MiB workspace limit: the selection no longer fits its share, so the fitting pass forms it again, four
    chunks in the counting pass and more in the fitting pass; at the default limit it is one chunk and the selection is kept"""
    g, net = overlap_case()
    X, Xe, Xm = objects(g, 240)
    X = X * np.random.RandomState(5).lognormal(0., 0.1, size=(len(X), 1))
    kw = dict(lprob_kwargs=FREE, track_scale=True, verbose=False)
    keys = ('neighbors', 'Nneighbors', 'lmap', 'levid', 'lnkept') + tuple(PADS)
    eng = engine()
    with np.errstate(all='ignore'):
        sf = net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), **kw)
        assert sf.NKEEP == sf.Nneighbors.max()
        before = eng.workspace_limit()
        assert before // 4 >= len(X) * (20 * 4 + 4) > (1 << 20) // 4
        eng.set_workspace_limit(1 << 20)
        try:
            small = net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), **kw)
        finally:
            eng.set_workspace_limit(before)
        res = net.fit_sparse(X.copy(), Xe.copy(), Xm.copy(), resident=True, **kw)
    for k in keys:
        np.testing.assert_array_equal(getattr(small, k), getattr(sf, k), err_msg=k)
    for k in ('neighbors', 'Nneighbors', 'fit_lnlike', 'fit_lnprob'):
        assert not isinstance(getattr(res, k), np.ndarray)
        np.testing.assert_array_equal(getattr(res, k).numpy(), getattr(sf, k), err_msg=k)
    for k in ('fit_lnprior', 'fit_Ndim', 'fit_chi2', 'fit_scale', 'fit_scale_err'):
        assert getattr(res, k) is None
    for k in ('lmap', 'levid', 'lnkept'):
        np.testing.assert_array_equal(getattr(res, k), getattr(sf, k), err_msg=k)
    # the resident rows are used in place by a consumer
    z, ze = np.linspace(0.1, 5., net.NMODEL), np.full(net.NMODEL, 0.05)
    with np.errstate(all='ignore'):
        np.testing.assert_array_equal(res.predict_quantiles(z, ze), sf.predict_quantiles(z, ze))
