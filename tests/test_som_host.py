"""SelfOrganizingMap training, host side (no GPU): the tables the device path is handed -- node grid positions, the draw stream,
learning rates and sigmas -- and a NumPy restatement of the reference's step loop, all against G15 (tests/golden/g15_som_train.npz,
made by tests/golden/make_golden_som.py from the reference)."""
import math
import os

import numpy as np
import pytest

from frankenz_amd import networks as net

G15 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g15_som_train.npz')
CASES = {   # tag: (models seed, rstate seed, nside, nproj, neighbour, learn, learn_kwargs, wt_thresh, cdf_thresh, lprob_kwargs, track)
    'a': (151, 1501, 8, 2, 'gauss', 'harmonic', {}, 1e-3, 2e-4, {'free_scale': True, 'ignore_model_err': True}, False),
    'b': (152, 1502, 5, 3, 'lorentz', 'geometric', {'start': .8, 'end': .05}, 1e-2, 2e-4,
          {'free_scale': True, 'ignore_model_err': True}, False),
    'c': (153, 1503, 8, 2, 'gauss', 'harmonic', {}, None, 0.01, {'free_scale': True, 'ignore_model_err': True}, False),
    'd': (154, 1504, 6, 2, 'gauss', 'harmonic', {}, 1e-3, 2e-4, {'free_scale': True, 'ignore_model_err': True, 'return_scale': True},
          True),
    'e': (155, 1505, 8, 2, 'gauss', 'harmonic', {}, 1e-3, 2e-4, {'free_scale': False, 'ignore_model_err': False}, False),
}


MODELS = {'a': (151, 3000, 5, True), 'b': (152, 1500, 8, True), 'c': (153, 2000, 5, 'err'), 'd': (154, 2000, 5, True),
          'e': (155, 2000, 5, True), 'f': (156, 500, 5, False), 'g': (157, 20000, 5, 'err')}


def som_models(seed, M, B, bad=True):
    """tests/golden/make_golden_som.py's models: G15 keeps their sums and which entries are bad, the tests regenerate them"""
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
    """the case's models, checked against what G15 recorded of them"""
    Y, Ye, Ym = som_models(*MODELS[tag])
    np.testing.assert_allclose([np.sum(np.where(np.isfinite(Y), Y, 0)), np.sum(np.where(np.isfinite(Ye), Ye, 0)), Ym.sum()],
                               g[tag + '_in_sums'], rtol=1e-13)
    np.testing.assert_array_equal(np.flatnonzero(~(np.isfinite(Y) & np.isfinite(Ye) & (Ye > 0))), g[tag + '_in_bad'])
    return Y, Ye, Ym


def expected_cleaned(g, tag, Y, Ye, Ym):
    """the caller's arrays after training: the entries G15 saw change set to (0, 1, 0) -- the clean of pdf.py:309-311"""
    ch = g[tag + '_out_changed']
    out = []
    for a, k, v in zip((Y, Ye, Ym), range(3), (0., 1., 0.)):
        a = a.copy(); a.ravel()[ch[k]] = v; out.append(a)
    return out


@pytest.fixture(scope='module')
def g():
    return dict(np.load(G15))


def test_nodes_pos(g):
    for tag in 'abcdef':
        nside, nproj = {'a': (8, 2), 'b': (5, 3), 'c': (8, 2), 'd': (6, 2), 'e': (8, 2), 'f': (4, 2)}[tag]
        np.testing.assert_array_equal(net.som_nodes_pos(nside, nproj), g[tag + '_nodes_pos'])


def test_draw_stream_is_one_randint_call(g):
    """T scalar rstate.choice(Nmodel) calls == one randint(0, Nmodel, size=T) for the legacy RandomState"""
    for tag, (mseed, rseed, nside, nproj) in ((t, c[:4]) for t, c in CASES.items()):
        M = MODELS[tag][1]
        rs = np.random.RandomState(rseed)
        if tag != 'd':
            rs.choice(M, size=nside**nproj, replace=False)           # the node initialisation comes first
        np.testing.assert_array_equal(net._draw_stream(rs, M, 1000), g[tag + '_draws'])
    rs = np.random.RandomState(1507)
    rs.choice(20000, size=2500, replace=False)
    np.testing.assert_array_equal(net._draw_stream(rs, 20000, 1000), g['g_draws_head'])
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    assert [a.choice(77) for _ in range(500)] == list(net._draw_stream(b, 77, 500))


def test_learn_and_neighbor_functions(g):
    ts = np.linspace(0., 1., 7)
    for nm in ('learn_linear', 'learn_geometric', 'learn_harmonic'):
        f = getattr(net, nm)
        np.testing.assert_array_equal([f(t, start=.6, end=.03) for t in ts], g['fn_' + nm])
        np.testing.assert_array_equal(net._learn_table(f, ts, (), {'start': .6, 'end': .03}), g['fn_' + nm])
    pos = np.array([[0, 0], [1, 2], [3, 1], [4, 4]], dtype=float)
    for nm in ('neighbor_gauss', 'neighbor_lorentz'):
        w, s = getattr(net, nm)(0.3, pos[1], pos, 5, rate='geometric')
        np.testing.assert_array_equal(w, g['fn_' + nm]); assert s == g['fn_' + nm + '_sigma']
        assert net._sigma_table(getattr(net, nm), np.array([0.3]), 5, (), {'rate': 'geometric'})[0] == s
    with pytest.raises(ValueError):
        net._sigma_table(net.neighbor_gauss, ts, 5, (), {'rate': 'cubic'})
    # the whole-array form of the +-*/ rates equals the per-t calls bit for bit
    T = np.linspace(0., 1., 100000)
    for f in (net.learn_linear, net.learn_harmonic):
        v = net._learn_table(f, T, (), {})
        assert all(v[i] == f(T[i]) for i in range(0, 100000, 997))


def restated_lnprob(x, xe, xm, y, kw):
    """pdf.py:76-98 / 171-235 for one row against noiseless, unmasked nodes (ye = 0, ym = 1)"""
    free, dim_prior = kw.get('free_scale', False), kw.get('dim_prior', True)
    tot_var = np.square(xe) + np.zeros_like(y)
    tot_mask = xm * np.ones_like(y)
    Ndim = np.sum(tot_mask, axis=1)
    scale = np.ones(len(y))
    if free:
        inter = np.sum(tot_mask * y * x[None, :] / tot_var, axis=1)
        shape = np.sum(tot_mask * np.square(y) / tot_var, axis=1)
        scale = inter / shape
        chi2 = np.sum(tot_mask * np.square(x - scale[:, None] * y) / tot_var, axis=1)
    else:
        chi2 = np.sum(tot_mask * np.square(x - y) / tot_var, axis=1)
    if dim_prior:
        a = 0.5 * (Ndim - 1) if free else 0.5 * Ndim
        xl = np.where(a - 1. == 0, np.where(np.isnan(chi2), chi2, 0.), (a - 1.) * np.log(chi2))
        lnl = xl - chi2 / 2. - np.array([math.lgamma(v) for v in a]) - np.log(2.) * a
    else:
        lnl = -0.5 * chi2 - 0.5 * (Ndim * np.log(2. * np.pi) + np.sum(np.log(tot_var), axis=1))
    return lnl, scale


def restated_training(Y, Ye, Ym, rseed, nside, nproj, neighbour, learn, learn_kwargs, wt_thresh, cdf_thresh, lprob_kwargs, track,
                      nodes_init=None, niter=40, nbatch=25):
    """networks.py:1812-1867 with the tables of the device path and the rows cleaned up front"""
    T = niter * nbatch
    times = np.linspace(0., 1., T)
    rs = np.random.RandomState(rseed)
    pos = net.som_nodes_pos(nside, nproj)
    if nodes_init is None:
        nodes = np.array(Y[rs.choice(len(Y), size=nside**nproj, replace=False)])
    else:
        nodes = nodes_init.copy()
    draws = net._draw_stream(rs, len(Y), T)
    lr = net._learn_table(getattr(net, 'learn_' + learn), times, (), learn_kwargs)
    sig = net._sigma_table(getattr(net, 'neighbor_' + neighbour), times, nside, (), {})
    x, xe, xm = Y.copy(), Ye.copy(), Ym.copy()
    net._clean_rows(x, xe, xm, np.arange(len(Y)))
    bmus = np.zeros(T, dtype=int)
    for i in range(T):
        j = draws[i]
        lnl, s = restated_lnprob(x[j], xe[j], xm[j], nodes, lprob_kwargs)
        if track:
            nodes *= s[:, None]
        bmu = bmus[i] = np.argmax(lnl)
        d = np.sum((pos[bmu] - pos)**2, axis=1)
        w = np.exp(-0.5 * d / sig[i]**2) if neighbour == 'gauss' else sig[i]**2 / (d + sig[i]**2)
        if wt_thresh is not None:
            keep = np.arange(len(w))[w > wt_thresh * np.max(w)]
        else:
            o = np.argsort(w, kind='stable')                          # ties in node-index order
            keep = o[np.cumsum(w[o] / np.sum(w)) <= 1. - cdf_thresh]
        nodes[keep] += lr[i] * w[keep, None] * (x[j] - nodes[keep])
    return nodes, bmus, (x, xe, xm), draws


@pytest.mark.parametrize('tag', sorted(CASES))
def test_restated_loop_reproduces_g15(g, tag):
    c = CASES[tag]
    Y, Ye, Ym = case_models(g, tag)
    if tag == 'e':
        Ye = np.sqrt(Ye**2 + np.full_like(Ye, g['e_err_kernel'])**2)
    with np.errstate(all='ignore'):
        nodes, bmus, clean, draws = restated_training(Y, Ye, Ym, *c[1:], nodes_init=g['d_init'] if tag == 'd' else None)
    np.testing.assert_array_equal(bmus, g[tag + '_bmus'])
    np.testing.assert_allclose(nodes, g[tag + '_nodes'], rtol=1e-10)
    if tag == 'a':
        # the caller's arrays end with every DRAWN row cleaned (pdf.py:309-311), the others untouched
        x, xe, xm = Y.copy(), Ye.copy(), Ym.copy()
        net._clean_rows(x, xe, xm, np.unique(draws))
        for mine, ref in zip((x, xe, xm), expected_cleaned(g, 'a', Y, Ye, Ym)):
            np.testing.assert_array_equal(mine, ref)
        assert g['a_out_changed'][0].any() and g['a_out_changed'][1].any()
