"""G15: SelfOrganizingMap.train_network of the reference (networks.py:1490-1867), recorded for tests/test_som_host.py and
tests/test_hip_som.py.  Run from the repository root with the reference importable (as make_golden.py is):

    python tests/golden/make_golden_som.py

Recorded per case: the draw stream (a recording stand-in for the RandomState), every step's BMU, the final nodes, nodes_pos, and
the two safety margins of an exact comparison -- the smallest relative gap between the best and the second-best node ln-prob of a
step, and the smallest relative distance of a weight (wt_thresh rule) or of a running probability (CDF rule) to its threshold.
The script asserts that neither is within rounding and that no tie group of equal weights straddles the CDF boundary."""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('FRANKENZ_REFERENCE', '/root/reference'))

from frankenz import networks as rnet  # noqa: E402


def som_models(seed, M, B, bad=True):
    """lognormal fluxes, 5 % errors, ~2 % of the bands masked and (bad=True) a few non-finite values / non-positive errors
    (bad='err': the errors only -- a nan value in a row the nodes are initialised from makes that node the BMU of every step)"""
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


def lp_foreign(x, xe, xm, y, ye, ym, *args, **kwargs):
    """case f's user likelihood: a plain chi2 without cleaning or priors"""
    chi2 = np.sum(xm * (x - y)**2 / xe**2, axis=1)
    lnl = -0.5 * chi2
    return np.zeros_like(lnl), lnl, lnl, np.sum(xm * ym, axis=1), chi2


class Recorder(object):
    """RandomState stand-in: records every scalar choice (the per-step draws)"""
    def __init__(self, seed):
        self.rs = np.random.RandomState(seed); self.draws = []

    def choice(self, a, size=None, replace=True, p=None):
        out = self.rs.choice(a, size=size, replace=replace, p=p)
        if size is None:
            self.draws.append(int(out))
        return out


def run(tag, Y, Ye, Ym, seed, nodes_init=None, **kw):
    som = rnet.SelfOrganizingMap(Y, Ye, Ym)
    rec = Recorder(seed)
    models, models_err, models_mask = Y, Ye, Ym
    err_kernel = kw.pop('err_kernel', None)
    if err_kernel is not None:
        models_err = np.sqrt(models_err**2 + err_kernel**2)
    nside, nbatch, niter = kw.get('nside', 50), kw.get('nbatch', 50), kw.get('niter', 2000)
    wt_thresh, cdf_thresh = kw.get('wt_thresh', 1e-3), kw.get('cdf_thresh', 2e-4)
    neighbor = kw.get('neighbor_func', rnet.neighbor_gauss)
    nkw = kw.get('neighbor_kwargs', {})
    times = np.linspace(0., 1., niter * nbatch)
    bmus, gap, margin = [], np.inf, np.inf
    t0 = time.time()
    for i, (res, bmu, lr, sig) in enumerate(som._train_network(models, models_err, models_mask, nodes_init=nodes_init, rstate=rec, **kw)):
        lp = np.asarray(res[2])
        bmus.append(int(bmu))
        if np.isfinite(lp).all():
            top = np.sort(lp)[-2:]
            gap = min(gap, (top[1] - top[0]) / max(1., abs(top[1])))
        w, _ = neighbor(times[i], som.nodes_pos[bmu], som.nodes_pos, nside, **nkw)
        if wt_thresh is not None:
            wmin = wt_thresh * np.max(w)
            margin = min(margin, np.min(np.abs(w - wmin)) / wmin)
        else:
            srt = np.sort(w)
            cdf = np.cumsum(srt / np.sum(w))
            lim = 1. - cdf_thresh
            margin = min(margin, np.min(np.abs(cdf - lim)))
            nk = int(np.sum(cdf <= lim))
            if 0 < nk < len(w):
                assert srt[nk - 1] != srt[nk], "%s step %d: a tie group straddles the CDF boundary" % (tag, i)
    print('%s: %d steps in %.1f s, min top-2 gap %.3g, min threshold margin %.3g' % (tag, len(bmus), time.time() - t0, gap, margin))
    assert gap > 1e-9 and margin > 1e-9, tag
    return som, np.array(rec.draws, dtype=np.int64), np.array(bmus, dtype=np.int16), gap, margin


def changed(new, old):
    """which entries the training changed in place (the reference cleans every drawn row of the arrays it reads, pdf.py:309-311)"""
    return ~((new == old) | (np.isnan(new) & np.isnan(old))).ravel()


def main():
    out = {}

    def inputs(tag, Y, Ye, Ym):
        """the tests regenerate the models from the seed: keep their sums, and which entries were non-finite or err <= 0"""
        out[tag + '_in_sums'] = np.array([np.sum(np.where(np.isfinite(Y), Y, 0)), np.sum(np.where(np.isfinite(Ye), Ye, 0)), Ym.sum()])
        out[tag + '_in_bad'] = np.flatnonzero(~(np.isfinite(Y) & np.isfinite(Ye) & (Ye > 0))).astype(np.int32)

    def keep(tag, som, draws, bmus, gap, margin, nodes=True):
        out[tag + '_draws'], out[tag + '_bmus'] = draws.astype(np.int16), bmus
        out[tag + '_gap'], out[tag + '_margin'] = np.array(gap), np.array(margin)
        out[tag + '_nodes_pos'] = som.nodes_pos.astype(np.int8)
        if nodes:
            out[tag + '_nodes'] = np.asarray(som.nodes)

    # a: defaults at a small size, with masked bands and entries the likelihood cleans
    Y, Ye, Ym = som_models(151, 3000, 5)
    inputs('a', Y, Ye, Ym)
    Y0, Ye0, Ym0 = Y.copy(), Ye.copy(), Ym.copy()
    res = run('a', Y, Ye, Ym, 1501, nside=8, nproj=2, niter=40, nbatch=25)
    keep('a', *res)
    out['a_out_changed'] = np.stack([changed(Y, Y0), changed(Ye, Ye0), changed(Ym, Ym0)])
    # b: three grid dimensions, Lorentzian neighbourhood, geometric learning rate, wt_thresh 1e-2, 8 bands
    Y, Ye, Ym = som_models(152, 1500, 8)
    inputs('b', Y, Ye, Ym)
    keep('b', *run('b', Y, Ye, Ym, 1502, nside=5, nproj=3, niter=40, nbatch=25, neighbor_func=rnet.neighbor_lorentz,
                   learn_func=rnet.learn_geometric, learn_kwargs={'start': .8, 'end': .05}, wt_thresh=1e-2))
    # c: the CDF rule.  Grid nodes at equal distances from the BMU share a weight, so almost any boundary inside the neighbourhood
    # splits a tie group (whose order np.argsort leaves open); a cdf_thresh below the BMU's own probability (>= 1 / 64 here) puts
    # the boundary just before the BMU at every step
    Y, Ye, Ym = som_models(153, 2000, 5, bad='err')
    inputs('c', Y, Ye, Ym)
    keep('c', *run('c', Y, Ye, Ym, 1503, nside=8, nproj=2, niter=40, nbatch=25, wt_thresh=None, cdf_thresh=0.01))
    # d: track_scale with the scale returned, nodes_init given (trained in place)
    Y, Ye, Ym = som_models(154, 2000, 5)
    rs = np.random.RandomState(1544)
    init = Y[rs.choice(2000, 36, replace=False)] * rs.uniform(0.5, 1.5, size=(36, 1))
    init = np.where(np.isfinite(init), init, 1.)
    inputs('d', Y, Ye, Ym)
    out['d_init'] = init.copy()
    ni = init.copy()
    res = run('d', Y, Ye, Ym, 1504, nodes_init=ni, nside=6, nproj=2, niter=40, nbatch=25, track_scale=True,
              lprob_kwargs={'free_scale': True, 'ignore_model_err': True, 'return_scale': True})
    assert res[0].nodes is ni
    keep('d', *res)
    out['d_init_after'] = ni
    # e: err_kernel and a fixed-scale likelihood that keeps the model errors (dim_prior on)
    Y, Ye, Ym = som_models(155, 2000, 5)
    ek = np.full_like(Ye, 0.02)
    inputs('e', Y, Ye, Ym)
    out['e_err_kernel'] = np.array(0.02)
    Y0, Ye0, Ym0 = Y.copy(), Ye.copy(), Ym.copy()
    keep('e', *run('e', Y, Ye, Ym, 1505, nside=8, nproj=2, niter=40, nbatch=25, err_kernel=ek,
                   lprob_kwargs={'free_scale': False, 'ignore_model_err': False}))
    out['e_out_changed'] = np.stack([changed(Y, Y0), changed(Ye, Ye0), changed(Ym, Ym0)])
    # f: a foreign lprob_func (host loop)
    Y, Ye, Ym = som_models(156, 500, 5, bad=False)
    inputs('f', Y, Ye, Ym)
    keep('f', *run('f', Y, Ye, Ym, 1506, nside=4, nproj=2, niter=10, nbatch=10, lprob_func=lp_foreign))
    # the learn / neighbour functions at a few points
    ts = np.linspace(0., 1., 7)
    for nm in ('learn_linear', 'learn_geometric', 'learn_harmonic'):
        out['fn_' + nm] = np.array([getattr(rnet, nm)(t, start=.6, end=.03) for t in ts])
    pos = np.array([[0, 0], [1, 2], [3, 1], [4, 4]], dtype=float)
    for nm in ('neighbor_gauss', 'neighbor_lorentz'):
        w, s = getattr(rnet, nm)(0.3, pos[1], pos, 5, rate='geometric')
        out['fn_' + nm], out['fn_' + nm + '_sigma'] = w, np.array(s)
    # g: the default size (nside 50, niter 2000, nbatch 50) on 20 000 models; the models are regenerated by the tests from the seed
    Y, Ye, Ym = som_models(157, 20000, 5, bad='err')
    inputs('g', Y, Ye, Ym)
    som, draws, bmus, gap, margin = run('g', Y, Ye, Ym, 1507)
    out['g_bmus'], out['g_nodes'] = bmus, np.asarray(som.nodes)
    out['g_draws_head'] = draws[:1000].astype(np.int16)
    out['g_gap'], out['g_margin'] = np.array(gap), np.array(margin)
    np.savez_compressed(os.path.join(HERE, 'g15_som_train'), **out)
    print('wrote', os.path.join(HERE, 'g15_som_train.npz'), os.path.getsize(os.path.join(HERE, 'g15_som_train.npz')))


if __name__ == '__main__':
    main()
