"""Plain NumPy restatement of the four per-object loops of the reference's plotting.py (input_vs_pdf, input_vs_dpdf, cdf_vs_epdf,
cdf_vs_ecdf) without any drawing: what tests/test_hip_diag.py compares the device against at shapes the G19 fixture does not
hold.  tests/test_diag_host.py pins it to G19 (stacks to rtol 1e-14 for np.sum's pairwise order, draws bit for bit).

One object at a time, float64 throughout, the reference's operation order inside an object: cut, divide the kept entries by
their sum, outer product with the clipped kernel, divide by the product's total, times the weight."""
import numpy as np


def select_objects(weights, nobj, wt_thresh=1e-3, cdf_thresh=2e-4):
    """[(object, weight it is stacked with)] in loop order; the CDF rule pairs the object at sorted position i with weights[i]"""
    if weights is None:
        weights = np.ones(nobj, dtype='float32')
    weights = np.asarray(weights)
    if wt_thresh is None and cdf_thresh is None:
        wt_thresh = -np.inf
    if wt_thresh is not None:
        order, keep = np.arange(nobj), weights > wt_thresh * np.max(weights)
    else:
        order = np.argsort(weights, kind='stable')
        run = np.cumsum(weights[order])
        run /= run[-1]
        keep = run <= 1. - cdf_thresh
    return [(int(order[i]), weights[i]) for i in range(nobj) if keep[i]]


def cut_pdf(p, pdf_wt_thresh=1e-3, pdf_cdf_thresh=2e-4):
    """(kept columns, kept entries divided by their sum)"""
    p = np.array(p, dtype=np.float64)
    if pdf_wt_thresh is None and pdf_cdf_thresh is None:
        pdf_wt_thresh = -np.inf
    if pdf_wt_thresh is not None:
        with np.errstate(invalid='ignore'):                         # 0 * -inf = nan for a row of zeros: nothing is kept
            cols = np.flatnonzero(p > max(p) * pdf_wt_thresh)
    else:
        order = np.argsort(p, kind='stable')
        cols = order[np.cumsum(p[order]) <= 1. - pdf_cdf_thresh]
    return cols, p[cols] / np.sum(p[cols])


def stack_rows(vals, errs, vdict, rows, weights=None, pdf_wt_thresh=1e-3, pdf_cdf_thresh=2e-4, wt_thresh=1e-3, cdf_thresh=2e-4):
    """the (vdict.Ngrid, rows.shape[1]) stack of ``rows`` (PDFs, or PDFs already recentred)"""
    gx = vdict.Ngrid
    out = np.zeros((gx, rows.shape[1]))
    cidx, eidx = vdict.fit(np.asarray(vals), np.asarray(errs))
    for obj, w in select_objects(weights, len(vals), wt_thresh, cdf_thresh):
        cols, q = cut_pdf(rows[obj], pdf_wt_thresh, pdf_cdf_thresh)
        e, c = eidx[obj], cidx[obj]
        hw, kern = vdict.sigma_width[e], np.asarray(vdict.sigma_dict[e])
        lo, hi = max(c - hw, 0), min(c + hw + 1, gx)
        block = np.outer(kern[lo - (c - hw):hi - (c - hw)], q)
        block /= np.sum(block)
        out[lo:hi, cols] += block * w
    return out


def input_vs_pdf(vals, errs, vdict, pdfs, pgrid, weights=None, **thresholds):
    return stack_rows(vals, errs, vdict, np.asarray(pdfs), weights, **thresholds)


def recentre(pdfs, pgrid, pdf_cent, dgrid, disp=None):
    """row i resampled onto dgrid around pdf_cent[i]; disp(pgrid, cent) defaults to pgrid - cent"""
    if disp is None:
        disp = lambda g, c: g - c                                   # noqa: E731
    return np.array([np.interp(dgrid, disp(np.asarray(pgrid), c), p) for p, c in zip(pdfs, pdf_cent)])


def input_vs_dpdf(vals, errs, vdict, pdfs, pgrid, pdf_cent, dgrid, weights=None, disp=None, **thresholds):
    return stack_rows(vals, errs, vdict, recentre(pdfs, pgrid, pdf_cent, dgrid, disp), weights, **thresholds)


def cdf_draws(vals, errs, pdfs, pdf_grid, Nmc, rstate):
    """(Nobj, Nmc) CDF values at per-object normal draws of the truth, drawn object by object"""
    out = np.zeros((len(vals), Nmc))
    for i in range(len(vals)):
        cdf = np.cumsum(pdfs[i])
        cdf = cdf / cdf[-1]
        out[i] = np.interp(rstate.normal(vals[i], errs[i], size=Nmc), pdf_grid, cdf)
    return out


def cdf_vs_epdf(vals, errs, pdfs, pdf_grid, Nmc=100, weights=None, Nbins=50, rstate=None):
    w = np.ones(len(vals)) if weights is None else np.asarray(weights, dtype=np.float64)
    draws = cdf_draws(vals, errs, pdfs, pdf_grid, Nmc, rstate)
    n, _ = np.histogram(draws.ravel(), bins=np.linspace(0., 1., Nbins + 1), weights=np.repeat(w, Nmc), density=True)
    return n


def cdf_vs_ecdf(vals, errs, pdfs, pdf_grid, Nmc=100, weights=None, rstate=None):
    w = np.repeat(np.ones(len(vals)) if weights is None else np.asarray(weights, dtype=np.float64), Nmc)
    draws = cdf_draws(vals, errs, pdfs, pdf_grid, Nmc, rstate).ravel()
    order = np.argsort(draws)
    d, w = draws[order], w[order]
    step = np.append(d[0], d[1:] - d[:-1])
    return np.cumsum(w) / np.sum(w), np.cumsum(w * step) / np.sum(w * step)


class StoredDict(object):
    """the dictionary of a golden file, from its stored arrays (nothing is recomputed): the attributes ``plotting`` reads"""

    def __init__(self, g):
        self.grid, self.sigma_grid = g['xgrid'], g['sigma_grid']
        self.Ngrid, self.Ndict = len(self.grid), len(self.sigma_grid)
        self.delta, self.dsigma = float(g['delta']), float(g['dsigma'])
        self.sigma_width = g['sigma_width']
        off = np.concatenate(([0], np.cumsum(2 * self.sigma_width + 1)))
        self.sigma_dict = [g['kern'][a:b] for a, b in zip(off[:-1], off[1:])]
        self.sigma_dict_cdf = [g['kern_cdf'][a:b] for a, b in zip(off[:-1], off[1:])]

    def fit(self, X, Xe):
        X_idx = ((np.asarray(X) - self.grid[0]) / self.delta).round().astype('int')
        Xe_idx = np.array(np.round((np.asarray(Xe) - self.sigma_grid[0]) / self.dsigma), dtype='int')
        np.clip(Xe_idx, 0, self.Ndict - 1, out=Xe_idx)
        return X_idx, Xe_idx
