"""A plain, high-precision restatement of what the four network-inference kernels of fz_net.h compute (the reference's
networks.py:885-896 and 316-333: selection and its statistics; 907-919: the union table and the gather; 1459-1473: the stack of
node PDFs).  NumPy only: no GPU, no import of the package.  Probabilities, running sums and weighted sums are np.longdouble.

Two conventions are the project's, not NumPy's, and are said so where they apply (docs/deviations.md):
  * ties under the CDF rule go by column index (a stable sort); np.argsort leaves them undefined;
  * wt_thresh < 0 (the -inf that Network substitutes when both thresholds are None) keeps every column; NumPy's log gives nan."""
import numpy as np

LD = np.longdouble


def _lse(v):
    """scipy's logsumexp in longdouble: (max, logsumexp); a max that is not finite is its own logsumexp"""
    v = np.asarray(v, dtype=np.float64)
    mx = np.max(v)
    if not np.isfinite(mx):
        return mx, LD(mx)                                           # -inf: log 0; +inf: log inf; nan: nan
    return mx, LD(mx) + np.log(np.sum(np.exp(v.astype(LD) - LD(mx))))


def select(lnprob_row, use_wt, wt_thresh, cdf_thresh):
    """(sel, gap): the selected column indices in the reference's order, and the smallest |cdf - (1 - cdf_thresh)| of the row
    (inf under the weight rule, and where no cdf is a number).  A row holding a nan selects nothing."""
    lp = np.asarray(lnprob_row, dtype=np.float64)
    none = np.zeros(0, dtype=np.int64)
    with np.errstate(all='ignore'):
        if use_wt:
            if wt_thresh < 0:                                       # the project's sentinel: no clipping
                return (none if np.isnan(lp).any() else np.arange(len(lp))), np.inf
            return np.arange(len(lp))[lp > np.log(wt_thresh) + np.max(lp)], np.inf
        if np.isnan(lp).any():
            return none, np.inf
        order = np.argsort(lp, kind='stable')
        mx, lse = _lse(lp)
        # (a max of -inf: -inf - -inf = nan everywhere; of +inf: exp(-inf) = 0 below it and inf - inf = nan at it)
        prob = np.exp(lp.astype(LD) - lse)
        cdf = np.cumsum(prob[order])
        lim = LD(1. - cdf_thresh)
        gaps = np.abs(cdf - lim)
        gaps = gaps[~np.isnan(gaps)]
        return order[cdf <= lim], (float(gaps.min()) if len(gaps) else np.inf)


def stats(lnprob_row, sel):
    """(max, longdouble logsumexp) over the kept entries; an empty selection gives (-inf, -inf)"""
    if len(sel) == 0:
        return -np.inf, LD(-np.inf)
    with np.errstate(all='ignore'):
        return _lse(np.asarray(lnprob_row, dtype=np.float64)[sel])


def rawlen(sel, match, csr_off):
    """summed length of the selected columns' node lists"""
    nd = np.asarray(match)[sel]
    return int(np.sum(np.asarray(csr_off)[nd + 1] - np.asarray(csr_off)[nd])) if len(sel) else 0


def table(sel_rows, match, csr_off, csr_items, W):
    """(N, W): every object's selected nodes' lists concatenated in selection order, cut at W, padded with the row's first entry
    (0 where the row has none)"""
    out = np.zeros((len(sel_rows), W), dtype=np.int64)
    for i, sel in enumerate(sel_rows):
        parts = [csr_items[csr_off[match[c]]:csr_off[match[c] + 1]] for c in sel]
        row = np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, dtype=np.int64)
        n = min(len(row), W)
        out[i, :n] = row[:n]
        out[i, n:] = row[0] if len(row) else 0
    return out


def gather(plane, sel_rows, W, pad):
    """(N, W) of the plane's dtype: plane[i, sel] in selection order, `pad` beyond"""
    out = np.full((len(sel_rows), W), pad, dtype=plane.dtype)
    for i, sel in enumerate(sel_rows):
        n = min(len(sel), W)
        out[i, :n] = plane[i, sel[:n]]
    return out


def stack(lnprob, sel_rows, match, node_pdfs):
    """(pdfs (N, G) longdouble, lmap (N,), levid (N,) longdouble): softmax over the selected ln-probabilities @ the selected nodes'
    PDFs, each row divided by its sum; an empty selection gives a nan row (0 / 0) and (-inf, -inf)"""
    N, G = len(sel_rows), node_pdfs.shape[1]
    pdfs = np.zeros((N, G), dtype=LD); lmap = np.zeros(N); levid = np.zeros(N, dtype=LD)
    with np.errstate(all='ignore'):
        for i, sel in enumerate(sel_rows):
            lmap[i], levid[i] = stats(lnprob[i], sel)
            wt = np.exp(lnprob[i][sel].astype(LD) - levid[i])
            p = (wt[:, None] * node_pdfs[np.asarray(match)[sel]].astype(LD)).sum(axis=0)
            pdfs[i] = p / p.sum()
    return pdfs, lmap, levid
