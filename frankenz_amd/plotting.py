"""
Validation of PDFs against known values: the reference's ``frankenz/plotting.py`` (plotting.py:31-520) with its per-object
Python loops run on the GPU (docs/diagnostics.md).

``input_vs_pdf`` / ``input_vs_dpdf`` stack, per object, the outer product of its dictionary kernel at the true value and its
thresholded, renormalised PDF; summed over objects that is one matrix product (``fz_stack2d``).  ``cdf_vs_epdf`` /
``cdf_vs_ecdf`` draw the truth ``Nmc`` times per object and read each draw off the object's CDF (``fz_cdf_draws``).

Names, positional order and defaults are the reference's.  Two keyword extensions everywhere: ``device=None`` (as in the rest
of the package) and ``plot=True`` -- with ``plot=False`` nothing of matplotlib is imported and only the numbers are returned.
``pdfs`` may be a NumPy array or a device-resident array (anything with ``data_ptr()``), which is never copied to the host.
The drawing itself is the reference's matplotlib calls, unchanged.
"""
import numpy as np

from .engine import get_engine

__all__ = ["input_vs_pdf", "input_vs_dpdf", "cdf_vs_epdf", "cdf_vs_ecdf", "disp_scaled"]


def disp_scaled(pgrid, cent):
    """Redshift-scaled dispersion ``(pgrid - cent) / (1 + cent)`` for ``input_vs_dpdf(disp_func=disp_scaled)``: recognised
    by identity and evaluated on the device with the same roundings."""
    return (pgrid - cent) / (1. + cent)


def _is_resident(pdfs):
    return not isinstance(pdfs, np.ndarray) and hasattr(pdfs, "data_ptr")


def _as_pdfs(pdfs, Nobj, Ngrid):
    """a C-contiguous float64 (Nobj, Ngrid) host array, or the resident array as it is"""
    if _is_resident(pdfs):
        if tuple(pdfs.shape) != (Nobj, Ngrid) or pdfs.element_size() != 8 or not pdfs.is_contiguous():
            raise ValueError("a device-resident `pdfs` must be a contiguous float64 array of shape (Nobj, Ngrid)")
        return pdfs
    pdfs = np.ascontiguousarray(pdfs, dtype=np.float64)
    if pdfs.shape != (Nobj, Ngrid):
        raise ValueError("`pdfs` must have shape (Nobj, Ngrid) = (%d, %d)" % (Nobj, Ngrid))
    return pdfs


def _finite_1d(name, a):
    bad = np.flatnonzero(~np.isfinite(a))
    if len(bad):
        raise ValueError("`%s` of object %d is not finite" % (name, bad[0]))


def stack_selection(vals, errs, vdict, weights=None, wt_thresh=1e-3, cdf_thresh=2e-4):
    """The object bookkeeping of ``input_vs_pdf`` / ``input_vs_dpdf`` (plotting.py:110-129, 146-152), O(N log N) on the host.

    Returns ``(objids, weff, cent, eidx)`` of the selected objects in loop order: the object's index, the weight it is stacked
    with, the grid index of its centre and its dictionary entry (``vdict.fit``).  Weight rule: ``weights > wt_thresh *
    max(weights)``; both thresholds ``None``: every object.  CDF rule (``wt_thresh=None``), as the reference has it: ascending
    sort, running sum divided by its last entry, keep ``<= 1 - cdf_thresh`` -- and the object at sorted position ``i`` is
    stacked with ``weights[i]``, the weight at the loop position, not its own (plotting.py:129, 159).  The sort is stable (the
    reference's order among equal weights is unspecified).

    Raises ``ValueError`` naming the object for a non-finite value, error or weight, for a selected object whose dictionary
    entry is malformed (``len(sigma_dict[e]) != 2 * sigma_width[e] + 1``), and for one whose window ``[c - w, c + w]`` does
    not meet the grid."""
    vals, errs = np.asarray(vals, dtype=np.float64), np.asarray(errs, dtype=np.float64)
    Nobj = len(vals)
    if weights is None:
        weights = np.ones(Nobj, dtype='float32')
    weights = np.asarray(weights)
    if len(errs) != Nobj or len(weights) != Nobj:
        raise ValueError("`vals`, `errs` and `weights` must have the same length")
    _finite_1d("weights", weights)
    _finite_1d("vals", vals)
    _finite_1d("errs", errs)
    if Nobj == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, np.zeros(0), z, z
    if wt_thresh is None and cdf_thresh is None:
        wt_thresh = -np.inf
    if wt_thresh is not None:
        sel_arr = weights > (wt_thresh * np.max(weights))
        objids = np.arange(Nobj)
    else:
        idx_sort = np.argsort(weights, kind='stable')
        w_cdf = np.cumsum(weights[idx_sort])
        w_cdf /= w_cdf[-1]
        sel_arr = w_cdf <= (1. - cdf_thresh)
        objids = idx_sort
    pos = np.flatnonzero(sel_arr)
    objids = objids[pos].astype(np.int64)
    weff = weights[pos].astype(np.float64)                      # weights[i] of the loop position
    vidxs, eidxs = vdict.fit(vals, errs)
    cent, eidx = np.asarray(vidxs)[objids].astype(np.int64), np.asarray(eidxs)[objids].astype(np.int64)
    width = np.asarray(vdict.sigma_width, dtype=np.int64)
    lens = np.array([len(k) for k in vdict.sigma_dict], dtype=np.int64)
    bad = np.flatnonzero(lens[eidx] != 2 * width[eidx] + 1)
    if len(bad):
        raise ValueError("object %d: dictionary entry %d is malformed (%d taps for half-width %d)"
                         % (objids[bad[0]], eidx[bad[0]], lens[eidx[bad[0]]], width[eidx[bad[0]]]))
    w = width[eidx]
    bad = np.flatnonzero((cent + w < 0) | (cent - w > vdict.Ngrid - 1))
    if len(bad):
        k = bad[0]
        raise ValueError("object %d: its window [%d, %d] does not meet the grid [0, %d)"
                         % (objids[k], cent[k] - w[k], cent[k] + w[k], vdict.Ngrid))
    return objids, weff, cent, eidx


def _check_rows_finite(pdfs, objids, chunk=1 << 14):
    for lo in range(0, len(objids), chunk):
        ids = objids[lo:lo + chunk]
        ok = np.isfinite(pdfs[ids]).all(axis=1)
        if not ok.all():
            raise ValueError("the PDF of object %d holds a value that is not finite" % ids[np.flatnonzero(~ok)[0]])


def _cut_row(tpdf, pdf_wt_thresh, pdf_cdf_thresh):
    """plotting.py:137-143 for one row, by the reference's arithmetic: the row with its kept entries divided, the rest zero"""
    if pdf_wt_thresh is not None:
        tsel = tpdf > max(tpdf) * pdf_wt_thresh
    else:
        psort = np.argsort(tpdf, kind='stable')
        pcdf = np.cumsum(tpdf[psort])
        tsel = psort[pcdf <= (1. - pdf_cdf_thresh)]
    out = np.zeros_like(tpdf)
    out[tsel] = tpdf[tsel] / np.sum(tpdf[tsel])
    return out


def _sorted_by_centre(objids, weff, cent, eidx):
    o = np.argsort(cent, kind='stable')
    return (np.ascontiguousarray(objids[o]), np.ascontiguousarray(weff[o]), np.ascontiguousarray(cent[o]),
            np.ascontiguousarray(eidx[o]))


def _stack(eng, vdict, pdfs, Gy, sel, pdf_wt_thresh, pdf_cdf_thresh, prepare=None, full_range=False):
    """the stack of the selected objects ``sel = (objids, weff, cent, eidx)``.  ``prepare(ids) -> rows``: host rows of the
    objects ``ids`` replacing their PDFs (``input_vs_dpdf`` with a callable dispersion); with it, or with the per-row CDF rule,
    the rows are cut on the host in chunks and stacked as they stand."""
    objids, weff, cent, eidx = _sorted_by_centre(*sel)
    eng.upload_dict(vdict)
    stack = np.zeros((vdict.Ngrid, Gy))
    if pdf_wt_thresh is None and pdf_cdf_thresh is None:
        pdf_wt_thresh = -np.inf
    host_cut = prepare is not None or pdf_wt_thresh is None
    if not host_cut:
        eng.stack2d(pdfs, len(pdfs), Gy, objids, cent, eidx, weff, pdf_wt_thresh, False, stack, full_range=full_range)
        return stack
    if _is_resident(pdfs):
        raise NotImplementedError("the per-row CDF rule (pdf_wt_thresh=None) and a callable disp_func prepare the rows on the "
                                  "host: pass `pdfs` as a NumPy array")
    chunk = max(1, (1 << 27) // (8 * Gy))
    for n, lo in enumerate(range(0, len(objids), chunk)):
        ids = objids[lo:lo + chunk]
        src = pdfs[ids] if prepare is None else prepare(ids)
        rows = np.ascontiguousarray([_cut_row(np.array(r), pdf_wt_thresh, pdf_cdf_thresh) for r in src], dtype=np.float64)
        rows = rows.reshape(len(ids), Gy)
        eng.stack2d(rows, len(ids), Gy, np.arange(len(ids), dtype=np.int64), cent[lo:lo + chunk], eidx[lo:lo + chunk],
                    weff[lo:lo + chunk], -np.inf, True, stack, full_range=full_range, accumulate=n > 0)
    return stack


def _finish_stack(stack, smooth, plot_thresh, plot, xgrid, ygrid, cmap, plot_kwargs):
    if smooth != 0:
        from scipy.ndimage import gaussian_filter
        stack = gaussian_filter(stack, smooth)
    stack[stack < plot_thresh] = np.nan
    if plot:
        from matplotlib import pyplot as plt
        plt.imshow(stack.T, origin='lower', aspect='auto', extent=(xgrid[0], xgrid[-1], ygrid[0], ygrid[-1]), cmap=cmap,
                   **plot_kwargs)
        plt.colorbar(label='Number Density')
        plt.xlim([xgrid[0], xgrid[-1]])
        plt.ylim([ygrid[0], ygrid[-1]])
        plt.xlabel('Input')
        plt.ylabel('Predicted')
        plt.tight_layout()
    return stack


def input_vs_pdf(vals, errs, vdict, pdfs, pgrid, weights=None, pdf_wt_thresh=1e-3, pdf_cdf_thresh=2e-4, wt_thresh=1e-3,
                 cdf_thresh=2e-4, plot_thresh=0., cmap='viridis', smooth=0, plot_kwargs=None, verbose=False, *args,
                 device=None, plot=True, **kwargs):
    """Input values vs their PDFs (plotting.py:31-181): the ``(vdict.Ngrid, len(pgrid))`` stack of, per selected object, its
    dictionary kernel at ``(val, err)`` times its cut and renormalised PDF, normalised to unit sum and weighted.

    The objects are selected on the host (``stack_selection``); the per-PDF cut ``p > max(p) * pdf_wt_thresh``, the
    normalisations and the sum over objects run on the device, and a device-resident ``pdfs`` stays there.  With
    ``pdf_wt_thresh=None`` and a ``pdf_cdf_thresh`` (the per-row sorted-CDF cut) the rows are cut on the host in chunks, by
    the reference's arithmetic, and only the stack of the prepared rows is formed on the device; ``pdfs`` must then be a NumPy
    array.  ``smooth`` (``scipy.ndimage.gaussian_filter``) and ``plot_thresh`` are applied to the finished stack on the host.
    ``plot=False`` returns the stack without importing matplotlib.  ``verbose`` is accepted and prints nothing: there is no
    per-object loop to report on."""
    Gy, Nobj = len(pgrid), len(vals)
    pdfs = _as_pdfs(pdfs, Nobj, Gy)
    sel = stack_selection(vals, errs, vdict, weights, wt_thresh, cdf_thresh)
    if not _is_resident(pdfs):
        _check_rows_finite(pdfs, sel[0])
    stack = _stack(get_engine(device), vdict, pdfs, Gy, sel, pdf_wt_thresh, pdf_cdf_thresh)
    return _finish_stack(stack, smooth, plot_thresh, plot, vdict.grid, pgrid, cmap, plot_kwargs or dict())


def input_vs_dpdf(vals, errs, vdict, pdfs, pgrid, pdf_cent, dgrid, weights=None, disp_func=None, disp_args=None,
                  disp_kwargs=None, pdf_wt_thresh=1e-3, pdf_cdf_thresh=2e-4, wt_thresh=1e-3, cdf_thresh=2e-4, plot_thresh=0.,
                  cmap='viridis', smooth=0, plot_kwargs=None, verbose=False, *args, device=None, plot=True, **kwargs):
    """Input values vs their PDFs recentred on ``pdf_cent`` and resampled onto the dispersion grid ``dgrid``
    (plotting.py:184-366): ``np.interp(dgrid, disp_func(pgrid, cent_i), pdf_i)`` per object, then the stack of
    ``input_vs_pdf`` with ``len(dgrid)`` columns.

    ``disp_func=None`` (``pgrid - cent``) and ``disp_func=disp_scaled`` (``(pgrid - cent) / (1 + cent)``), without
    ``disp_args`` / ``disp_kwargs``, are resampled on the device, chunk by chunk, and a resident ``pdfs`` stays there.  Any
    other callable, and the per-row CDF cut (``pdf_wt_thresh=None``), prepare the rows on the host in chunks by the
    reference's arithmetic; the stack of the prepared rows is still formed on the device, and ``pdfs`` must be a NumPy array."""
    Gy, Gd, Nobj = len(pgrid), len(dgrid), len(vals)
    pdfs = _as_pdfs(pdfs, Nobj, Gy)
    pgrid_a, dgrid_a = np.ascontiguousarray(pgrid, dtype=np.float64), np.ascontiguousarray(dgrid, dtype=np.float64)
    pdf_cent = np.ascontiguousarray(pdf_cent, dtype=np.float64)
    if len(pdf_cent) != Nobj:
        raise ValueError("`pdf_cent` must have one entry per object")
    _finite_1d("pdf_cent", pdf_cent)
    sel = stack_selection(vals, errs, vdict, weights, wt_thresh, cdf_thresh)
    if not _is_resident(pdfs):
        _check_rows_finite(pdfs, sel[0])
    eng = get_engine(device)
    on_device = (disp_func is None or disp_func is disp_scaled) and not disp_args and not disp_kwargs
    both_none = pdf_wt_thresh is None and pdf_cdf_thresh is None
    if on_device and (pdf_wt_thresh is not None or both_none):
        objids, weff, cent, eidx = _sorted_by_centre(*sel)
        eng.upload_dict(vdict)
        stack = np.zeros((vdict.Ngrid, Gd))
        thresh = -np.inf if both_none else pdf_wt_thresh
        chunk = max(1, min(max(Nobj, 1), (1 << 29) // (8 * Gd)))
        buf = eng.device_empty((chunk, Gd))
        base, done = (pdfs.data_ptr() if _is_resident(pdfs) else None), False
        for lo in range(0, Nobj, chunk):
            hi = min(Nobj, lo + chunk)
            m = (objids >= lo) & (objids < hi)
            if not m.any():
                continue
            src = base + lo * Gy * 8 if base is not None else pdfs[lo:hi]
            eng.recentre_rows(src, hi - lo, pgrid_a, pdf_cent[lo:hi], int(disp_func is disp_scaled), dgrid_a, buf)
            eng.stack2d(buf, hi - lo, Gd, np.ascontiguousarray(objids[m] - lo), np.ascontiguousarray(cent[m]),
                        np.ascontiguousarray(eidx[m]), np.ascontiguousarray(weff[m]), thresh, False, stack, accumulate=done)
            done = True
    else:
        if _is_resident(pdfs):
            raise NotImplementedError("a callable disp_func and the per-row CDF rule prepare the rows on the host: pass `pdfs` "
                                      "as a NumPy array")
        if disp_func is None:
            def disp_func(pgrid, cent):
                return pgrid - cent
        dargs, dkw = disp_args or [], disp_kwargs or dict()

        def prepare(ids):
            return [np.interp(dgrid_a, disp_func(pgrid, pdf_cent[i], *dargs, **dkw), pdfs[i]) for i in ids]
        stack = _stack(eng, vdict, pdfs, Gd, sel, pdf_wt_thresh, pdf_cdf_thresh, prepare=prepare)
    return _finish_stack(stack, smooth, plot_thresh, plot, vdict.grid, dgrid, cmap, plot_kwargs or dict())


def _mc_truths(vals, errs, Nmc, rstate):
    """the ``Nmc`` normal draws of every truth in ONE call: it consumes the stream exactly as the reference's per-object
    ``rstate.normal(val, err, size=Nmc)`` calls do (plotting.py:430)"""
    vals, errs = np.asarray(vals, dtype=np.float64), np.asarray(errs, dtype=np.float64)
    _finite_1d("vals", vals)
    _finite_1d("errs", errs)
    if rstate is None:
        rstate = np.random
    return np.ascontiguousarray(rstate.normal(vals[:, None], errs[:, None], size=(len(vals), int(Nmc))))


def _cdf_inputs(vals, pdfs, pdf_grid, weights):
    Nobj, Ngrid = len(vals), len(pdf_grid)
    pdfs = _as_pdfs(pdfs, Nobj, Ngrid)
    if weights is None:
        weights = np.ones(Nobj, dtype='float32')
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    if len(weights) != Nobj:
        raise ValueError("`weights` must have one entry per object")
    _finite_1d("weights", weights)
    if not _is_resident(pdfs):
        _check_rows_finite(pdfs, np.arange(Nobj))
    return pdfs, np.ascontiguousarray(pdf_grid, dtype=np.float64), weights


def cdf_vs_epdf(vals, errs, pdfs, pdf_grid, Nmc=100, weights=None, Nbins=50, plot_kwargs=None, rstate=None, *args,
                device=None, plot=True, **kwargs):
    """CDF draws vs the empirical PDF (plotting.py:369-440): the density-normalised weighted histogram of the ``Nobj * Nmc``
    CDF values ``np.interp(normal(val, err), pdf_grid, cdf_i)`` over ``Nbins`` bins of [0, 1].

    The truths are drawn on the host in one call that consumes ``rstate`` as the reference does; CDFs, interpolation and
    the weighted counts run on the device, and the draws never come back.  ``density=True`` is applied on the host.  With
    ``plot=True`` the finished bars are drawn by ``plt.hist`` over the bin centres."""
    pdfs, grid, w = _cdf_inputs(vals, pdfs, pdf_grid, weights)
    mc = _mc_truths(vals, errs, Nmc, rstate)
    edges = np.linspace(0., 1., Nbins + 1)
    counts = np.zeros(Nbins)
    get_engine(device).cdf_draws(pdfs, len(mc), grid, mc, weights=w, edges=edges, hist=counts)
    n = counts / counts.sum() / np.diff(edges)
    if plot:
        from matplotlib import pyplot as plt
        if plot_kwargs is None:
            plot_kwargs = dict(color='blue', alpha=0.6)
        plt.hist(0.5 * (edges[1:] + edges[:-1]), bins=edges, weights=n, **plot_kwargs)
        plt.xlabel('CDF Draws')
        plt.ylabel('Normalized Counts')
    return n


def cdf_vs_ecdf(vals, errs, pdfs, pdf_grid, Nmc=100, weights=None, plot_kwargs=None, rstate=None, *args, device=None,
                plot=True, **kwargs):
    """CDF draws vs the empirical CDF (plotting.py:443-521): ``(x, y)``, the running weight and the running weighted
    spacing of the sorted draws, each divided by its total.

    The draws are made as in ``cdf_vs_epdf`` and brought back; the sort, the differences and the two running sums are the
    reference's NumPy calls on the host."""
    pdfs, grid, w = _cdf_inputs(vals, pdfs, pdf_grid, weights)
    mc = _mc_truths(vals, errs, Nmc, rstate)
    draws = np.empty_like(mc)
    get_engine(device).cdf_draws(pdfs, len(mc), grid, mc, draws=draws)
    cdf_draws = draws.flatten()
    wts = np.repeat(w, mc.shape[1])
    sort_idx = np.argsort(cdf_draws)
    cdf_sorted, weights_sorted = cdf_draws[sort_idx], wts[sort_idx]
    cdf_diff = np.append(cdf_sorted[0], cdf_sorted[1:] - cdf_sorted[:-1])
    x, y = weights_sorted, weights_sorted * cdf_diff
    x = x.cumsum() / x.sum()
    y = y.cumsum() / y.sum()
    if plot:
        from matplotlib import pyplot as plt
        if plot_kwargs is None:
            plot_kwargs = dict(color='blue', alpha=0.6)
        plt.plot(x, y, **plot_kwargs)
        plt.xlabel('Sorted CDF Draws')
        plt.ylabel('Empirical CDF')
    return x, y
