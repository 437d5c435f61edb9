"""
Function-level surface of ``frankenz.pdf`` for the hot path (reference
frankenz/pdf.py): ``logprob`` / ``loglike`` (pdf.py:238-411), ``gauss_kde`` /
``gauss_kde_dict`` (pdf.py:444-622), ``PDFDict`` (pdf.py:778-852) and the k-NN
feature maps ``luptitude`` / ``magnitude`` (pdf.py:625-657, 695-734).

The likelihood and KDE arithmetic runs on the GPU through the C ABI.  ``PDFDict``
(a one-off table of a few hundred short kernels) and the feature maps (O(N*B)
elementwise set-up for the neighbour search) are host-side set-up, as in the
reference; their tables are uploaded verbatim so the device reproduces the
reference's kernels, malformed entries included.
"""
import math

import numpy as np

from .engine import HostObjects, get_engine, kde_opts, like_opts

__all__ = ["loglike", "logprob", "logprob_prior", "logprob_prior_lerp", "lerp_cells", "gaussian", "gauss_kde", "gauss_kde_dict",
           "magnitude", "luptitude", "PDFDict", "pdfs_summarize", "pdfs_resample", "sample_labels", "sparsify_logwt", "posterior_moments",
           "gaussian_bin", "posterior_bins", "posterior_cdf", "posterior_quantiles", "posterior_scores", "BINS_MAX",
           "SCORES_NMAX"]

BINS_MAX = 256       # FZ_BINS_MAX: bins of a posterior_bins call, points of a posterior_cdf call


def _ndim_dtype(data_mask, models_mask):
    """np.sum(data_mask * models_mask, axis=1) keeps the masks' arithmetic type
    (pdf.py:82-83): bool/int masks give int64 counts, float masks float64."""
    t = np.result_type(np.asarray(data_mask).dtype, np.asarray(models_mask).dtype)
    return np.float64 if np.issubdtype(t, np.floating) else np.int64


def loglike(data, data_err, data_mask, models, models_err, models_mask, free_scale=False,
            ignore_model_err=False, dim_prior=True, ltol=1e-4, return_scale=False, device=None,
            *args, **kwargs):
    """One object against all models (pdf.py:238-323).  ``data``, ``data_err`` and
    ``data_mask`` are cleaned IN PLACE exactly like the reference (pdf.py:310-311).
    Returns ``(lnlike, Ndim, chi2[, scale, scale_err])``."""
    eng = get_engine(device)
    eng.upload_models(models, models_err, models_mask)
    obj = HostObjects(np.atleast_2d(data), np.atleast_2d(data_err), np.atleast_2d(data_mask))
    M = eng.M
    lnl, chi2 = np.empty((1, M)), np.empty((1, M))
    ndim = np.empty((1, M), dtype=np.int64)
    sc = se = None
    if free_scale and return_scale:
        sc, se = np.empty((1, M)), np.empty((1, M))
    opts = like_opts(dict(free_scale=free_scale, ignore_model_err=ignore_model_err,
                          dim_prior=dim_prior, ltol=ltol))
    eng.fit(obj.x, obj.xe, obj.xm, opts, lnl, chi2, ndim, sc, se)
    # in-place clean visible to the caller
    for dst, buf in ((data, obj.x), (data_err, obj.xe), (data_mask, obj.xm)):
        if isinstance(dst, np.ndarray) and not np.shares_memory(dst, buf):
            dst[...] = buf.reshape(dst.shape)
    nd = ndim[0].astype(_ndim_dtype(data_mask, models_mask))
    if free_scale and return_scale:
        return lnl[0], nd, chi2[0], sc[0], se[0]
    return lnl[0], nd, chi2[0]


def logprob(data, data_err, data_mask, models, models_err, models_mask, free_scale=False,
            ignore_model_err=False, dim_prior=True, ltol=1e-4, return_scale=False, *args,
            **kwargs):
    """pdf.py:326-411: ``(lnprior=0, lnlike, lnprob, Ndim, chi2[, scale, scale_err])``."""
    res = loglike(data, data_err, data_mask, models, models_err, models_mask,
                  free_scale=free_scale, ignore_model_err=ignore_model_err, dim_prior=dim_prior,
                  ltol=ltol, return_scale=return_scale, *args, **kwargs)
    lnl = res[0]
    return (np.zeros_like(lnl), lnl, lnl.copy()) + tuple(res[1:])       # lnprob = lnlike + lnprior is a fresh array in the reference (pdf.py:405)


class logprob_prior(object):
    """``lprob_func`` with an additive ln-prior, passed as DATA so that it can run on
    the device (extension; the reference's hook is a Python callable returning
    ``(lnprior, lnlike, lnlike + lnprior, ...)`` per object -- bruteforce.py:193-199,
    demos/2 cell 69's ``lprob_bpz``).

    ``lnprior`` is a ``(P, Nmodel)`` float64 table of ln-prior rows (NumPy array or a
    device tensor exposing ``data_ptr()``; ``(Nmodel,)`` means one shared row) and
    ``rows`` the ``(Ndata,)`` row each object reads.  Without ``rows``: ``P == 1``
    broadcasts, ``P == Ndata`` is a dense per-object prior.  ``lprob_kwargs`` keep
    their meaning (free_scale, ignore_model_err, dim_prior, ltol).

    Pass an instance as ``lprob_func=`` to ``BruteForce`` / ``NearestNeighbors``.
    Calling it for one object with the reference's signature also works
    (``row=`` picks the table row)."""

    def __init__(self, lnprior, rows=None):
        if isinstance(lnprior, np.ndarray) or not hasattr(lnprior, "data_ptr"):
            lnprior = np.atleast_2d(np.ascontiguousarray(lnprior, dtype=np.float64))
        elif lnprior.dim() != 2 or not lnprior.is_contiguous() or lnprior.element_size() != 8:
            raise ValueError("a device ln-prior table must be a contiguous 2-D float64 tensor")
        self.table = lnprior
        self.P, self.M = int(lnprior.shape[0]), int(lnprior.shape[1])
        if rows is not None and (isinstance(rows, np.ndarray) or not hasattr(rows, "data_ptr")):
            rows = np.ascontiguousarray(rows, dtype=np.int64)
        self.rows = rows

    def chunk(self, lo, hi, Ndata):
        """the ``(table, P, rows)`` triple of objects [lo, hi) out of Ndata"""
        if self.rows is not None:
            if len(self.rows) != Ndata:
                raise ValueError("ln-prior `rows` has %d entries for %d objects" % (len(self.rows), Ndata))
            return self.table, self.P, self.rows[lo:hi]
        if self.P == 1:
            return self.table, 1, None
        if self.P != Ndata:
            raise ValueError("ln-prior table has %d rows for %d objects and no `rows`" % (self.P, Ndata))
        return self.table[lo:hi], hi - lo, None

    def __call__(self, data, data_err, data_mask, models, models_err, models_mask, row=0,
                 free_scale=False, ignore_model_err=False, dim_prior=True, ltol=1e-4,
                 return_scale=False, device=None):
        rows = np.array([row], dtype=np.int64)
        return _prior_one_object(self.M, (self.table, self.P, rows), data, data_err, data_mask, models, models_err,
                                 models_mask, free_scale, ignore_model_err, dim_prior, ltol, return_scale, device)


def _prior_one_object(Mtab, prior, data, data_err, data_mask, models, models_err, models_mask, free_scale,
                      ignore_model_err, dim_prior, ltol, return_scale, device):
    """one object through ``fz_fit_prior`` / ``fz_fit_prior_lerp`` with the reference's ``lprob_func`` return tuple; ``prior``
    is the engine's prior tuple for that object"""
    eng = get_engine(device)
    eng.upload_models(models, models_err, models_mask)
    if eng.M != Mtab:
        raise ValueError("ln-prior rows hold %d models, the model set %d" % (Mtab, eng.M))
    obj = HostObjects(np.atleast_2d(data), np.atleast_2d(data_err), np.atleast_2d(data_mask))
    M = eng.M
    lnp, lnl, lpr, chi2 = (np.empty((1, M)) for _ in range(4))
    ndim = np.empty((1, M), dtype=np.int64)
    sc = se = None
    if free_scale and return_scale:
        sc, se = np.empty((1, M)), np.empty((1, M))
    opts = like_opts(dict(free_scale=free_scale, ignore_model_err=ignore_model_err,
                          dim_prior=dim_prior, ltol=ltol))
    eng.fit_prior(obj.x, obj.xe, obj.xm, opts, prior, lnp, lnl, lpr, chi2, ndim, sc, se)
    for dst, buf in ((data, obj.x), (data_err, obj.xe), (data_mask, obj.xm)):
        if isinstance(dst, np.ndarray) and not np.shares_memory(dst, buf):
            dst[...] = buf.reshape(dst.shape)
    out = (lnp[0], lnl[0], lpr[0], ndim[0].astype(_ndim_dtype(data_mask, models_mask)), chi2[0])
    if free_scale and return_scale:
        out = out + (sc[0], se[0])
    return out


def lerp_cells(grid, coord):
    """Cell and fraction of every ``coord`` on the strictly ascending nodes ``grid`` (P >= 2): ``coord`` is clipped to the grid,
    ``r = clip(searchsorted(grid, coord, 'right') - 1, 0, P - 2)`` and ``f = (coord - grid[r]) / (grid[r + 1] - grid[r])``, so
    that the top node is ``(P - 2, 1.0)`` and row ``P`` is never read.  ``nan`` raises ``ValueError``."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    coord = np.atleast_1d(np.asarray(coord, dtype=np.float64))
    if grid.ndim != 1 or len(grid) < 2:
        raise ValueError("an interpolated prior needs a 1-D `grid` of at least 2 nodes")
    if not np.all(np.diff(grid) > 0):
        raise ValueError("`grid` must be strictly ascending (and free of nan)")
    if coord.ndim != 1:
        raise ValueError("`coord` must be one number per object")
    if np.isnan(coord).any():
        raise ValueError("`coord` holds nan: the interpolated prior is undefined there")
    c = np.clip(coord, grid[0], grid[-1])
    r = np.clip(np.searchsorted(grid, c, side='right') - 1, 0, len(grid) - 2).astype(np.int64)
    f = (c - grid[r]) / (grid[r + 1] - grid[r])
    return r, np.ascontiguousarray(f, dtype=np.float64)


class logprob_prior_lerp(object):
    """``lprob_func`` with a prior that is LINEAR along one per-object coordinate (extension; the BPZ prior P(z, t | m) of the
    reference's priors.py along the magnitude, ``priors.logprob_bpz``):

        lnprior[i][j] = ln((1 - f_i) table[r_i][j] + f_i table[r_i + 1][j])

    ``table`` is ``(P, Nmodel)`` float64 prior VALUES (not logarithms; NumPy array or a device tensor exposing
    ``data_ptr()``) on the ``P >= 2`` strictly ascending nodes ``grid``, ``coord`` the ``(Ndata,)`` coordinate of every object
    (clipped to the grid; ``nan`` raises ``ValueError``) and ``(r_i, f_i)`` its cell and fraction (``lerp_cells``).  A zero
    value gives ``-inf``, a negative or nan value ``nan``, like ``np.log``.

    Used like ``logprob_prior``; the one-object call takes ``index=``, the object's position in ``coord``."""

    def __init__(self, table, grid, coord):
        if isinstance(table, np.ndarray) or not hasattr(table, "data_ptr"):
            table = np.ascontiguousarray(table, dtype=np.float64)
            if table.ndim != 2:
                raise ValueError("the prior table must be 2-D (P, Nmodel)")
        elif table.dim() != 2 or not table.is_contiguous() or table.element_size() != 8:
            raise ValueError("a device prior table must be a contiguous 2-D float64 tensor")
        self.table = table
        self.P, self.M = int(table.shape[0]), int(table.shape[1])
        self.grid = np.ascontiguousarray(grid, dtype=np.float64)
        if self.grid.shape != (self.P,):
            raise ValueError("`grid` has shape %s for a table of %d rows" % (self.grid.shape, self.P))
        self.rows, self.frac = lerp_cells(self.grid, coord)

    def chunk(self, lo, hi, Ndata):
        """the ``(table, P, rows, frac)`` tuple of objects [lo, hi) out of Ndata"""
        if len(self.rows) != Ndata:
            raise ValueError("the prior's `coord` has %d entries for %d objects" % (len(self.rows), Ndata))
        return self.table, self.P, self.rows[lo:hi], self.frac[lo:hi]

    def __call__(self, data, data_err, data_mask, models, models_err, models_mask, index=0,
                 free_scale=False, ignore_model_err=False, dim_prior=True, ltol=1e-4,
                 return_scale=False, device=None):
        prior = (self.table, self.P, self.rows[index:index + 1].copy(), self.frac[index:index + 1].copy())
        return _prior_one_object(self.M, prior, data, data_err, data_mask, models, models_err, models_mask, free_scale,
                                 ignore_model_err, dim_prior, ltol, return_scale, device)


def sample_labels(idx, model_labels, model_label_errs=None, rstate=None):
    """Labels of posterior draws (extension; ``BruteForce.fit_sample`` / ``.sample``, docs/draws.md): ``model_labels[idx]`` for any
    label of the model set, afterwards, on the host; with ``model_label_errs`` AND ``rstate`` each value is jittered by
    ``N(0, err)`` of its model; ``nan`` where ``idx == -1`` (a row without a posterior)."""
    idx = np.asarray(idx)
    labels = np.asarray(model_labels, dtype=np.float64)
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError("`idx` must hold integer model indices")
    if idx.size and (idx.min() < -1 or idx.max() >= len(labels)):
        raise IndexError("`idx` holds an index outside [-1, %d)" % len(labels))
    bad = idx < 0
    safe = np.where(bad, 0, idx)
    out = labels[safe]
    if model_label_errs is not None and rstate is not None:
        out = rstate.normal(out, np.asarray(model_label_errs, dtype=np.float64)[safe])
    out[bad] = np.nan
    return out


def sparsify_logwt(logwt, Nkeep=256, wt_thresh=1e-3, device=None):
    """Sparse rows out of stored or foreign dense rows of ln-weights (extension; docs/sparse_fits.md): per row of ``logwt``
    ``(Ndata, Nmodel)`` (NumPy or a device array) the exact ``Nkeep`` largest entries among those with ``wt > wt_thresh * max(wt)``,
    as a ``sparse.SparseFits`` in which only ``fit_lnprob`` is set (NumPy arrays)."""
    from .sparse import SparseFits, check_keep
    lw = logwt if hasattr(logwt, "data_ptr") else np.ascontiguousarray(logwt, dtype=np.float64)
    if len(lw.shape) != 2 or (hasattr(lw, "data_ptr") and not (lw.element_size() == 8 and lw.is_contiguous())):
        raise ValueError("`logwt` must be a C-contiguous float64 (Ndata, Nmodel) array; got shape %s" % (tuple(lw.shape),))
    N, M = (int(v) for v in lw.shape)
    if M < 1:
        raise ValueError("`logwt` has rows without entries")
    W, lncut = check_keep(Nkeep, wt_thresh, M)
    nbr, cnt = np.full((N, W), -99, dtype=np.int64), np.zeros(N, dtype=np.int64)
    vals = np.full((N, W), -np.inf)
    lmap, levid, lnkept = np.zeros(N), np.zeros(N), np.zeros(N)
    if N:
        get_engine(device).sparsify_logwt(lw, W, lncut, nbr, cnt, vals=vals, lmap=lmap, levid=levid, lnkept=lnkept, n=N, M=M)
    return SparseFits(nbr, cnt, M, lmap, levid, lnkept, fit_lnprob=vals, device=device)


def _rows_arg(a, dtype, name):
    """a NumPy array made C-contiguous in ``dtype``, or a device array of 8-byte items used where it lies"""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        if (hasattr(a, "element_size") and a.element_size() != 8) or (hasattr(a, "is_contiguous") and not a.is_contiguous()):
            raise ValueError("`%s` on the device must be C-contiguous with 8-byte items" % name)
        return a
    return np.ascontiguousarray(a, dtype=dtype)


def posterior_moments(logwt, values, value_errs=None, value_mask=None, scale=None, neighbors=None, Nneighbors=None,
                      return_share=False, device=None):
    """Posterior mean and variance of per-model values under rows of ln-weights (extension; docs/predictive.md states the law).

    ``logwt`` ``(Ndata, W)``; with ``neighbors`` ``(Ndata, W)`` / ``Nneighbors`` ``(Ndata,)`` entry ``t`` of a row belongs to model
    ``neighbors[i, t]`` and only the first ``Nneighbors[i]`` count, without them the rows are dense (``W == Nmodel``).  ``values``
    ``(Nmodel, L)`` or ``(Nmodel,)`` (one column; the results are then ``(Ndata,)``), ``value_errs`` their standard deviations
    (added as the law of total variance), ``value_mask`` non-zero where a value is usable, ``scale`` ``(Ndata, W)`` a factor per
    entry.  Every array is NumPy or a device array.  Returns ``(mean, var)`` or ``(mean, var, share)``; ``share`` is the part of
    the row's weight that had a usable value.  A row without a posterior gives nan (share 0)."""
    if (neighbors is None) != (Nneighbors is None):
        raise ValueError("`neighbors` and `Nneighbors` come together")
    lw = _rows_arg(logwt, np.float64, "logwt")
    V = _rows_arg(values, np.float64, "values")
    one = len(V.shape) == 1
    if len(lw.shape) != 2 or len(V.shape) not in (1, 2):
        raise ValueError("`logwt` must be (Ndata, W) and `values` (Nmodel, L) or (Nmodel,)")
    N, W = (int(v) for v in lw.shape)
    M, L = int(V.shape[0]), (1 if one else int(V.shape[1]))
    Ve, Vm = _rows_arg(value_errs, np.float64, "value_errs"), _rows_arg(value_mask, np.float64, "value_mask")
    for a, name in ((Ve, "value_errs"), (Vm, "value_mask")):
        if a is not None and tuple(a.shape) != tuple(V.shape):
            raise ValueError("`%s` has shape %s, `values` %s" % (name, tuple(a.shape), tuple(V.shape)))
    sc = _rows_arg(scale, np.float64, "scale")
    nb, nn = _rows_arg(neighbors, np.int64, "neighbors"), _rows_arg(Nneighbors, np.int64, "Nneighbors")
    if sc is not None and tuple(sc.shape) != (N, W):
        raise ValueError("`scale` has shape %s, `logwt` %s" % (tuple(sc.shape), (N, W)))
    if nb is not None and (tuple(nb.shape) != (N, W) or tuple(nn.shape) != (N,)):
        raise ValueError("`neighbors` must have the shape of `logwt` and `Nneighbors` one entry per object")
    if nb is None and W != M:
        raise ValueError("dense rows have one entry per model: %d entries, %d models" % (W, M))
    if W < 1 or M < 1 or L < 1:
        raise ValueError("rows of %d entries over %d models and %d columns" % (W, M, L))
    mean, var = np.full((N, L), np.nan), np.full((N, L), np.nan)
    share = np.zeros((N, L)) if return_share else None
    get_engine(device).row_moments(lw, N, W, M, L, V, mean, var=var, share=share, value_errs=Ve, value_mask=Vm, scale=sc,
                                   neighbors=nb, nnbr=nn)
    out = (mean, var, share) if return_share else (mean, var)
    return tuple(a[:, 0] for a in out) if one else out


def gaussian(mu, std, x):
    """N(x | mu, std) on a grid (pdf.py:414-425) -- host helper used to build the
    dictionary tables."""
    d = (np.asarray(x) - mu) / std
    return np.exp(-0.5 * np.square(d)) / (math.sqrt(2.0 * math.pi) * std)


def gaussian_bin(mu, std, bins):
    """N(mu, std) integrated over the bins with edges ``bins`` (pdf.py:428-441): the ``len(bins) - 1`` differences of the CDF
    ``0.5 (1 + erf)`` at the edges -- host helper, the reference's arithmetic."""
    from scipy.special import erf
    dif = bins - mu
    y = dif / (np.sqrt(2) * std)
    cdf = 0.5 * (1. + erf(y))
    return cdf[1:] - cdf[:-1]


def _bins_rows(logwt, labels, label_errs, neighbors, Nneighbors, wt_thresh):
    """the arguments `posterior_bins` and `posterior_cdf` share, checked before any device call
    -> lw, y, s, nb, nn, N, W, M, lncut"""
    if (neighbors is None) != (Nneighbors is None):
        raise ValueError("`neighbors` and `Nneighbors` come together")
    lw = _rows_arg(logwt, np.float64, "logwt")
    y, s = _rows_arg(labels, np.float64, "labels"), _rows_arg(label_errs, np.float64, "label_errs")
    if len(lw.shape) != 2 or len(y.shape) != 1 or tuple(s.shape) != tuple(y.shape):
        raise ValueError("`logwt` must be (Ndata, W), `labels` and `label_errs` (Nmodel,)")
    N, W = (int(v) for v in lw.shape)
    M = int(y.shape[0])
    nb, nn = _rows_arg(neighbors, np.int64, "neighbors"), _rows_arg(Nneighbors, np.int64, "Nneighbors")
    if nb is not None and (tuple(nb.shape) != (N, W) or tuple(nn.shape) != (N,)):
        raise ValueError("`neighbors` must have the shape of `logwt` and `Nneighbors` one entry per object")
    if nb is None and W != M:
        raise ValueError("dense rows have one entry per model: %d entries, %d models" % (W, M))
    if W < 1 or M < 1:
        raise ValueError("rows of %d entries over %d models" % (W, M))
    wt = 0. if wt_thresh is None else float(wt_thresh)
    if not (0. <= wt < 1.):
        raise ValueError("`wt_thresh` must lie in [0, 1) (got %r)" % (wt_thresh,))
    return lw, y, s, nb, nn, N, W, M, (np.log(wt) if wt > 0. else -np.inf)


def posterior_bins(logwt, labels, label_errs, bins, neighbors=None, Nneighbors=None, wt_thresh=1e-3, normalize=True,
                   return_outside=False, out=None, device=None):
    """Probability per bin, P(e_k <= label < e_k+1 | data), of a Gaussian label kernel under rows of ln-weights (extension;
    docs/bins.md states the law): per row the entries with ``wt > wt_thresh * max(wt)`` (decided in ln space; 0 or None: every entry
    with a positive weight), each model's ``N(labels[j], label_errs[j])`` integrated exactly between the edges ``bins`` -- a
    difference of two error functions, no grid.  ``label_errs == 0`` is a point mass.

    ``logwt`` ``(Ndata, W)`` with ``neighbors`` / ``Nneighbors`` as in ``posterior_moments`` (without them dense rows,
    ``W == Nmodel``); ``bins`` the ``Nbins + 1 <= 257`` finite, strictly increasing edges.  Every array is NumPy or a device array.
    ``normalize`` divides each row by its sum over the bins (conditional on the range: what ``samplers.population_sampler`` and
    ``hierarchical_sampler`` take; nan when no mass lies inside).  Returns ``(Ndata, Nbins)``, with ``return_outside`` also the
    masses ``(below, above)`` of the range.  ``out``: a C-contiguous float64 ``(Ndata, Nbins)`` NumPy or device array, filled in
    place and returned.  A row without a posterior gives nan."""
    lw, y, s, nb, nn, N, W, M, lncut = _bins_rows(logwt, labels, label_errs, neighbors, Nneighbors, wt_thresh)
    e = _rows_arg(bins, np.float64, "bins")
    if len(e.shape) != 1 or int(e.shape[0]) < 2:
        raise ValueError("`bins` must be a 1-D array of at least 2 edges")
    E = int(e.shape[0])
    if E - 1 > BINS_MAX:
        raise NotImplementedError("%d bins, the limit is %d (FZ_BINS_MAX)" % (E - 1, BINS_MAX))
    if isinstance(e, np.ndarray) and not (np.isfinite(e).all() and (np.diff(e) > 0).all()):
        raise ValueError("`bins` must be finite and strictly increasing")
    if out is None:
        out = np.full((N, E - 1), np.nan)
    elif tuple(out.shape) != (N, E - 1) or _rows_arg(out, np.float64, "out") is not out:
        raise ValueError("`out` must be a C-contiguous float64 array of shape (Ndata, Nbins) = (%d, %d)" % (N, E - 1))
    below, above = (np.full(N, np.nan), np.full(N, np.nan)) if return_outside else (None, None)
    get_engine(device).row_bins(lw, N, W, M, y, s, e, E, out, lncut=lncut, normalize=normalize, below=below, above=above,
                                neighbors=nb, nnbr=nn)
    return (out, (below, above)) if return_outside else out


def _cdf_points(points, N):
    """the `points` conventions `posterior_cdf` and `posterior_scores` share -> x, P, per_object, one (a point per object)"""
    x = _rows_arg(points, np.float64, "points")
    shape = tuple(int(v) for v in x.shape)
    one = len(shape) == 1 and shape[0] == N
    if one:
        P, per_object = 1, True
    elif len(shape) == 1 or (len(shape) == 2 and shape[0] == 1 and N != 1):
        P, per_object = shape[-1], False
    elif len(shape) == 2 and shape[0] == N:
        P, per_object = shape[1], True
    else:
        raise ValueError("`points` must be (Ndata, P), (1, P), (P,) or (Ndata,); got %s for %d objects" % (shape, N))
    if P < 1:
        raise ValueError("`points` is empty")
    if P > BINS_MAX:
        raise NotImplementedError("%d points, the limit is %d (FZ_BINS_MAX)" % (P, BINS_MAX))
    if isinstance(x, np.ndarray) and not np.isfinite(x).all():
        raise ValueError("`points` must be finite")
    return x, P, per_object, one


def posterior_cdf(logwt, labels, label_errs, points, neighbors=None, Nneighbors=None, wt_thresh=1e-3, device=None):
    """The mixture CDF P(label <= x | data) of the same kernel, selection and normalisation as ``posterior_bins`` (extension;
    docs/bins.md).  ``points``: ``(Ndata, P)`` per object, ``(1, P)`` or ``(P,)`` shared by all objects -- ``P <= 256``, finite, in
    any order -- giving ``(Ndata, P)``; or ``(Ndata,)``, one point per object, giving ``(Ndata,)``: with the true labels of a
    validation sample that is its PIT.  (A 1-D array of exactly ``Ndata`` points is read as one per object; pass ``(1, P)`` to share
    it.)"""
    lw, y, s, nb, nn, N, W, M, lncut = _bins_rows(logwt, labels, label_errs, neighbors, Nneighbors, wt_thresh)
    x, P, per_object, pit = _cdf_points(points, N)
    cdf = np.full((N, P), np.nan)
    get_engine(device).row_cdf(lw, N, W, M, y, s, x, P, cdf, per_object=per_object, lncut=lncut, neighbors=nb, nnbr=nn)
    return cdf[:, 0] if pit else cdf


def posterior_quantiles(logwt, labels, label_errs, q, neighbors=None, Nneighbors=None, wt_thresh=1e-3, out=None, return_info=False,
                        device=None):
    """Quantiles of the mixture ``posterior_cdf`` inverts, without a grid (extension; docs/quantiles.md states the law): per row
    ``Q(p) = inf{x : C(x) >= p}`` under the selection and normalisation of ``posterior_bins``, found by a safeguarded Newton on the
    device to the resolution of float64 in ``C`` and in ``x``.  ``q``: the probabilities, each strictly inside (0, 1), shared by all
    objects, in any order, at most 256; a scalar gives ``(Ndata,)``, otherwise ``(Ndata, Q)``.  ``label_errs`` must be finite
    (``posterior_bins`` accepts ``inf``; a flat kernel has no quantile), 0 is a point mass.  ``out``: a C-contiguous float64
    ``(Ndata, Q)`` NumPy or device array, filled in place and returned.  ``return_info`` adds a dict with ``nskip`` (rows without a
    posterior: nan), ``nfail`` (solves that ended on the cap of 128 evaluations and returned their bracket midpoint; also a
    ``RuntimeWarning``) and ``niter`` (evaluations of the CDF in all)."""
    lw, y, s, nb, nn, N, W, M, lncut = _bins_rows(logwt, labels, label_errs, neighbors, Nneighbors, wt_thresh)
    one = not hasattr(q, "data_ptr") and np.ndim(q) == 0
    p = _rows_arg(np.atleast_1d(q) if not hasattr(q, "data_ptr") else q, np.float64, "q")
    if len(p.shape) != 1 or int(p.shape[0]) < 1:
        raise ValueError("`q` must be a scalar or a 1-D array of at least one probability")
    Q = int(p.shape[0])
    if Q > BINS_MAX:
        raise NotImplementedError("%d probabilities, the limit is %d (FZ_BINS_MAX)" % (Q, BINS_MAX))
    if isinstance(p, np.ndarray) and not ((p > 0.) & (p < 1.)).all():
        raise ValueError("`q` must lie strictly inside (0, 1)")
    if isinstance(y, np.ndarray) and not np.isfinite(y).all():
        raise ValueError("`labels` must be finite")
    if isinstance(s, np.ndarray) and not (np.isfinite(s) & (s >= 0.)).all():
        raise ValueError("`label_errs` must be finite and not negative (a flat kernel, inf, has no quantile)")
    if isinstance(y, np.ndarray) and isinstance(s, np.ndarray):
        with np.errstate(over='ignore'):
            bad = ~np.isfinite(np.abs(y) + 40. * s)
        if bad.any():
            raise ValueError("model %d: |label| + 40 label_err overflows" % int(np.argmax(bad)))
    if out is None:
        out = np.full((N, Q), np.nan)
    elif tuple(out.shape) != (N, Q) or _rows_arg(out, np.float64, "out") is not out:
        raise ValueError("`out` must be a C-contiguous float64 array of shape (Ndata, Q) = (%d, %d)" % (N, Q))
    nskip, nfail, niter = get_engine(device).row_quantiles(lw, N, W, M, y, s, p, Q, out, lncut=lncut, neighbors=nb, nnbr=nn)
    if nfail:
        import warnings
        warnings.warn("posterior_quantiles: %d solves ended on the cap of 128 evaluations and return their bracket midpoint" % nfail,
                      RuntimeWarning, stacklevel=2)
    res = out[:, 0] if (one and isinstance(out, np.ndarray)) else out
    return (res, dict(nskip=nskip, nfail=nfail, niter=niter)) if return_info else res


SCORES_NMAX = 16384  # FZ_SCORES_NMAX: included entries of a row whose pair sums (crps, spread, sqnorm) are asked for
_SCORES = ('lnpdf', 'crps', 'spread', 'sqnorm', 'ninc')


def posterior_scores(logwt, labels, label_errs, points, neighbors=None, Nneighbors=None, wt_thresh=1e-3, want=('lnpdf', 'crps', 'sqnorm'),
                     return_info=False, device=None):
    """Scoring rules of the mixture ``posterior_cdf`` evaluates, in closed form and without a grid (extension; docs/scores.md states
    the law): under the selection and normalisation of ``posterior_bins``, per row and point ``x``

    * ``lnpdf``  the ln-density at ``x`` (the log score), formed in ln space;
    * ``crps``   the continuous ranked probability score ``E|X - x| - E|X - X'| / 2``;
    * ``spread`` its second term ``E|X - X'| / 2``, per row;
    * ``sqnorm`` the integral of the squared density, per row (the CDE loss is ``sqnorm - 2 exp(lnpdf)``);
    * ``ninc``   the number of included entries, per row (int64).

    ``points`` as in ``posterior_cdf``: ``(Ndata, P)``, ``(1, P)`` or ``(P,)`` with ``P <= 256``, or ``(Ndata,)``, one point per
    object -- the true labels of a validation sample -- giving ``(Ndata,)`` for ``lnpdf`` and ``crps``.  ``labels`` and ``points``
    must be finite, ``label_errs`` finite and not negative; 0 is a point mass (``sqnorm`` is then ``inf``, ``lnpdf`` ``inf`` at the
    label itself).  ``want`` names the results to form; ``crps``, ``spread`` and ``sqnorm`` sum over all pairs of a row's included
    entries, and a row with more than 16384 of them (``SCORES_NMAX``) is refused with ``NotImplementedError``.  Returns a dict of
    arrays, with ``return_info`` also a dict with ``nskip`` (rows without a posterior: nan)."""
    lw, y, s, nb, nn, N, W, M, lncut = _bins_rows(logwt, labels, label_errs, neighbors, Nneighbors, wt_thresh)
    x, P, per_object, one = _cdf_points(points, N)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(k not in _SCORES for k in want):
        raise ValueError("`want` names results among %s (got %r)" % (", ".join(_SCORES), want))
    if isinstance(y, np.ndarray) and not np.isfinite(y).all():
        raise ValueError("`labels` must be finite")
    if isinstance(s, np.ndarray) and not (np.isfinite(s) & (s >= 0.)).all():
        raise ValueError("`label_errs` must be finite and not negative (a flat kernel, inf, has no finite score)")
    out = {k: (np.zeros(N, dtype=np.int64) if k == 'ninc' else np.full((N, P) if k in ('lnpdf', 'crps') else N, np.nan))
           for k in _SCORES if k in want}
    nskip = get_engine(device).row_scores(lw, N, W, M, y, s, x, P, per_object=per_object, lncut=lncut, neighbors=nb, nnbr=nn, **out)
    if one:
        out = {k: (v[:, 0] if k in ('lnpdf', 'crps') else v) for k, v in out.items()}
    return (out, dict(nskip=nskip)) if return_info else out


class PDFDict(object):
    """Grid + dictionary of truncated Gaussian kernels (pdf.py:778-852).  Same
    attributes as the reference: ``Ngrid, min, max, delta, grid, Ndict, sigma_grid,
    dsigma, sigma_width, sigma_dict, sigma_dict_cdf`` and ``fit``."""

    def __init__(self, pdf_grid, sigma_grid, sigma_trunc=5.):
        self.Ngrid = len(pdf_grid)
        self.min, self.max = min(pdf_grid), max(pdf_grid)
        self.delta = pdf_grid[1] - pdf_grid[0]
        self.grid = np.array(pdf_grid)
        self.Ndict = len(sigma_grid)
        self.sigma_grid = np.array(sigma_grid)
        self.dsigma = sigma_grid[1] - sigma_grid[0]
        # half-widths in grid cells; the slice below is taken literally so entries
        # wider than half the grid come out malformed just like pdf.py:814-816
        self.sigma_width = np.ceil(self.sigma_grid * sigma_trunc / self.delta).astype('int')
        mid = int(self.Ngrid / 2)
        self.sigma_dict = []
        self.sigma_dict_cdf = []
        for s, w in zip(self.sigma_grid, self.sigma_width):
            k = gaussian(self.grid[mid], s, self.grid[mid - w:mid + w + 1])
            self.sigma_dict.append(k)
            self.sigma_dict_cdf.append(np.cumsum(k))

    def fit(self, X, Xe):
        """(value, error) -> (grid index, dictionary index) (pdf.py:843-852): mean
        index by round-half-even and NOT clamped; error index clamped."""
        X, Xe = np.asarray(X), np.asarray(Xe)
        X_idx = ((X - self.grid[0]) / self.delta).round().astype('int')
        Xe_idx = np.array(np.round((Xe - self.sigma_grid[0]) / self.dsigma), dtype='int')
        np.clip(Xe_idx, 0, self.Ndict - 1, out=Xe_idx)
        return X_idx, Xe_idx


def gauss_kde(y, y_std, x, dx=None, y_wt=None, sig_thresh=5., wt_thresh=1e-3, cdf_thresh=2e-4,
              device=None, *args, **kwargs):
    """Direct weighted Gaussian KDE on grid ``x`` (pdf.py:444-526), un-normalised."""
    eng = get_engine(device)
    y = np.asarray(y, dtype=float)
    wt = np.ones(len(y)) if y_wt is None else np.ascontiguousarray(y_wt, dtype=np.float64)
    if wt.shape != (len(y),) or len(np.atleast_1d(y_std)) != len(y):
        raise ValueError("`y`, `y_std` and `y_wt` must have the same length")
    eng.upload_labels_grid(y, y_std, x, dx=dx, sig_thresh=sig_thresh)
    out = np.empty((1, len(x)))
    ko = kde_opts(dict(wt_thresh=wt_thresh, cdf_thresh=cdf_thresh), normalize=False)
    eng.predict_logwt(wt.reshape(1, -1), ko, out, is_log=False)
    return out[0]


def gauss_kde_dict(pdfdict, y=None, y_std=None, y_idx=None, y_std_idx=None, y_wt=None,
                   wt_thresh=1e-3, cdf_thresh=2e-4, device=None, *args, **kwargs):
    """Dictionary KDE (pdf.py:529-622), un-normalised."""
    if y_idx is not None and y_std_idx is not None:
        pass
    elif y is not None and y_std is not None:
        y_idx, y_std_idx = pdfdict.fit(y, y_std)
    else:
        raise ValueError("At least one pair of (`y`, `y_std`) or (`y_idx`, `y_idx_std`) must "
                         "be specified.")
    eng = get_engine(device)
    wt = np.ones(len(y_idx)) if y_wt is None else np.ascontiguousarray(y_wt, dtype=np.float64)
    if wt.shape != (len(y_idx),) or len(y_std_idx) != len(y_idx):
        raise ValueError("`y_idx`, `y_std_idx` and `y_wt` must have the same length")
    eng.upload_dict(pdfdict)
    eng.upload_labels_dict(y_idx, y_std_idx)
    out = np.empty((1, pdfdict.Ngrid))
    ko = kde_opts(dict(wt_thresh=wt_thresh, cdf_thresh=cdf_thresh), normalize=False)
    eng.predict_logwt(wt.reshape(1, -1), ko, out, is_log=False)
    return out[0]


def magnitude(phot, err, zeropoints=1., *args, **kwargs):
    """AB magnitudes and errors (pdf.py:625-657); k-NN feature map."""
    phot, err = np.asarray(phot), np.asarray(err)
    return -2.5 * np.log10(phot / zeropoints), 2.5 / math.log(10.) * err / phot


def luptitude(phot, err, skynoise=1., zeropoints=1., *args, **kwargs):
    """asinh magnitudes and errors (pdf.py:695-734); the default k-NN feature map."""
    phot, err = np.asarray(phot), np.asarray(err)
    mag = -2.5 / math.log(10.) * (np.arcsinh(phot / (2. * skynoise)) + np.log(skynoise / zeropoints))
    mag_err = np.sqrt(np.square(2.5 * np.log10(np.e) * err)
                      / (np.square(2. * skynoise) + np.square(phot)))
    return mag, mag_err


def _default_wconf(point):
    return (1. + point) * 0.03


def pdfs_summarize(pdfs, pgrid, renormalize=True, rstate=None, pkern='lorentz', pkern_grid=None,
                   wconf_func=None, device=None):
    """PDF summary statistics (pdf.py:899-1074): mean / median / mode / "best" estimators
    with their std, conf and risk, the 68 % / 95 % credible bounds and a Monte-Carlo
    draw.  Same signature and return tuple as the reference; ``pdfs`` is renormalised
    in place.  The (G,G) loss kernel is a host-side table (pdf.py:1003-1023); the
    (N,G)x(G,G) risk product, the CDFs and every per-object reduction run on the GPU.
    A custom ``wconf_func`` is evaluated on the host (once per estimator and object,
    like the reference) between two device passes."""
    if rstate is None:
        rstate = np.random
    if not isinstance(pdfs, np.ndarray) or pdfs.dtype != np.float64 or not pdfs.flags.c_contiguous:
        raise ValueError("`pdfs` must be a C-contiguous float64 array (it is renormalised in place)")
    pgrid_a = np.ascontiguousarray(pgrid, dtype=np.float64)
    Nobj, Ngrid = len(pdfs), len(pgrid_a)
    if pdfs.shape != (Nobj, Ngrid):
        raise ValueError("`pdfs` must have shape (Npdf, len(pgrid))")
    # kernel over (truth, guess) pairs, exactly as pdf.py:1003-1023
    if pkern_grid is None:
        ptrue = pgrid_a.reshape(Ngrid, 1)
        pguess = pgrid_a.reshape(1, Ngrid)
        pkern_grid = (ptrue - pguess) / ((1. + ptrue) * 0.15)
    if isinstance(pkern, str) and pkern == 'tophat':
        kernel = (np.square(pkern_grid) < 1.)
    elif isinstance(pkern, str) and pkern == 'gaussian':
        kernel = np.exp(-0.5 * np.square(pkern_grid))
    elif isinstance(pkern, str) and pkern == 'lorentz':
        kernel = 1. / (1. + np.square(pkern_grid))
    else:
        try:
            kernel = pkern(pkern_grid)
        except Exception:
            raise RuntimeError("The input kernel does not appear to be valid.")
    loss = np.ascontiguousarray(1.0 - kernel, dtype=np.float64)
    urand = np.array([rstate.rand() for _ in range(Nobj)], dtype=np.float64)      # pdf.py:1000, one draw per object
    eng = get_engine(device)
    stats = np.empty((21, Nobj))
    eng.pdfs_summarize(pdfs, pgrid_a, renormalize, urand, loss, None, 0.03, stats)
    if wconf_func is not None:
        widths = np.array([[wconf_func(stats[4 * e, i]) for e in range(4)] for i in range(Nobj)], dtype=np.float64)
        eng.pdfs_summarize(pdfs, pgrid_a, False, urand, loss, np.ascontiguousarray(widths), 0.03, stats)
    s = stats
    return ((s[0], s[1], s[2], s[3]), (s[4], s[5], s[6], s[7]), (s[8], s[9], s[10], s[11]),
            (s[12], s[13], s[14], s[15]), (s[16], s[17], s[18], s[19]), s[20])


def pdfs_resample(pdfs, old_grid, new_grid, renormalize=True, left=0., right=0., device=None):
    """Resample PDFs onto a new grid (pdf.py:855-896: ``numpy.interp`` per row, then an
    optional renormalisation to unit sum)."""
    og = np.ascontiguousarray(old_grid, dtype=np.float64)
    ng = np.ascontiguousarray(new_grid, dtype=np.float64)
    if isinstance(pdfs, np.ndarray) or not hasattr(pdfs, "data_ptr"):
        pdfs = np.ascontiguousarray(pdfs, dtype=np.float64)
    out = np.empty((len(pdfs), len(ng)))
    get_engine(device).pdfs_resample(pdfs, og, ng, left, right, renormalize, out, n=len(pdfs))
    return out
