"""
Thin object wrapper over one ``fz_ctx`` (one per GPU).  Everything numeric happens
inside libfrankenz_hip.so; this file only marshals arrays.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import KdeOpts, LikeOpts, Prior, PriorLerp, Timing, check, ptr

# the reference's logprob keywords + one extension: exact_evidence=True sums every weight of the fused path's
# ln-evidence in fp64 (default: the weights below wt_thresh of the best are summed in fp32, ~1e-9 on levid)
_LIKE_KEYS = ("free_scale", "ignore_model_err", "dim_prior", "ltol", "return_scale", "exact_evidence")


def like_opts(lprob_kwargs, max_iter=0):
    """lprob_kwargs of pdf.logprob (pdf.py:326-328) -> fz_like_opts."""
    kw = dict(lprob_kwargs or {})
    extra = set(kw) - set(_LIKE_KEYS)
    if extra:
        raise NotImplementedError(
            "lprob_kwargs %s are not understood by the HIP likelihood "
            "(supported: %s)" % (sorted(extra), ", ".join(_LIKE_KEYS)))
    return LikeOpts(int(bool(kw.get("free_scale", False))),
                    int(bool(kw.get("ignore_model_err", False))),
                    int(bool(kw.get("dim_prior", True))), int(max_iter),
                    float(kw.get("ltol", 1e-4)), int(bool(kw.get("exact_evidence", False))), 0)


def merge_kde_args(kde_args, kde_kwargs, use_dict):
    """Positional ``kde_args`` of predict / fit_predict, as the reference hands them on (bruteforce.py:361-369):
    ``gauss_kde_dict(label_dict, y_idx=.., y_std_idx=.., y_wt=wt, *kde_args, **kde_kwargs)`` -- up to two positionals land
    on ``y`` / ``y_std``, which the function ignores when the indices are given (pdf.py:570-573), a third collides with
    ``y_idx``; ``gauss_kde(labels, label_errs, grid, y_wt=wt, *kde_args, **kde_kwargs)`` -- the first positional is ``dx``,
    a second collides with ``y_wt``.  Returns the keyword dict to use; raises the TypeError Python raises for the rest."""
    kw = dict(kde_kwargs or {})
    args = tuple(kde_args or ())
    if use_dict:
        if len(args) > 2:
            raise TypeError("gauss_kde_dict() got multiple values for argument 'y_idx'")
        return kw
    if len(args) > 1:
        raise TypeError("gauss_kde() got multiple values for argument 'y_wt'")
    if len(args) == 1:
        if 'dx' in kw:
            raise TypeError("gauss_kde() got multiple values for argument 'dx'")
        kw['dx'] = args[0]
    return kw


def kde_opts(kde_kwargs, normalize=True):
    """kde_kwargs of gauss_kde / gauss_kde_dict -> fz_kde_opts.  ``wt_thresh=None``
    with ``cdf_thresh=None`` means no thresholding (pdf.py:495-496, 578-579)."""
    kw = dict(kde_kwargs or {})
    wt = kw.pop("wt_thresh", 1e-3)
    cdf = kw.pop("cdf_thresh", 2e-4)
    ex = int(bool(kw.pop("exact_evidence", False)))         # extension: the whole logsumexp in fp64
    kw.pop("sig_thresh", None)
    kw.pop("dx", None)
    if kw:
        raise NotImplementedError("kde_kwargs %s are not supported" % sorted(kw))
    if wt is None and cdf is None:
        return KdeOpts(-np.inf, 1, int(normalize), 0.0, ex, 0)
    if wt is None:
        return KdeOpts(0.0, 0, int(normalize), float(cdf), ex, 0)
    return KdeOpts(float(wt), 1, int(normalize), 0.0 if cdf is None else float(cdf), ex, 0)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


try:
    import xxhash as _xx

    def _hash_bytes(h, a):
        h.update(memoryview(a).cast('B'))

    def _new_hash():
        return _xx.xxh3_128()
except ImportError:                                   # pragma: no cover  (xxhash ships with the image)
    import hashlib as _hl

    def _hash_bytes(h, a):
        h.update(memoryview(a).cast('B'))

    def _new_hash():
        return _hl.blake2b(digest_size=16)


def _digest(*arrays):
    """(shapes, 128-bit content hash) of C-contiguous arrays: the key under which an upload is remembered"""
    h = _new_hash()
    for a in arrays:
        if a.size:
            _hash_bytes(h, a)
    return (tuple(a.shape for a in arrays), h.hexdigest())


class _PinnedBlock(object):
    """A page-locked host block (fz_host_alloc) behind ``__array_interface__``: the NumPy array made from it keeps it alive
    as its base; when the last view dies the block goes back to a small pool (page-locking 5.6 GB costs about as much
    as copying it) or to the runtime."""
    _pool = []                      # free blocks [(nbytes, ptr)], at most _POOL_MAX bytes in total
    # One result block of the largest call so far stays page-locked between calls (page-locking 5.6 GB costs about as much as
    # copying it); FRANKENZ_PINNED_POOL_GB sizes the pool (0: nothing is kept), ``release_pinned_pool()`` empties it.
    _POOL_MAX = int(float(os.environ.get("FRANKENZ_PINNED_POOL_GB", "6")) * (1 << 30))

    def __init__(self, ptr_, nbytes, shape, dtype):
        self.ptr, self.nbytes = ptr_, nbytes
        self.__array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str, "data": (ptr_, False), "version": 3}

    def __del__(self):
        try:
            pool = _PinnedBlock._pool
            if sum(b[0] for b in pool) + self.nbytes <= _PinnedBlock._POOL_MAX:
                pool.append((self.nbytes, self.ptr))
            else:
                _lib.load().fz_host_free(self.ptr)
        except Exception:           # interpreter shutdown
            pass


def release_pinned_pool():
    """give every pooled page-locked block back to the runtime (hosts short of unswappable memory, several ranks per node)"""
    pool = _PinnedBlock._pool
    while pool:
        _lib.load().fz_host_free(pool.pop()[1])


def pinned_empty(shape, dtype=np.float64, min_bytes=1 << 24):
    """Uninitialised result array in page-locked host memory (arrays below ``min_bytes`` and any allocation the runtime
    refuses: ordinary ``np.empty``).  A device-to-host copy into pageable memory is staged by the runtime (~14 GB/s
    measured, and it blocks the host); into page-locked memory it runs at the link rate behind the next chunk's kernel."""
    shape = tuple(int(v) for v in np.atleast_1d(shape)) if not isinstance(shape, tuple) else tuple(int(v) for v in shape)
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    if nbytes < min_bytes:
        return np.empty(shape, dtype=dtype)
    pool = _PinnedBlock._pool
    best = None
    for k, (nb, _) in enumerate(pool):          # smallest free block that fits without wasting more than half of itself
        if nbytes <= nb <= 2 * nbytes and (best is None or nb < pool[best][0]):
            best = k
    if best is not None:
        nb, p = pool.pop(best)
    else:
        h = C.c_void_p()
        if _lib.load().fz_host_alloc(nbytes, C.byref(h)) != 0:
            while pool:                         # make room once, then give up on page-locking
                _lib.load().fz_host_free(pool.pop()[1])
            if _lib.load().fz_host_alloc(nbytes, C.byref(h)) != 0:
                return np.empty(shape, dtype=dtype)
        nb, p = nbytes, h.value
    return np.asarray(_PinnedBlock(p, nb, shape, dtype))


class Engine(object):
    """One device context.  Not thread-safe."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.fz_ctx_create(int(device), C.byref(h)))
        self.h = h
        self.device = int(device)
        self.M = self.B = 0
        self._models_key = self._dict_key = self._labels_key = self._trees_key = None      # content keys of what the device holds

    def close(self):
        if getattr(self, "h", None):
            self.lib.fz_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- uploads ----------------------------------------------------------
    # What is already on the device is not sent again.  The reference holds REFERENCES to the caller's model
    # arrays (bruteforce.py:54-56), so an in-place edit between two calls must be seen: the key is a hash of the
    # bytes (xxh3: ~1 ms per 12 MB), not the arrays' identity.
    def upload_models(self, models, models_err, models_mask):
        y, ye, ym = _f64(models), _f64(models_err), _f64(models_mask)
        if y.ndim != 2 or ye.shape != y.shape or ym.shape != y.shape:
            raise ValueError("models, models_err, models_mask must share a (Nmodel, Nfilt) shape")
        key = _digest(y, ye, ym)
        if key == self._models_key:
            return
        self._models_key = self._labels_key = None              # labels belong to the model set they were uploaded with
        check(self.lib.fz_models_upload(self.h, ptr(y), ptr(ye), ptr(ym), y.shape[0], y.shape[1]))
        self.M, self.B = y.shape
        self._models_key = key

    def upload_dict(self, pdfdict):
        lens = np.array([len(k) for k in pdfdict.sigma_dict], dtype=np.int64)
        offs = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=offs[1:])
        kern = _f64(np.concatenate(pdfdict.sigma_dict))
        kcdf = _f64(np.concatenate(pdfdict.sigma_dict_cdf))
        widths = np.ascontiguousarray(pdfdict.sigma_width, dtype=np.int64)
        key = (int(pdfdict.Ngrid),) + _digest(widths, offs, kern, kcdf)
        if key == self._dict_key:
            return
        self._dict_key = self._labels_key = None
        check(self.lib.fz_kdedict_upload(self.h, int(pdfdict.Ngrid), len(lens), ptr(widths),
                                         ptr(offs), ptr(kern), ptr(kcdf)))
        self._dict_key = key

    def upload_labels_dict(self, y_idx, y_std_idx):
        yi = np.ascontiguousarray(y_idx, dtype=np.int64)
        si = np.ascontiguousarray(y_std_idx, dtype=np.int64)
        key = ("dict", self._dict_key, self._models_key) + _digest(yi, si)
        if key == self._labels_key and self._dict_key is not None:
            return
        self._labels_key = None
        check(self.lib.fz_labels_upload_dict(self.h, ptr(yi), ptr(si), len(yi)))
        self._labels_key = key

    def upload_labels_grid(self, y, y_std, grid, dx=None, sig_thresh=5.0):
        y, ys, g = _f64(y), _f64(y_std), _f64(grid)
        if dx is None:
            dx = g[1] - g[0]
        key = ("grid", float(dx), float(sig_thresh), self._models_key) + _digest(y, ys, g)
        if key == self._labels_key:
            return
        self._labels_key = None              # (the library restores the dictionary's grid length itself when dictionary labels return)
        check(self.lib.fz_labels_upload_grid(self.h, ptr(y), ptr(ys), len(y), ptr(g), len(g),
                                             float(dx), float(sig_thresh)))
        self._labels_key = key

    def set_labels(self, labels, label_errs, label_dict=None, label_grid=None, kde_kwargs=None):
        """bruteforce.py:598-599 / 361-369: dictionary path if a PDFDict is given,
        else the direct KDE on ``label_grid``.  Returns Nx."""
        if label_dict is None and label_grid is None:
            raise ValueError("`label_dict` or `label_grid` must be specified.")
        kw = kde_kwargs or {}
        if label_dict is not None:
            yi, si = label_dict.fit(np.asarray(labels), np.asarray(label_errs))
            self.upload_dict(label_dict)
            self.upload_labels_dict(yi, si)
            return label_dict.Ngrid
        self.upload_labels_grid(labels, label_errs, label_grid, dx=kw.get("dx"),
                                sig_thresh=kw.get("sig_thresh", 5.0))
        return len(label_grid)

    # -- compute ----------------------------------------------------------
    def fit(self, x, xe, xm, opts, lnlike=None, chi2=None, ndim=None, scale=None, scale_err=None,
            n=None):
        n = len(x) if n is None else n
        check(self.lib.fz_fit(self.h, ptr(x), ptr(xe), ptr(xm), n, C.byref(opts), ptr(lnlike),
                              ptr(chi2), ptr(ndim), ptr(scale), ptr(scale_err)))

    def fit_predict(self, x, xe, xm, opts, kopts, pdfs, lmap=None, levid=None, n=None):
        n = len(x) if n is None else n
        check(self.lib.fz_fit_predict(self.h, ptr(x), ptr(xe), ptr(xm), n, C.byref(opts),
                                      C.byref(kopts), ptr(pdfs), ptr(lmap), ptr(levid)))

    @staticmethod
    def _prior_struct(prior):
        """(table, P, rows) -> ("", fz_prior*) or ("", NULL); (table, P, rows, frac) -> ("_lerp", fz_prior_lerp*): the suffix of
        the entry point that takes the struct.  The arrays must outlive the call."""
        if prior is None:
            return "", None
        if len(prior) == 4:
            table, P, rows, frac = prior
            return "_lerp", C.byref(PriorLerp(ptr(table), int(P), ptr(rows), ptr(frac)))
        table, P, rows = prior
        return "", C.byref(Prior(ptr(table), int(P), ptr(rows)))

    def fit_prior(self, x, xe, xm, opts, prior, lnprior=None, lnlike=None, lnprob=None, chi2=None,
                  ndim=None, scale=None, scale_err=None, n=None):
        """fz_fit_prior: ``prior`` is ``(table (P,M), P, rows (n,) or None)`` or None; with a fourth entry ``frac (n,)`` it is
        the interpolated form (fz_fit_prior_lerp)."""
        n = len(x) if n is None else n
        sfx, ps = self._prior_struct(prior)
        check(getattr(self.lib, "fz_fit_prior" + sfx)(self.h, ptr(x), ptr(xe), ptr(xm), n, C.byref(opts),
                                                      ps, ptr(lnprior), ptr(lnlike), ptr(lnprob),
                                                      ptr(chi2), ptr(ndim), ptr(scale), ptr(scale_err)))

    def fit_predict_prior(self, x, xe, xm, opts, kopts, prior, pdfs, lmap=None, levid=None, n=None):
        n = len(x) if n is None else n
        sfx, ps = self._prior_struct(prior)
        check(getattr(self.lib, "fz_fit_predict_prior" + sfx)(self.h, ptr(x), ptr(xe), ptr(xm), n, C.byref(opts),
                                                              C.byref(kopts), ps, ptr(pdfs), ptr(lmap), ptr(levid)))

    def prior_rows_from_grid(self, base, iz, g, t, table):
        """fz_prior_rows_from_grid: ``base`` (P, NZ, NT) float64, ``iz`` / ``t`` (M,) int32, ``g`` (M,) float64 -> the device
        ``table`` (P, M)."""
        P, NZ, NT = base.shape
        check(self.lib.fz_prior_rows_from_grid(self.h, ptr(base), P, NZ, NT, ptr(iz), ptr(g), ptr(t), len(iz), ptr(table)))

    def predict_logwt(self, logwt, kopts, pdfs, lmap=None, levid=None, is_log=True, n=None):
        n = len(logwt) if n is None else n
        check(self.lib.fz_predict_logwt(self.h, ptr(logwt), n, int(bool(is_log)), C.byref(kopts),
                                        ptr(pdfs), ptr(lmap), ptr(levid)))

    # -- posterior draws over the model set (docs/draws.md; fz_draw.h) -----------
    @staticmethod
    def _draw_source(u, key):
        """the uniforms of a draw call: the caller's ``u`` (N, S), or a two-word Philox ``key`` -> (u pointer, key0, key1)"""
        if u is None and key is None:
            raise ValueError("posterior draws need uniforms `u` or a Philox `key`")
        k0, k1 = (0, 0) if key is None else (int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF)
        return ptr(u), k0, k1

    @staticmethod
    def _prior_lerp_struct(prior):
        """(table, P, rows[, frac]) -> fz_prior_lerp* (frac NULL: a plain ln table), or NULL"""
        if prior is None:
            return None
        return C.byref(PriorLerp(ptr(prior[0]), int(prior[1]), ptr(prior[2]), ptr(prior[3]) if len(prior) == 4 else None))

    def draw_logwt(self, logwt, S, idx, u=None, key=None, first=0, neighbors=None, nnbr=None, lmap=None, levid=None, n=None, W=None):
        """fz_draw_logwt: ``S`` draws per row of ``logwt`` (n, W) into ``idx`` (n, S) int64; ``neighbors`` / ``nnbr``: the k-NN
        form (valid entries per row, and the model index returned for each)"""
        n = len(logwt) if n is None else n
        W = logwt.shape[1] if W is None else W
        up, k0, k1 = self._draw_source(u, key)
        check(self.lib.fz_draw_logwt(self.h, ptr(logwt), int(n), int(W), ptr(neighbors), ptr(nnbr), up, k0, k1, int(first), int(S),
                                     ptr(idx), ptr(lmap), ptr(levid)))

    def fit_draw(self, x, xe, xm, opts, prior, S, idx, u=None, key=None, first=0, lmap=None, levid=None, n=None):
        """fz_fit_draw: objects -> ``S`` draws each over the uploaded model set; ``prior`` as in ``fit_prior``"""
        n = len(x) if n is None else n
        up, k0, k1 = self._draw_source(u, key)
        check(self.lib.fz_fit_draw(self.h, ptr(x), ptr(xe), ptr(xm), int(n), C.byref(opts), self._prior_lerp_struct(prior), up, k0, k1,
                                   int(first), int(S), ptr(idx), ptr(lmap), ptr(levid)))

    def knn_search_fit_draw(self, q, x, xe, xm, k, lp_norm, distance_upper_bound, opts, prior, S, idx, u=None, key=None, first=0,
                            neighbors=None, nnbr=None, lmap=None, levid=None, n=None):
        """fz_knn_search_fit_draw: the K searches, the subset likelihood and ``S`` draws (model indices) per object"""
        n = len(x) if n is None else n
        up, k0, k1 = self._draw_source(u, key)
        check(self.lib.fz_knn_search_fit_draw(self.h, ptr(q), ptr(x), ptr(xe), ptr(xm), int(n), int(k), float(lp_norm),
                                              float(distance_upper_bound), C.byref(opts), self._prior_lerp_struct(prior), up, k0, k1,
                                              int(first), int(S), ptr(neighbors), ptr(nnbr), ptr(idx), ptr(lmap), ptr(levid)))

    # -- sparse rows out of an exhaustive fit (docs/sparse_fits.md; fz_sparse.h) ----
    def sparsify_logwt(self, logwt, W, lncut, neighbors, nnbr, vals=None, lmap=None, levid=None, lnkept=None, n=None, M=None):
        """fz_sparsify_logwt: per row of ``logwt`` (n, M) the ``W`` largest entries within ``lncut`` of its max -> ``neighbors``
        (n, W) int64, ``nnbr`` (n) int64 [, ``vals`` (n, W), ``lmap`` / ``levid`` of the full row, ``lnkept``]"""
        n = len(logwt) if n is None else n
        M = logwt.shape[1] if M is None else M
        check(self.lib.fz_sparsify_logwt(self.h, ptr(logwt), int(n), int(M), int(W), float(lncut), ptr(neighbors), ptr(nnbr), ptr(vals),
                                         ptr(lmap), ptr(levid), ptr(lnkept)))

    def fit_sparse(self, x, xe, xm, opts, prior, W, lncut, neighbors, nnbr, lnprior=None, lnlike=None, lnprob=None, chi2=None, ndim=None,
                   scale=None, scale_err=None, lmap=None, levid=None, lnkept=None, n=None):
        """fz_fit_sparse: objects -> the ``W`` best models each of the uploaded set, in the k-NN layout; ``prior`` as in ``fit_prior``"""
        n = len(x) if n is None else n
        check(self.lib.fz_fit_sparse(self.h, ptr(x), ptr(xe), ptr(xm), int(n), C.byref(opts), self._prior_lerp_struct(prior), int(W),
                                     float(lncut), ptr(neighbors), ptr(nnbr), ptr(lnprior), ptr(lnlike), ptr(lnprob), ptr(chi2), ptr(ndim),
                                     ptr(scale), ptr(scale_err), ptr(lmap), ptr(levid), ptr(lnkept)))

    # -- Gibbs over model weights (docs/model_weights.md; fz_mw.h) ----------------
    def mw_sweep(self, rows, n, W, M, lnw, counts, u=None, key=None, first=0, sweep=0, neighbors=None, nnbr=None, assign=None):
        """fz_mw_sweep: one draw per row of ``rows + lnw[neighbors]`` -> ``counts`` (M) int64 [and ``assign`` (n) int64]"""
        up, k0, k1 = self._draw_source(u, key)
        check(self.lib.fz_mw_sweep(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(lnw), up, k0, k1, int(first),
                                   int(sweep), ptr(counts), ptr(assign)))

    def mw_dirichlet(self, alpha, counts, M, key, sweep, pos, lnw):
        """fz_mw_dirichlet: ``pos ~ Dirichlet(alpha + counts)`` and ``lnw = ln pos`` under the Philox ``key``"""
        check(self.lib.fz_mw_dirichlet(self.h, ptr(alpha), ptr(counts), int(M), int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF,
                                       int(sweep), ptr(pos), ptr(lnw)))

    def mw_chain(self, rows, n, W, M, alpha, lnw, key, sweep0, nsweeps, counts, pos, first=0, neighbors=None, nnbr=None, counts_all=None):
        """fz_mw_chain: ``nsweeps`` sweeps on device-resident rows; ``lnw`` in and out, ``counts`` / ``pos`` of the last one"""
        check(self.lib.fz_mw_chain(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(alpha), ptr(lnw),
                                   int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF, int(first), int(sweep0), int(nsweeps), ptr(counts),
                                   ptr(pos), ptr(counts_all)))

    # -- EM over model weights (docs/model_weights.md; fz_mw_em.h) ----------------
    def mw_em_index_bytes(self, n, W, M, nnbr):
        """fz_mw_em_index_bytes -> (entries, bytes) of the inverted index of these neighbour counts"""
        e, b = C.c_int64(0), C.c_int64(0)
        check(self.lib.fz_mw_em_index_bytes(self.h, int(n), int(W), ptr(nnbr), int(M), C.addressof(e), C.addressof(b)))
        return int(e.value), int(b.value)

    def mw_em_index(self, rows, n, W, M, neighbors, nnbr, entries, col_off, col_obj, col_val):
        """fz_mw_em_index: device rows and tables -> ``col_off`` (M + 1) int64, ``col_obj`` (entries) int32, ``col_val`` (entries)"""
        check(self.lib.fz_mw_em_index(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), int(entries), ptr(col_off),
                                      ptr(col_obj), ptr(col_val)))

    def mw_loglike(self, rows, n, W, M, lnw, neighbors=None, nnbr=None, ell=None):
        """fz_mw_loglike -> (sum_i logsumexp_k (rows + lnw[neighbors])_ik over the rows with a posterior, rows skipped)"""
        out, ns = np.zeros(1), np.zeros(1, dtype=np.int64)
        check(self.lib.fz_mw_loglike(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(lnw), ptr(ell), ptr(out),
                                     ptr(ns)))
        return float(out[0]), int(ns[0])

    def mw_em(self, rows, n, W, M, alpha, lnw, niter, pos, counts, trace, nskip, neighbors=None, nnbr=None, index=None, entries=0):
        """fz_mw_em: ``niter`` EM iterations on device-resident rows (and ``index`` = (col_off, col_obj, col_val)); ``lnw`` in and out"""
        co, cj, cv = index if index is not None else (None, None, None)
        check(self.lib.fz_mw_em(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(co), ptr(cj), ptr(cv), int(entries),
                                ptr(alpha), ptr(lnw), int(niter), ptr(pos), ptr(counts), ptr(trace), ptr(nskip)))

    # -- posterior moments and zero-point sums (docs/predictive.md; fz_moments.h) ----
    def row_moments(self, rows, n, W, M, L, values, mean, var=None, share=None, value_errs=None, value_mask=None, scale=None,
                    neighbors=None, nnbr=None):
        """fz_row_moments: rows (n, W) of ln-weights over ``values`` (M, L) -> ``mean`` (n, L) [, ``var``, ``share``]; returns the
        number of rows without a posterior"""
        ns = np.zeros(1, dtype=np.int64)
        check(self.lib.fz_row_moments(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), ptr(scale), int(M), int(L), ptr(values),
                                      ptr(value_errs), ptr(value_mask), ptr(mean), ptr(var), ptr(share), ptr(ns)))
        return int(ns[0])

    # -- posterior bin masses and mixture CDFs (docs/bins.md; fz_bins.h) ----
    def row_bins(self, rows, n, W, M, labels, label_errs, edges, E, p, lncut=-np.inf, normalize=True, below=None, above=None,
                 neighbors=None, nnbr=None):
        """fz_row_bins: rows (n, W) of ln-weights over Gaussian labels (M) -> the masses ``p`` (n, E - 1) of the bins between the ``E``
        edges [, ``below``, ``above`` (n)]; ``lncut`` = ln(wt_thresh) (-inf: none); returns the number of rows without a posterior"""
        ns = np.zeros(1, dtype=np.int64)
        check(self.lib.fz_row_bins(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(labels), ptr(label_errs),
                                   ptr(edges), int(E), float(lncut), int(bool(normalize)), ptr(p), ptr(below), ptr(above), ptr(ns)))
        return int(ns[0])

    def row_cdf(self, rows, n, W, M, labels, label_errs, points, P, cdf, per_object=False, lncut=-np.inf, neighbors=None, nnbr=None):
        """fz_row_cdf: the mixture CDF of every row at ``points`` (P) or, with ``per_object``, (n, P) -> ``cdf`` (n, P); returns the
        number of rows without a posterior"""
        ns = np.zeros(1, dtype=np.int64)
        check(self.lib.fz_row_cdf(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(labels), ptr(label_errs),
                                  ptr(points), int(P), int(bool(per_object)), float(lncut), ptr(cdf), ptr(ns)))
        return int(ns[0])

    def row_quantiles(self, rows, n, W, M, labels, label_errs, probs, Q, out, lncut=-np.inf, neighbors=None, nnbr=None):
        """fz_row_quantiles (docs/quantiles.md): the quantiles of every row's mixture CDF at the ``Q`` shared probabilities ``probs`` ->
        ``out`` (n, Q); returns (rows without a posterior, solves that ended on the evaluation cap, evaluations in all)"""
        cnt = np.zeros(3, dtype=np.int64)
        check(self.lib.fz_row_quantiles(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(labels), ptr(label_errs),
                                        ptr(probs), int(Q), float(lncut), ptr(out), ptr(cnt[0:1]), ptr(cnt[1:2]), ptr(cnt[2:3])))
        return int(cnt[0]), int(cnt[1]), int(cnt[2])

    def row_scores(self, rows, n, W, M, labels, label_errs, points, P, per_object=False, lncut=-np.inf, lnpdf=None, crps=None, spread=None,
                   sqnorm=None, ninc=None, neighbors=None, nnbr=None):
        """fz_row_scores (docs/scores.md): the scoring rules of every row's mixture at ``points`` (P) or, with ``per_object``, (n, P) ->
        whichever of ``lnpdf`` (n, P), ``crps`` (n, P), ``spread`` (n), ``sqnorm`` (n) and ``ninc`` (n) int64 are given; returns the
        number of rows without a posterior"""
        ns = np.zeros(1, dtype=np.int64)
        check(self.lib.fz_row_scores(self.h, ptr(rows), int(n), int(W), ptr(neighbors), ptr(nnbr), int(M), ptr(labels), ptr(label_errs),
                                     ptr(points), int(P), int(bool(per_object)), float(lncut), ptr(lnpdf), ptr(crps), ptr(spread),
                                     ptr(sqnorm), ptr(ninc), ptr(ns)))
        return int(ns[0])

    def phot_sums(self, x, xe, xm, mean, var, n, B, clip=0.):
        """fz_phot_sums -> (sums (3, B) float64 = A, B, C; counts (2, B) int64 = n, nclip)"""
        sums, counts = np.zeros((3, int(B))), np.zeros((2, int(B)), dtype=np.int64)
        check(self.lib.fz_phot_sums(self.h, ptr(x), ptr(xe), ptr(xm), ptr(mean), ptr(var), int(n), int(B), float(clip), ptr(sums),
                                    ptr(counts)))
        return sums, counts

    # -- k-NN ------------------------------------------------------------
    def knn_upload_trees(self, feats, key=None):
        """``key``: the caller's content key of ``feats`` (``_digest``); an unchanged set is not sent (nor Morton-sorted) again"""
        f = np.ascontiguousarray(feats, dtype=np.float32)
        K, M, F = f.shape
        if key is None:
            key = _digest(f)
        if key == self._trees_key:
            return
        self._trees_key = None
        check(self.lib.fz_knn_upload_trees(self.h, ptr(f), K, M, F))
        self._trees_key = key

    def knn_draw_features(self, x, xe, n, F, fmap, key, first, q):
        """fz_knn_draw_features: ``q = map(x + xe z)`` (n, F) float64 for objects ``first .. first + n - 1`` under the Philox ``key``;
        ``x``, ``xe``, ``q`` host or device, the rows as given (not cleaned); ``fmap``: a ``_lib.KnnMap``"""
        check(self.lib.fz_knn_draw_features(self.h, ptr(x), ptr(xe), int(n), int(F), C.byref(fmap), int(key[0]) & 0xFFFFFFFF,
                                            int(key[1]) & 0xFFFFFFFF, int(first), ptr(q)))

    def knn_draw_trees(self, models, models_err, K, fmap, key, feats_out):
        """fz_knn_draw_trees: the K feature sets drawn on the device from the user's ``models`` / ``models_err`` (the shape of the
        uploaded model set) and installed as the resident sets; ``feats_out`` (K, M, F) float32 receives them and their content key
        becomes the engine's, so that ``knn_upload_trees`` of the same floats sends nothing.  Returns that key."""
        y, ye = _f64(models), _f64(models_err)
        M, F = y.shape
        self._trees_key = None
        check(self.lib.fz_knn_draw_trees(self.h, ptr(y), ptr(ye), int(K), int(M), int(F), C.byref(fmap), int(key[0]) & 0xFFFFFFFF,
                                         int(key[1]) & 0xFFFFFFFF, ptr(feats_out)))
        self._trees_key = _digest(feats_out)
        return self._trees_key

    def knn_query(self, q, k, distance_upper_bound, idx, n=None, lp_norm=2):
        n = len(q) if n is None else n
        check(self.lib.fz_knn_query(self.h, ptr(q), n, int(k), float(lp_norm), float(distance_upper_bound), ptr(idx)))

    def knn_fit_predict(self, x, xe, xm, idx, W, opts, kopts, neighbors=None, nnbr=None, lnlike=None,
                        chi2=None, ndim=None, scale=None, scale_err=None, pdfs=None, lmap=None,
                        levid=None, n=None):
        n = len(x) if n is None else n
        check(self.lib.fz_knn_fit_predict(self.h, ptr(x), ptr(xe), ptr(xm), n, ptr(idx), int(W),
                                          C.byref(opts), C.byref(kopts) if kopts is not None else None,
                                          ptr(neighbors), ptr(nnbr), ptr(lnlike), ptr(chi2), ptr(ndim),
                                          ptr(scale), ptr(scale_err), ptr(pdfs), ptr(lmap), ptr(levid)))

    def knn_fit_predict_prior(self, x, xe, xm, idx, W, opts, kopts, prior, neighbors=None, nnbr=None,
                              lnprior=None, lnlike=None, lnprob=None, chi2=None, ndim=None, scale=None,
                              scale_err=None, pdfs=None, lmap=None, levid=None, n=None):
        n = len(x) if n is None else n
        sfx, ps = self._prior_struct(prior)
        check(getattr(self.lib, "fz_knn_fit_predict_prior" + sfx)(
            self.h, ptr(x), ptr(xe), ptr(xm), n, ptr(idx), int(W), C.byref(opts),
            C.byref(kopts) if kopts is not None else None, ps, ptr(neighbors),
            ptr(nnbr), ptr(lnprior), ptr(lnlike), ptr(lnprob), ptr(chi2), ptr(ndim), ptr(scale),
            ptr(scale_err), ptr(pdfs), ptr(lmap), ptr(levid)))

    def knn_predict_logwt(self, logwt, neighbors, nnbr, W, kopts, pdfs, lmap=None, levid=None, n=None):
        n = len(logwt) if n is None else n
        check(self.lib.fz_knn_predict_logwt(self.h, ptr(logwt), ptr(neighbors), ptr(nnbr), n, int(W),
                                            C.byref(kopts), ptr(pdfs), ptr(lmap), ptr(levid)))

    # -- inference through a trained network (networks.py; fz_net.h) -----------
    def net_select(self, lnprob, use_wt, wt_thresh, cdf_thresh, match, csr_off, nsel, sel, rawlen=None, lmap=None, levid=None):
        n, nn = lnprob.shape
        nnodes = 0 if csr_off is None else len(csr_off) - 1
        check(self.lib.fz_net_select(self.h, ptr(lnprob), n, nn, int(bool(use_wt)), float(wt_thresh), float(cdf_thresh), ptr(match),
                                     ptr(csr_off), nnodes, ptr(nsel), ptr(sel), ptr(rawlen), ptr(lmap), ptr(levid)))

    def net_table(self, nsel, sel, match, csr_off, csr_items, W, idx):
        n, nn = sel.shape
        check(self.lib.fz_net_table(self.h, ptr(nsel), ptr(sel), n, nn, ptr(match), ptr(csr_off), ptr(csr_items), len(csr_off) - 1,
                                    int(W), ptr(idx)))

    def net_union(self, nsel, sel, match, csr_off, csr_items, M, nuniq, W=0, idx=None, n=None, nn=None):
        """fz_net_union: per object the union of its selected nodes' lists, repeats removed -> ``nuniq`` (n) int64 and, with ``idx``
        (n, W) int64, its elements ascending, padded with the smallest (``idx`` None: the counting call).  ``n`` / ``nn``: the
        shape of ``sel`` where it is handed over as a raw pointer"""
        if n is None:
            n, nn = sel.shape
        check(self.lib.fz_net_union(self.h, ptr(nsel), ptr(sel), int(n), int(nn), ptr(match), ptr(csr_off), ptr(csr_items),
                                    len(csr_off) - 1, int(M), int(W), ptr(nuniq), ptr(idx)))

    def net_gather(self, plane, nsel, sel, W, pad, out):
        n, nn = sel.shape
        bits = int(np.array([pad], dtype=plane.dtype).view(np.uint64)[0])
        check(self.lib.fz_net_gather(self.h, ptr(plane), ptr(nsel), ptr(sel), n, nn, int(W), bits, ptr(out)))

    def net_stack(self, lnprob, nsel, sel, match, node_pdfs, pdfs, lmap=None, levid=None):
        n, nn = sel.shape
        check(self.lib.fz_net_stack(self.h, ptr(lnprob), ptr(nsel), ptr(sel), n, nn, ptr(match), ptr(node_pdfs), node_pdfs.shape[0],
                                    node_pdfs.shape[1], ptr(pdfs), ptr(lmap), ptr(levid)))

    def som_train(self, x, xe, xm, nodes, pos, draws, lr, sig, kind, use_wt, wt_thresh, cdf_thresh, opts, track_scale, s0, s1, bmus):
        """steps [s0, s1) of SOM training (fz_som_train); arrays are NumPy or torch tensors on this engine's GPU"""
        M, B = x.shape
        nn, npj = pos.shape
        check(self.lib.fz_som_train(self.h, ptr(x), ptr(xe), ptr(xm), int(M), int(B), ptr(nodes), ptr(pos), int(nn), int(npj),
                                    ptr(draws), ptr(lr), ptr(sig), int(len(draws)), int(kind), int(bool(use_wt)), float(wt_thresh),
                                    float(cdf_thresh), C.byref(opts), int(bool(track_scale)), int(s0), int(s1), ptr(bmus)))

    def gng_train(self, x, xe, xm, draws, fstate, istate, ids, cap, max_degree, prune_cap, edge_cap, nbatch, max_age, max_nodes,
                  nnode_init, learn_best, learn_neighbor, new_err_keep, all_err_keep, opts, track_scale, alias0, alias1, s0, s1, bmus,
                  batch):
        """steps [s0, s1) of GNG training (fz_gng_train); arrays are NumPy or torch tensors on this engine's GPU"""
        M, B = x.shape
        check(self.lib.fz_gng_train(self.h, ptr(x), ptr(xe), ptr(xm), int(M), int(B), ptr(draws), int(len(draws)), ptr(fstate),
                                    ptr(istate), ptr(ids), int(cap), int(max_degree), int(prune_cap), int(edge_cap), int(nbatch),
                                    int(max_age), int(max_nodes), int(nnode_init), float(learn_best), float(learn_neighbor),
                                    float(new_err_keep), float(all_err_keep), C.byref(opts), int(bool(track_scale)), int(alias0),
                                    int(alias1), int(s0), int(s1), ptr(bmus), ptr(batch)))

    def pdfs_summarize(self, pdfs, pgrid, renormalize, urand, loss, widths, wscale, stats, n=None):
        n = len(pdfs) if n is None else n
        check(self.lib.fz_pdfs_summarize(self.h, ptr(pdfs), n, len(pgrid), ptr(pgrid), int(bool(renormalize)),
                                         ptr(urand), ptr(loss), ptr(widths), float(wscale), ptr(stats)))

    def pdfs_resample(self, pdfs, old_grid, new_grid, left, right, renormalize, out, n=None):
        n = len(pdfs) if n is None else n
        check(self.lib.fz_pdfs_resample(self.h, ptr(pdfs), n, len(old_grid), ptr(old_grid), len(new_grid), ptr(new_grid),
                                        float(left), float(right), int(bool(renormalize)), ptr(out)))

    def nz_assign(self, pdfs, nz, u, bins, counts, n=None):
        n = len(pdfs) if n is None else n
        check(self.lib.fz_nz_assign(self.h, ptr(pdfs), n, len(nz), ptr(nz), ptr(u), ptr(bins), ptr(counts)))

    def overlap_nz(self, pdfs, nz, pair, step, overlap, n=None):
        n = len(pdfs) if n is None else n
        out = np.zeros(1)
        pi, pj = (-1, -1) if pair is None else (int(pair[0]), int(pair[1]))
        check(self.lib.fz_overlap_nz(self.h, ptr(pdfs), n, len(nz), ptr(nz), pi, pj, float(step), ptr(overlap), ptr(out)))
        return float(out[0])

    # -- validation of a PDF stack (plotting.py; fz_diag.h) ---------------------
    def stack2d(self, pdfs, nrows, Gy, rows, cent, eidx, weff, pdf_thresh, prepared, stack, full_range=False, accumulate=False):
        """fz_stack2d over the dictionary last uploaded: ``rows`` / ``cent`` / ``eidx`` (int64) and ``weff`` (float64) are host
        arrays of the selected objects in ascending order of ``cent``; ``stack`` (Gx, Gy) is written, or added to"""
        check(self.lib.fz_stack2d(self.h, ptr(pdfs), int(nrows), int(Gy), len(rows), ptr(rows), ptr(cent), ptr(eidx), ptr(weff),
                                  float(pdf_thresh), int(bool(prepared)), int(bool(full_range)), int(bool(accumulate)), ptr(stack)))

    def recentre_rows(self, pdfs, n, pgrid, cent, disp, dgrid, out):
        """fz_recentre_rows: ``out`` (n, len(dgrid)) = every row resampled around its own centre (``disp`` 0: pgrid - cent,
        1: (pgrid - cent) / (1 + cent))"""
        check(self.lib.fz_recentre_rows(self.h, ptr(pdfs), int(n), len(pgrid), ptr(pgrid), ptr(cent), int(disp), len(dgrid),
                                        ptr(dgrid), ptr(out)))

    def cdf_draws(self, pdfs, n, grid, mc, weights=None, edges=None, draws=None, hist=None):
        """fz_cdf_draws: the CDF draws of ``mc`` (n, Nmc) into ``draws`` and / or their weighted histogram over ``edges``"""
        check(self.lib.fz_cdf_draws(self.h, ptr(pdfs), int(n), len(grid), ptr(grid), ptr(mc), int(mc.shape[1]), ptr(weights),
                                    ptr(edges), 0 if edges is None else len(edges) - 1, ptr(draws), ptr(hist)))

    # -- synthetic photometry (simulate.py; fz_synphot.h) -----------------------
    def synphot_upload(self, tb):
        """fz_synphot_upload of the tables ``tb`` (``simulate._Tables``); what the device already holds is not sent again"""
        key = _digest(tb.foff, tb.fwave, tb.flw, tb.fwt, tb.ftab, tb.toff, tb.tlw, tb.tas)
        if key == getattr(self, "_synphot_key", None):
            return
        self._synphot_key = None
        check(self.lib.fz_synphot_upload(self.h, tb.Nf, ptr(tb.foff), ptr(tb.fwave), ptr(tb.flw), ptr(tb.fwt), ptr(tb.ftab),
                                         tb.Nt, ptr(tb.toff), ptr(tb.tlw), ptr(tb.tas)))
        self._synphot_key = key

    def synphot(self, tmpl, z, ln1pz, igm, out):
        """fz_synphot: ``out`` (len(tmpl), Nf), host or device, of the (template, redshift) pairs; ``tmpl`` int64, ``z`` and
        ``ln1pz`` = log(1 + z) float64 host arrays; ``igm`` 0 none, 1 Madau"""
        check(self.lib.fz_synphot(self.h, len(tmpl), ptr(tmpl), ptr(z), ptr(ln1pz), int(igm), ptr(out)))

    # -- the n(z) samplers (samplers.py; fz_nzmc.h) ---------------------------
    def device_empty(self, shape, dtype=np.float64):
        """an uninitialised array in this engine's device memory that lives until its last reference dies (``DeviceArray``)"""
        return DeviceArray(self, shape, dtype)

    def device_array(self, a):
        """``a`` (NumPy) copied into device memory"""
        a = np.ascontiguousarray(a)
        d = DeviceArray(self, a.shape, a.dtype)
        d.set_rows(0, a)
        return d

    def dev_copy(self, dst, src, nbytes):
        """fz_dev_copy: ``nbytes`` from ``src`` to ``dst``, each a NumPy array, a device array or a raw address of either kind"""
        check(self.lib.fz_dev_copy(self.h, ptr(dst), ptr(src), int(nbytes)))

    def pdfs_colsum(self, pdfs, G, out, n=None):
        n = len(pdfs) if n is None else n
        check(self.lib.fz_pdfs_colsum(self.h, ptr(pdfs), n, int(G), ptr(out)))

    def nz_pairs(self, pdfs, n, G, pos, overlap, dcol, lnpost, pairs, normals, expo, nsamp, thin, mh_steps, s0, s1, samples,
                 samples_lnp, accept, gscale):
        """saved samples [s0, s1) of the population chain (fz_nz_pairs); pdfs, overlap and dcol live on this engine's GPU"""
        check(self.lib.fz_nz_pairs(self.h, ptr(pdfs), int(n), int(G), ptr(pos), ptr(overlap), ptr(dcol), ptr(lnpost), ptr(pairs),
                                   ptr(normals), ptr(expo), int(nsamp), int(thin), int(mh_steps), int(s0), int(s1), ptr(samples),
                                   ptr(samples_lnp), ptr(accept), ptr(gscale)))

    def nz_pair_eval(self, pdfs, n, G, overlap, dcol, what, pair, pend, step):
        """one evaluation of the population chain for a host-side decision (fz_nz_pair_eval); ``pend``: the accepted step not yet
        applied, or None.  Returns the two sums."""
        sums = np.zeros(2)
        pi, pj = (-1, -1) if pair is None else (int(pair[0]), int(pair[1]))
        check(self.lib.fz_nz_pair_eval(self.h, ptr(pdfs), int(n), int(G), ptr(overlap), ptr(dcol), int(what), pi, pj,
                                       int(pend is not None), 0. if pend is None else float(pend), float(step), ptr(sums)))
        return sums

    def nz_sweep(self, pdfs, n, nz, counts, u=None, key=None, sweep=0):
        """counts of one Gibbs sweep's categorical draws (fz_nz_sweep): the caller's uniforms ``u``, or Philox under ``key``"""
        k0, k1 = (0, 0) if key is None else (int(key[0]), int(key[1]))
        check(self.lib.fz_nz_sweep(self.h, ptr(pdfs), int(n), len(nz), ptr(nz), ptr(u), int(key is not None), k0, k1, int(sweep),
                                   ptr(counts)))

    def knn_search_fit_predict(self, q, x, xe, xm, k, lp_norm, distance_upper_bound, opts, kopts, prior=None,
                               neighbors=None, nnbr=None, lnprior=None, lnlike=None, lnprob=None, chi2=None, ndim=None,
                               scale=None, scale_err=None, pdfs=None, lmap=None, levid=None, n=None):
        """fz_knn_search_fit_predict_prior: the K searches and the subset likelihood / PDFs in one call, the neighbour
        table staying on the device"""
        n = len(x) if n is None else n
        sfx, ps = self._prior_struct(prior)
        check(getattr(self.lib, "fz_knn_search_fit_predict_prior" + sfx)(
            self.h, ptr(q), ptr(x), ptr(xe), ptr(xm), n, int(k), float(lp_norm), float(distance_upper_bound),
            C.byref(opts), C.byref(kopts) if kopts is not None else None, ps, ptr(neighbors),
            ptr(nnbr), ptr(lnprior), ptr(lnlike), ptr(lnprob), ptr(chi2), ptr(ndim), ptr(scale), ptr(scale_err),
            ptr(pdfs), ptr(lmap), ptr(levid)))

    def set_producer_stream(self, stream=None, mode=1):
        """fz_set_producer_stream.  ``mode`` 0: device-wide wait before device inputs are read (default of a fresh
        engine); 1: wait for ``stream`` only (an int ``hipStream_t``, e.g. ``torch.cuda.current_stream().cuda_stream``;
        None / 0: the legacy default stream); 2: inputs are complete, no wait."""
        check(self.lib.fz_set_producer_stream(self.h, int(stream or 0), int(mode)))
        self._producer = (stream, int(mode))

    def producer_stream(self):
        """(stream, mode) of the last ``set_producer_stream`` (a fresh context: (None, 0)): what a caller that changes the contract
        for the length of one call puts back"""
        return getattr(self, "_producer", (None, 0))

    def modec_info(self):
        """mode C since the last ``timing_reset``: ``(ambiguous objects re-run with IEEE divisions, iterations of the
        slowest object, 1 = one block per object / 2 = state planes, threads per block)``"""
        out = np.zeros(4, dtype=np.int64)
        check(self.lib.fz_modec_info(self.h, ptr(out)))
        return tuple(int(v) for v in out)

    def modec_niter(self, n):
        """passes of the loop at pdf.py:199 each of the first ``n`` objects of the last mode-C chunk took"""
        out = np.zeros(int(n), dtype=np.int32)
        check(self.lib.fz_modec_niter(self.h, int(n), ptr(out)))
        return out

    def clean(self, x, xe, xm):
        check(self.lib.fz_clean(self.h, ptr(x), ptr(xe), ptr(xm), x.shape[0], x.shape[1]))

    def sync(self):
        check(self.lib.fz_sync(self.h))

    def timing_reset(self):
        """zero the per-family timers (and the mode-C bookkeeping of ``modec_info``)"""
        check(self.lib.fz_timing_reset(self.h))

    def timing(self):
        t = Timing()
        check(self.lib.fz_timing_get(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timing._fields_}

    def last_form(self):
        """which kernel form the last fused fit_predict launch took (depends on the data)"""
        return self.lib.fz_last_form(self.h).decode("ascii", "replace")

    def set_workspace_limit(self, nbytes):
        check(self.lib.fz_set_workspace_limit(self.h, int(nbytes)))

    def workspace_limit(self):
        """the workspace budget in force, in bytes"""
        return int(self.lib.fz_get_workspace_limit(self.h))

    def cu_count(self):
        """compute units of the engine's device"""
        return int(self.lib.fz_cu_count(self.h))


class DeviceArray(object):
    """A C-contiguous array in an engine's device memory (fz_dev_alloc), with the few tensor-like members the host layer looks at
    (``shape``, ``data_ptr()``, ``len()``); ``numpy()`` copies it to the host, ``set_rows(r0, a)`` copies ``a`` in at row ``r0``,
    ``row_ptr(r0)`` is the address of that row."""

    def __init__(self, eng, shape, dtype=np.float64):
        self.shape = tuple(int(v) for v in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self._eng, self._ptr = eng, None
        h = C.c_void_p()
        check(eng.lib.fz_dev_alloc(eng.h, self.nbytes, C.byref(h)))
        self._ptr = h.value

    def data_ptr(self):
        return self._ptr

    def __len__(self):
        return self.shape[0]

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return True

    def element_size(self):
        return self.dtype.itemsize

    def numpy(self):
        out = np.empty(self.shape, dtype=self.dtype)
        check(self._eng.lib.fz_dev_copy(self._eng.h, ptr(out), self._ptr, self.nbytes))
        return out

    def row_ptr(self, r0):
        """the device address of row ``r0`` (one past the last row included: the end of the array)"""
        if not 0 <= r0 <= self.shape[0]:
            raise IndexError("row %d of an array of shape %r" % (r0, self.shape))
        return self._ptr + r0 * self.dtype.itemsize * int(np.prod(self.shape[1:], dtype=np.int64))

    def set_rows(self, r0, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.shape[1:] != self.shape[1:] or r0 < 0 or r0 + len(a) > self.shape[0]:
            raise ValueError("rows [%d, %d) do not fit an array of shape %r" % (r0, r0 + len(a), self.shape))
        check(self._eng.lib.fz_dev_copy(self._eng.h, self.row_ptr(r0), ptr(a), a.nbytes))

    def __del__(self):
        try:
            if self._ptr and getattr(self._eng, "h", None):
                self._eng.lib.fz_dev_free(self._eng.h, self._ptr)
        except Exception:           # interpreter shutdown
            pass


_engines = {}


def get_engine(device=None):
    """Process-wide engine for ``device`` (default: LOCAL_RANK or 0)."""
    import os
    if device is None:
        device = int(os.environ.get("FRANKENZ_DEVICE", os.environ.get("LOCAL_RANK", 0)))
        ndev = _lib.load().fz_device_count()
        if ndev > 0:
            device %= ndev
    if device not in _engines:
        _engines[device] = Engine(device)
    return _engines[device]


class HostObjects(object):
    """float64 C-contiguous staging of (data, data_err, data_mask) that writes the
    in-place clean of pdf.py:310-311 back into the caller's arrays."""

    def __init__(self, data, data_err, data_mask):
        self.src = (data, data_err, data_mask)
        self.x, self.xe, self.xm = _f64(data), _f64(data_err), _f64(data_mask)
        if self.x.ndim != 2 or self.xe.shape != self.x.shape or self.xm.shape != self.x.shape:
            raise ValueError("data, data_err, data_mask must share a (Ndata, Nfilt) shape")

    def writeback(self):
        for dst, buf in zip(self.src, (self.x, self.xe, self.xm)):
            if isinstance(dst, np.ndarray) and dst is not buf and not np.shares_memory(dst, buf):
                dst[...] = buf
