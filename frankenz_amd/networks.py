"""
Inference through a trained network (SOM / GNG): the reference's ``_Network`` (frankenz/networks.py:120-1473), and
the training of a ``SelfOrganizingMap`` (networks.py:1490-1867, ``fz_som_train``, docs/som.md) and of a ``GrowingNeuralGas``
(networks.py:1870-2260, ``fz_gng_train``, docs/gng.md) on the device, at the end of this file.
The network is DATA here -- node positions in data space -- and everything the reference then does with it runs
through the library:

* ``populate_network`` (networks.py:244-356): (Nmodel, Nnode) likelihoods with the nodes as noiseless models (``k_planes``), the
  thresholding rule, per-model max / logsumexp of the kept entries (``fz_net_select``); the per-node lists are the transpose of the
  kept (model, node) pairs -- integer bookkeeping, done with NumPy sorts.
* ``fit`` / ``predict`` / ``fit_predict`` (networks.py:782-936, 938-1128, 1130-1473): node likelihoods of the objects, thresholding
  (``fz_net_select``), then either the selected nodes as the models (``nodes_only``: ``fz_net_gather`` / ``fz_net_stack`` on the node
  PDFs) or the union of the selected nodes' model lists (``fz_net_table``) through the k-NN subset kernel (``fz_knn_fit_predict``:
  first-appearance de-dup = pandas.unique, likelihood, weights, KDE).
* ``get_pdfs`` (networks.py:413-560): per-node KDE of the member models (``fz_knn_predict_logwt``), scaled by exp(levid).
* ``fit_sparse`` (extension, docs/network.md "Sparse rows"): the fit as a ``SparseFits`` over the union of the selected nodes' lists
  with repeats removed on the device (``fz_net_union``), sized by the largest union instead of the summed list lengths.

A foreign ``lpnet_func`` / ``lprob_func`` is the user's code: it is called on the host per object exactly as the reference calls it;
the selection, the unions and the PDFs still run on the device.  The stages these share are listed in docs/network.md, "Python surface".
"""
import sys
from collections import namedtuple

import numpy as np

from . import pdf as _pdf
from .engine import HostObjects, get_engine, kde_opts, like_opts, merge_kde_args

__all__ = ["populate_network", "Network", "SelfOrganizingMap", "GrowingNeuralGas", "learn_linear", "learn_geometric", "learn_harmonic",
           "neighbor_gauss", "neighbor_lorentz"]

_NET_CHUNK = 1 << 16          # objects per device call
_NODES_MAX = 4096             # matched nodes fz_net_select takes (an object's row sits in LDS)
_UNION_MAX = 4096             # entries of an object's union table before de-duplication (FZ_KNN_WMAX)
_UNION_MMAX = 1 << 20         # models fz_net_union takes (FZ_NET_UNION_MMAX: an object's bitmap of the models sits in LDS)


class NetworkMap(object):
    """the attributes ``_Network._populate_network`` fills (networks.py:296-303)"""
    pass


def populate_network(nodes, models, models_err, models_mask, lpnet_kwargs=None, wt_thresh=1e-3,
                     cdf_thresh=2e-4, track_scale=True, device=None):
    """Map every model onto the nodes it is compatible with (networks.py:244-354).
    Returns an object with ``nodes_idxs, nodes_logwts, nodes_bmus, nodes_scales,
    nodes_scales_err, nodes_Nmatch, models_lmap, models_levid`` exactly as the reference
    leaves them on the network, plus ``results``: the per-model tuples the generator yields."""
    if lpnet_kwargs is None:
        lpnet_kwargs = {'free_scale': True, 'ignore_model_err': True, 'return_scale': True}
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    Nnodes, Nmodels = len(nodes), len(models)
    eng = get_engine(device)
    lnprob = np.empty((Nmodels, Nnodes))
    scale = np.ones((Nmodels, Nnodes)); scale_err = np.zeros((Nmodels, Nnodes))
    free = _fit_nodes(eng, nodes, HostObjects(models, models_err, models_mask), lpnet_kwargs, lnprob,
                      scale=scale if track_scale else None, scale_err=scale_err if track_scale else None)
    if track_scale and not free:
        raise ValueError("track_scale=True needs a likelihood that returns the scale (free_scale=True)")
    return _lists_from_plane(lnprob, scale, scale_err, wt_thresh, cdf_thresh, track_scale, eng)


def _selection_rule(wt_thresh, cdf_thresh):
    """-> (use_wt, wt_thresh, cdf_thresh) as fz_net_select / fz_som_train take them; neither given: the weight rule at -inf, keep all"""
    if wt_thresh is None and cdf_thresh is None:
        wt_thresh = -np.inf
    use_wt = wt_thresh is not None
    return use_wt, wt_thresh if use_wt else 0.0, 0.5 if use_wt else cdf_thresh


def _fit_nodes(eng, y, obj, lpnet_kwargs, lnprob, chi2=None, ndim=None, scale=None, scale_err=None, n=None):
    """The built-in node likelihood (networks.py:305-312, 880-882): the nodes ``y`` as noiseless, unmasked models, ``obj`` (HostObjects)
    fitted into host planes or a device plane (``n``), cleaned and written back.  Returns whether the scale is free (else not filled)."""
    eng.upload_models(y, np.zeros_like(y), np.ones_like(y))
    opts = like_opts(lpnet_kwargs)
    free = bool(opts.free_scale)
    eng.fit(obj.x, obj.xe, obj.xm, opts, lnprob, chi2, ndim, scale if free else None, scale_err if free else None, n=n)
    obj.writeback()
    return free


def _foreign_node_rows(lpnet_func, lpnet_args, lpnet_kwargs, y, data, data_err, data_mask, take=None):
    """the user's ``lpnet_func`` per object as networks.py:310-312, 880-882 call it; its result tuples (or the positions ``take`` of
    them: nothing else is held) stacked, one array per position"""
    ye = np.zeros_like(y)
    ym = np.ones_like(y, dtype='bool')                                     # (a boolean mask, as the reference hands over)
    calls = (lpnet_func(x, xe, xm, y, ye, ym, *lpnet_args, **lpnet_kwargs) for x, xe, xm in zip(data, data_err, data_mask))
    rows = [r if take is None else [r[k] for k in take] for r in calls]
    return [np.ascontiguousarray(np.array([r[k] for r in rows])) for k in range(len(rows[0]))]


def _select(eng, lnprob, wt_thresh, cdf_thresh, match=None, csr_off=None, want_stats=False):
    """fz_net_select on a host plane: (nsel, sel[, rawlen][, lmap, levid])"""
    n, nn = lnprob.shape
    nsel = np.zeros(n, dtype=np.int32); sel = np.zeros((n, nn), dtype=np.int32)
    rawlen = np.zeros(n, dtype=np.int64) if csr_off is not None else None
    lmap = np.zeros(n) if want_stats else None; levid = np.zeros(n) if want_stats else None
    eng.net_select(lnprob, *_selection_rule(wt_thresh, cdf_thresh), match, csr_off, nsel, sel, rawlen, lmap, levid)
    return nsel, sel, rawlen, lmap, levid


def _refuse_no_node(nsel, i0, wt_thresh, cdf_thresh):
    """(the reference fails here too, in np.max of nothing; a padded table would quietly fit model 0: docs/deviations.md)"""
    if not nsel.all():
        use_wt, wt, _ = _selection_rule(wt_thresh, cdf_thresh)
        raise ValueError("object %d selects no node of the network (%d of %d objects in this call do): its node ln-probabilities "
                         "hold a nan, or none passes the threshold (wt_thresh=%r, cdf_thresh=%r)"
                         % (i0 + int(np.argmin(nsel != 0)), int((nsel == 0).sum()), len(nsel), wt if use_wt else None, cdf_thresh))


def _refuse_no_model(counts, i0):
    """(``discrete``: a matched node need not be any model's best one; the reference fails in np.max of nothing)"""
    if not counts.all():
        raise ValueError("object %d: the nodes it selects list no model" % (i0 + int(np.argmin(counts != 0))))


def _lists_from_plane(lnprob, scale, scale_err, wt_thresh, cdf_thresh, track_scale, eng=None):
    """the (Nmodels, Nnodes) ln-prob plane -> the per-model selections and the per-node lists"""
    # The selection of every model's nodes (either rule, in the reference's order) and the max / logsumexp over the kept entries
    # come from the device (fz_net_select, networks.py:316-333); what follows is the transpose of the kept (model, node) pairs into
    # per-node lists -- models ascending inside a node, as the reference's model loop appends them.
    eng = eng if eng is not None else get_engine(None)
    nsel, sel, _, lmap, levid = _select(eng, np.ascontiguousarray(lnprob), wt_thresh, cdf_thresh, want_stats=True)
    return _lists_from_selection(lnprob, scale, scale_err, nsel, sel, lmap, levid, track_scale)


def _lists_from_selection(lnprob, scale, scale_err, nsel, sel, lmap, levid, track_scale):
    """the transpose: per-model selections (nsel, sel: fz_net_select) -> per-node lists, as networks.py:335-352 appends them"""
    Nmodels, Nnodes = lnprob.shape
    out = NetworkMap()
    rows = np.arange(Nmodels)
    out.models_bmu = np.argmax(lnprob, axis=1)
    keep = np.arange(Nnodes)[None, :] < nsel[:, None]
    pair_model = np.nonzero(keep)[0]
    pair_node = sel[keep].astype(np.int64)
    pair_lnp = lnprob[pair_model, pair_node]
    counts = nsel.astype(np.int64)
    out.models_lmap, out.models_levid = lmap, levid
    pair_logwt = pair_lnp - levid[pair_model]                        # networks.py:331
    if track_scale:
        pair_s, pair_se = scale[pair_model, pair_node], scale_err[pair_model, pair_node]
    else:
        pair_s, pair_se = np.ones_like(pair_node), np.zeros_like(pair_node)        # integer ones / zeros like the reference
    # per-node lists: the pairs regrouped by node, models ascending within a node (stable sort)
    by_node = np.argsort(pair_node, kind='stable')
    cuts = np.cumsum(np.bincount(pair_node, minlength=Nnodes))[:-1]
    out.nodes_idxs = [a.tolist() for a in np.split(pair_model[by_node], cuts)]
    out.nodes_logwts = [a.tolist() for a in np.split(pair_logwt[by_node], cuts)]
    out.nodes_scales = [a.tolist() for a in np.split(pair_s[by_node], cuts)]
    out.nodes_scales_err = [a.tolist() for a in np.split(pair_se[by_node], cuts)]
    out.nodes_Nmatch = np.bincount(pair_node, minlength=Nnodes).astype('int')
    bmu_order = np.argsort(out.models_bmu, kind='stable')
    out.nodes_bmus = [a.tolist() for a in np.split(rows[bmu_order], np.cumsum(np.bincount(out.models_bmu, minlength=Nnodes))[:-1])]
    # the per-model tuples the reference's generator yields
    mcuts = np.cumsum(counts)[:-1]
    out.results = list(zip(np.split(pair_node, mcuts), np.split(pair_logwt, mcuts), np.split(pair_s, mcuts), np.split(pair_se, mcuts)))
    return out


def _csr(lists):
    """ragged per-node lists -> (offsets int64[Nnodes + 1], items int64)"""
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(v) for v in lists], out=off[1:])
    items = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if off[-1] else np.zeros(1, dtype=np.int64)
    return off, np.ascontiguousarray(items)


def _padded(lists, lens, N, W, fill, dtype):
    """ragged per-row lists (or one scalar per row) -> the (N, W) table: row i holds its ``lens[i]`` entries, then ``fill``"""
    out = np.full((N, W), fill, dtype=dtype)
    for i in range(N):
        out[i, :lens[i]] = lists[i]
    return out


def _is_default(func):
    return func is None or func is _pdf.logprob


# the matched nodes: their indices (int64; int32 as the kernels take them), positions and number; the lists of ALL nodes as CSR
_Matched = namedtuple('_Matched', 'sel sel32 y Nn off items')


def _sparse_chunks(eng, mt, lpnet_kwargs, data, thresh, kept, nc, form):
    """A pass of ``fit_sparse`` over the objects, ``nc`` per device call: yields (i0, n, the staged objects, the device addresses of
    their nsel / sel) -- rows of ``kept``, the selection of the whole call, or arrays of the chunk's own.  ``form``: the node
    likelihoods (cleaned in place, written back) and the selection are formed now."""
    for i0 in range(0, len(data[0]), nc):
        n = min(nc, len(data[0]) - i0)
        own = kept or (eng.device_empty((n,), np.int32), eng.device_empty((n, mt.Nn), np.int32))
        d_nsel, d_sel = [a.row_ptr(i0 if kept else 0) for a in own]
        obj = HostObjects(*[a[i0:i0 + n] for a in data])
        if form:
            plane = eng.device_empty((n, mt.Nn), np.float64)
            _fit_nodes(eng, mt.y, obj, lpnet_kwargs, plane, n=n)
            eng.net_select(plane, *_selection_rule(*thresh), None, None, d_nsel, d_sel)
            del plane                                                  # (a chunk is sized with the plane gone before the tables come)
        yield i0, n, obj, d_nsel, d_sel


class Network(object):
    """The inference half of the reference's ``_Network`` (networks.py:120-1473): same constructor, methods, keywords, defaults and
    attributes; the network itself is handed over as data (``set_nodes``) instead of being trained here."""

    def __init__(self, models, models_err, models_mask, device=None):
        self.models, self.models_err, self.models_mask = models, models_err, models_mask
        self.NMODEL, self.NDIM = models.shape
        self.models_lmap = np.zeros(self.NMODEL) - np.inf
        self.models_levid = np.zeros(self.NMODEL) - np.inf
        self.fit_lnprior = self.fit_lnlike = self.fit_lnprob = self.fit_Ndim = self.fit_chi2 = None
        self.fit_scale = self.fit_scale_err = None
        self.nodes = self.nodes_pos = self.nodes_idxs = self.nodes_logwts = self.nodes_bmus = None
        self.nodes_scales = self.nodes_scales_err = self.nodes_Nmatch = self.nodes_only = None
        self.NNODE, self.NPROJ = None, None
        self.neighbors = self.Nneighbors = None
        self._device = device

    # -- the trained network, as data --------------------------------------------------------------------
    def set_nodes(self, nodes, nodes_pos=None):
        """node positions in data space (Nnode, Nfilt) [and on the manifold (Nnode, Nproj)]: what ``train_network`` leaves behind"""
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        self.NNODE = len(self.nodes)
        if nodes_pos is not None:
            self.nodes_pos = np.asarray(nodes_pos)
            self.NPROJ = self.nodes_pos.shape[1]
        return self

    def _training_models(self, models, models_err, models_mask, err_kernel):
        """the arrays ``train_network`` fits: the given ones, by default the object's own, ``err_kernel`` added to the errors"""
        models_err = _given(models_err, self.models_err)
        if err_kernel is not None:
            models_err = np.sqrt(models_err**2 + err_kernel**2)          # added in quadrature
        return _given(models, self.models), models_err, _given(models_mask, self.models_mask)

    def _eng(self):
        return get_engine(self._device)

    # -- networks.py:176-356 -----------------------------------------------------------------------------
    def populate_network(self, lpnet_func=None, wt_thresh=1e-3, cdf_thresh=2e-4, lpnet_args=None, lpnet_kwargs=None,
                         track_scale=True, verbose=True):
        for _ in self._populate_network(lpnet_func, wt_thresh, cdf_thresh, lpnet_args, lpnet_kwargs, track_scale):
            pass
        if verbose:
            sys.stderr.write('\rMapping objects 100%\n'); sys.stderr.flush()

    def _populate_network(self, lpnet_func=None, wt_thresh=1e-3, cdf_thresh=2e-4, lpnet_args=None, lpnet_kwargs=None,
                          track_scale=True):
        if self.nodes is None:
            raise ValueError("Network has not been trained!")
        lpnet_func, lpnet_args = _given(lpnet_func, _pdf.logprob), _given(lpnet_args, [])
        lpnet_kwargs = _given(lpnet_kwargs, {'free_scale': True, 'ignore_model_err': True, 'return_scale': True})
        self.lpnet_func, self.lpnet_args, self.lpnet_kwargs = lpnet_func, lpnet_args, lpnet_kwargs
        if _is_default(lpnet_func) and not lpnet_args:
            m = populate_network(self.nodes, self.models, self.models_err, self.models_mask, lpnet_kwargs=lpnet_kwargs, wt_thresh=wt_thresh,
                                 cdf_thresh=cdf_thresh, track_scale=track_scale, device=self._device)
        else:
            # the user's node likelihood, per model; selection and lists as above
            planes = _foreign_node_rows(lpnet_func, lpnet_args, lpnet_kwargs, self.nodes, self.models, self.models_err, self.models_mask,
                                        take=(2, 5, 6) if track_scale else (2,))
            planes = [np.ascontiguousarray(p, dtype=np.float64) for p in planes]
            sc, se = planes[1:] if track_scale else (None, None)
            m = _lists_from_plane(planes[0], sc, se, wt_thresh, cdf_thresh, track_scale, self._eng())
        self.nodes_idxs, self.nodes_logwts, self.nodes_bmus = m.nodes_idxs, m.nodes_logwts, m.nodes_bmus
        self.nodes_scales, self.nodes_scales_err, self.nodes_Nmatch = m.nodes_scales, m.nodes_scales_err, m.nodes_Nmatch
        self.models_lmap, self.models_levid = m.models_lmap, m.models_levid
        yield from m.results

    # -- networks.py:358-411 -----------------------------------------------------------------------------
    def get_node(self, idx=None, pos=None, discrete=False):
        if idx is None and pos is None:
            raise ValueError("Either `idx` or `pos` must be specified.")
        elif idx is not None and pos is not None:
            raise ValueError("Both `idx` and `pos` cannot be specified.")
        elif pos is not None:
            idx = np.argmin([sum((pos - p)**2) for p in self.nodes_pos])
        if discrete:
            idxs = self.nodes_bmus[idx]
            logwts = np.zeros_like(idxs)
        else:
            idxs, logwts = self.nodes_idxs[idx], self.nodes_logwts[idx]
        return (idx, self.nodes[idx], self.nodes_pos[idx] if self.nodes_pos is not None else None, idxs, logwts,
                self.nodes_scales[idx], self.nodes_scales_err[idx])

    # -- networks.py:413-560 -----------------------------------------------------------------------------
    def _labels(self, eng, model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs):
        if label_dict is None and label_grid is None:
            raise ValueError("`label_dict` or `label_grid` must be specified.")
        kw = merge_kde_args(kde_args, kde_kwargs, label_dict is not None)
        eng.upload_models(self.models, self.models_err, self.models_mask)
        eng.set_labels(model_labels, model_label_errs, label_dict=label_dict, label_grid=label_grid, kde_kwargs=kw)
        return kde_opts(kw), (label_dict.Ngrid if label_dict is not None else len(label_grid))

    def get_pdfs(self, model_labels, model_label_errs, label_dict=None, label_grid=None, kde_args=None, kde_kwargs=None,
                 return_gof=False, discrete=False, verbose=True):
        if label_dict is None and label_grid is None:
            raise ValueError("`label_dict` or `label_grid` must be specified.")
        if self.nodes_idxs is None:
            raise ValueError("Network has not been trained!")
        eng = self._eng()
        ko, G = self._labels(eng, model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs)
        lists = self.nodes_bmus if discrete else self.nodes_idxs
        lens = np.array([len(v) for v in lists], dtype=np.int64)
        W = max(int(lens.max()), 1)
        nbr = _padded(lists, lens, self.NNODE, W, 0, np.int64)
        lwt = _padded(np.zeros(self.NNODE) if discrete else self.nodes_logwts, lens, self.NNODE, W, -np.inf, np.float64)
        pdfs = np.zeros((self.NNODE, G)); lmap = np.zeros(self.NNODE); levid = np.zeros(self.NNODE)
        eng.knn_predict_logwt(lwt, nbr, lens, W, ko, pdfs, lmap, levid)
        empty = lens == 0
        pdfs[empty] = 0.0; lmap[empty] = -np.inf; levid[empty] = -np.inf
        pdfs *= np.exp(levid)[:, None]                              # scale to the associated object density (networks.py:548)
        if verbose:
            sys.stderr.write('\rGenerating node PDF {0}/{1}\n'.format(self.NNODE, self.NNODE)); sys.stderr.flush()
        return (pdfs, (lmap, levid)) if return_gof else pdfs

    def _get_pdfs(self, model_labels, model_label_errs, label_dict=None, label_grid=None, kde_args=None, kde_kwargs=None,
                  discrete=False):
        pdfs, (lmap, levid) = self.get_pdfs(model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs, True,
                                             discrete, False)
        for i in range(self.NNODE):
            yield pdfs[i], (lmap[i], levid[i])

    def get_pdf(self, idx, model_labels, model_label_errs, label_dict=None, label_grid=None, kde_args=None, kde_kwargs=None,
                return_gof=False, discrete=False):
        pdfs, (lmap, levid) = self.get_pdfs(model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs, True,
                                             discrete, False)
        return (pdfs[idx], (lmap[idx], levid[idx])) if return_gof else pdfs[idx]

    # -- the shared body of fit / fit_predict (networks.py:856-936, 1389-1473) ------------------------------
    def _run(self, data, data_err, data_mask, lprob_func, nodes_only, wt_thresh, cdf_thresh, lprob_args, lprob_kwargs, track_scale,
             discrete, save_fits, predict=None):
        """predict: None, or (model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs).  Returns per-object
        (idxs, Nidx, results[, pdf, (lmap, levid)]) tuples; stores the fits like the reference when save_fits."""
        if self.nodes_idxs is None:
            raise ValueError("Network has not been trained!")
        lprob = (lprob_func, lprob_args or [], lprob_kwargs or {})
        eng = self._eng()
        Ndata = len(data)
        mt = self._matched(discrete)
        self.nodes_only = nodes_only
        if save_fits:
            self.NDATA = Ndata
            self.Nneighbors = np.zeros(Ndata, dtype='int'); self.neighbors = []
            self.fit_lnprior, self.fit_lnlike, self.fit_lnprob, self.fit_Ndim, self.fit_chi2 = [], [], [], [], []
            self.fit_scale, self.fit_scale_err = [], []
        node_pdfs = None
        if predict is not None and nodes_only:
            node_pdfs = np.ascontiguousarray(self.get_pdfs(*predict, False, discrete, False))
        out = []
        for i0 in range(0, Ndata, _NET_CHUNK):
            sl = slice(i0, min(i0 + _NET_CHUNK, Ndata))
            chunk = (data[sl], data_err[sl], data_mask[sl])
            obj = HostObjects(*chunk)
            nres, lnp, width = self._node_results(eng, mt, obj, chunk)
            nsel, sel, rawlen, _, _ = _select(eng, lnp, wt_thresh, cdf_thresh, mt.sel32, None if nodes_only else mt.off)
            _refuse_no_node(nsel, i0, wt_thresh, cdf_thresh)
            if nodes_only:
                fit = self._fit_nodes_only(eng, mt, nres, lnp, width, nsel, sel, node_pdfs)
            else:
                _refuse_no_model(rawlen, i0)
                fit = self._fit_union(eng, mt, obj, chunk, i0, nsel, sel, rawlen, lprob, predict)
            out += self._emit(i0, save_fits, track_scale, *fit)
        return out

    def _matched(self, discrete):
        sel = np.arange(self.NNODE)[self.nodes_Nmatch > 0]
        y = np.ascontiguousarray(self.nodes[sel])
        return _Matched(sel, np.ascontiguousarray(sel, dtype=np.int32), y, len(y), *_csr(self.nodes_bmus if discrete else self.nodes_idxs))

    def _node_results(self, eng, mt, obj, chunk):
        """Node likelihoods of one chunk (networks.py:880-882): the (n, Nn) planes of the result tuple, the ln-probabilities as the
        selection takes them, how many planes ``nodes_only`` hands out (pdf.logprob: seven with return_scale, else five; the user's: all)"""
        if not (_is_default(self.lpnet_func) and not self.lpnet_args):
            nres = _foreign_node_rows(self.lpnet_func, self.lpnet_args, self.lpnet_kwargs, mt.y, *chunk)
            return nres, np.ascontiguousarray(nres[2], dtype=np.float64), len(nres)
        n, Nn = len(obj.x), mt.Nn
        lnp = np.empty((n, Nn)); chi2 = np.empty((n, Nn)); ndim = np.empty((n, Nn), dtype=np.int64)
        sc = np.ones((n, Nn)); se = np.zeros((n, Nn))
        _fit_nodes(eng, mt.y, obj, self.lpnet_kwargs, lnp, chi2, ndim, sc, se)
        return [np.zeros((n, Nn)), lnp, lnp, ndim, chi2, sc, se], lnp, 7 if self.lpnet_kwargs.get('return_scale', False) else 5

    def _fit_nodes_only(self, eng, mt, nres, lnp, width, nsel, sel, node_pdfs):
        """the selected nodes as the models (networks.py:907-909, 1463-1470): their results gathered, their PDFs stacked by weight"""
        n, W = len(nsel), max(int(nsel.max()), 1)
        res = []
        for pl in nres:
            pl = np.ascontiguousarray(pl)
            if pl.dtype not in (np.float64, np.int64):
                pl = pl.astype(np.float64)
            g = np.empty((n, W), dtype=pl.dtype)
            eng.net_gather(pl, nsel, sel, W, 0, g)
            res.append(g)
        nb = np.empty((n, W), dtype=np.int64)
        eng.net_gather(np.ascontiguousarray(np.broadcast_to(mt.sel.astype(np.int64), (n, mt.Nn))), nsel, sel, W, -99, nb)
        pdfs = lmap = levid = None
        if node_pdfs is not None:
            pdfs = np.empty((n, node_pdfs.shape[1])); lmap = np.empty(n); levid = np.empty(n)
            eng.net_stack(lnp, nsel, sel, mt.sel32, node_pdfs, pdfs, lmap, levid)
        return nb, nsel.astype(np.int64), lambda k, m: [p[k, :m].copy() for p in res[:width]], pdfs, lmap, levid

    def _fit_union(self, eng, mt, obj, chunk, i0, nsel, sel, rawlen, lprob, predict):
        """the union of the selected nodes' lists as the models (networks.py:913-936, 1413-1460); ``lprob`` = (func, args, kwargs)"""
        lprob_func, lprob_args, lprob_kwargs = lprob
        host_lprob = not (_is_default(lprob_func) and not lprob_args)
        n, W = len(nsel), max(int(rawlen.max()), 1)
        if W > _UNION_MAX:
            raise NotImplementedError("object %d: its selected nodes list %d models before repeats are removed; the union table "
                                      "of fz_knn_fit_predict holds at most %d (this is not the limit of %d matched nodes)"
                                      % (i0 + int(np.argmax(rawlen)), W, _UNION_MAX, _NODES_MAX))
        idx = np.empty((n, W), dtype=np.int64)
        eng.net_table(nsel, sel, mt.sel32, mt.off, mt.items, W, idx)
        nb = np.empty((n, W), dtype=np.int64); nn_ = np.empty(n, dtype=np.int64)
        eng.upload_models(self.models, self.models_err, self.models_mask)
        ko = pdfs = lmap = levid = None
        if predict is not None:
            ko, G = self._labels(eng, *predict)
            pdfs = np.empty((n, G)); lmap = np.empty(n); levid = np.empty(n)
        opts = like_opts({} if host_lprob else lprob_kwargs)
        lnl = np.empty((n, W)); c2 = np.empty((n, W)); nd = np.empty((n, W), dtype=np.int64)
        s_ = np.empty((n, W)); se_ = np.empty((n, W))
        eng.knn_fit_predict(obj.x, obj.xe, obj.xm, idx, W, opts, ko, nb, nn_, lnl, c2, nd, s_, se_,
                            *((None, None, None) if host_lprob else (pdfs, lmap, levid)))
        obj.writeback()
        if not host_lprob:
            planes = [np.zeros((n, W)), lnl, lnl, nd, c2, s_, se_][:7 if lprob_kwargs.get('return_scale', False) else 5]
            return nb, nn_, lambda k, m: [p[k, :m].copy() for p in planes], pdfs, lmap, levid
        # the user's likelihood on each object's model subset (networks.py:925-928), the PDFs from its ln-posteriors; the result of
        # an object is the user's own tuple, as it came
        X, Xe, Xm = chunk
        lw = np.full((n, W), -np.inf)
        rows = []
        for k in range(n):
            ii = nb[k, :nn_[k]]
            r = lprob_func(X[k], Xe[k], Xm[k], self.models[ii], self.models_err[ii], self.models_mask[ii], *lprob_args, **lprob_kwargs)
            rows.append(r); lw[k, :nn_[k]] = r[2]
        if predict is not None:
            # (the user's function may have used this device's context itself -- the package's own logprob does: the model and
            #  label sets are put back before the PDFs are stacked)
            ko, _ = self._labels(eng, *predict)
            eng.knn_predict_logwt(lw, nb, nn_, W, ko, pdfs, lmap, levid)
        return nb, nn_, lambda k, m: rows[k], pdfs, lmap, levid

    def _emit(self, i0, save_fits, track_scale, nb, nn, results_of, pdfs, lmap, levid):
        """What a fit path returns of the chunk at ``i0`` -- neighbour table (n, W), counts (n), ``results_of(k, m)`` = the result tuple
        of object k with its m neighbours, PDFs with lmap / levid or None -- as per-object tuples (idxs, Nidx, results[, pdf, (lmap,
        levid)]); stores the fits like the reference when save_fits."""
        out = []
        for k in range(len(nn)):
            m = int(nn[k])
            idxs = nb[k, :m].copy()
            results = results_of(k, m)
            if save_fits:
                self.Nneighbors[i0 + k] = m
                self.neighbors.append(np.array(idxs))
                self.fit_lnprior.append(results[0]); self.fit_lnlike.append(results[1]); self.fit_lnprob.append(results[2])
                self.fit_Ndim.append(results[3]); self.fit_chi2.append(results[4])
                if track_scale:
                    self.fit_scale.append(results[5]); self.fit_scale_err.append(results[6])
            out.append((idxs, m, results) if pdfs is None else (idxs, m, results, pdfs[k], (lmap[k], levid[k])))
        return out

    # -- networks.py:782-936 -----------------------------------------------------------------------------
    def fit(self, data, data_err, data_mask, lprob_func=None, nodes_only=False, wt_thresh=1e-3, cdf_thresh=2e-4, lprob_args=None,
            lprob_kwargs=None, track_scale=False, discrete=False, verbose=True):
        self._run(data, data_err, data_mask, lprob_func, nodes_only, wt_thresh, cdf_thresh, lprob_args, lprob_kwargs, track_scale,
                  discrete, True)
        if verbose:
            sys.stderr.write('\rFitting object {0}/{0}\n'.format(len(data))); sys.stderr.flush()

    def _fit(self, data, data_err, data_mask, lprob_func=None, nodes_only=False, wt_thresh=1e-3, cdf_thresh=2e-4, lprob_args=None,
             lprob_kwargs=None, track_scale=False, discrete=False, save_fits=True):
        yield from self._run(data, data_err, data_mask, lprob_func, nodes_only, wt_thresh, cdf_thresh, lprob_args, lprob_kwargs,
                             track_scale, discrete, save_fits)

    # -- extension: the fit as sparse rows (docs/network.md, "Sparse rows") ---------------------------------------------------
    def fit_sparse(self, data, data_err, data_mask, lprob_func=None, wt_thresh=1e-3, cdf_thresh=2e-4, lprob_args=None,
                   lprob_kwargs=None, track_scale=False, discrete=False, resident=False, verbose=True):
        """Extension (no reference counterpart; docs/network.md, "Sparse rows"): the fit of ``fit`` -- the same selection of nodes,
        the built-in likelihood of every object against the models its selected nodes list -- left as a ``SparseFits`` in the layout
        ``NearestNeighbors.fit`` leaves, so that ``predict`` / ``sample`` / ``weight_sampler`` / ``weight_em`` / ``moments`` /
        ``predict_bins`` / ``predict_cdf`` / ``predict_quantiles`` / ``predict_phot`` run on a fit through the network.  The
        candidate set of an object is the union of its nodes' lists with repeats removed (``fz_net_union``), and the width of the
        rows is the largest such union of the call (at most ``FZ_KNN_WMAX``), not the summed list length ``fit`` is sized by.
        ``neighbors`` holds each row's model indices in ASCENDING order, padded -99 (column 0 is the smallest index, not the MAP
        model); ``lmap`` / ``levid`` are the max / logsumexp of the row and ``cover()`` is 1.  There is no ``nodes_only``.  No
        attribute of this object is touched; the in-place clean of the objects reaches the caller's arrays.  ``resident=True``
        leaves ``neighbors``, ``Nneighbors``, ``fit_lnlike`` and ``fit_lnprob`` as device arrays of the engine (the other ``fit_*``
        are then None)."""
        if self.nodes_idxs is None:
            raise ValueError("Network has not been trained!")
        if not (_is_default(lprob_func) and not lprob_args):
            raise NotImplementedError("fit_sparse needs the built-in likelihood (a foreign `lprob_func` returns rows of its own "
                                      "layout: use `fit`)")
        if not (_is_default(getattr(self, 'lpnet_func', None)) and not getattr(self, 'lpnet_args', None)):
            raise NotImplementedError("fit_sparse needs a network populated with the built-in node likelihood (`lpnet_func`)")
        if self.NMODEL > _UNION_MMAX:
            raise NotImplementedError("%d models exceed FZ_NET_UNION_MMAX = %d (an object's bitmap of the models sits in LDS)"
                                      % (self.NMODEL, _UNION_MMAX))
        opts = like_opts(lprob_kwargs)
        eng, mt, Ndata, thresh = self._eng(), self._matched(discrete), len(data), (wt_thresh, cdf_thresh)
        lists = eng.device_array(mt.sel32), eng.device_array(mt.off), eng.device_array(mt.items)
        # Objects per device call: the (n, Nn) node plane, sel (n, Nn) int32, nsel and the counts inside a quarter of the workspace
        # budget.  The selection of the counting pass stays on the device for the fitting pass while all of it fits another quarter;
        # otherwise the fitting pass forms it again, chunk by chunk.
        limit = eng.workspace_limit()
        sel_row = mt.Nn * 4 + 4
        keep = Ndata * sel_row <= limit // 4
        kept = (eng.device_empty((Ndata,), np.int32), eng.device_empty((Ndata, mt.Nn), np.int32)) if keep and Ndata else None
        chunks = lambda per_object, form: _sparse_chunks(eng, mt, self.lpnet_kwargs, (data, data_err, data_mask), thresh, kept,
                                                         int(max(1, min(_NET_CHUNK, (limit // 4) // per_object))), form)
        # ---- pass 1: the selections and the sizes of the unions; every refusal falls here, before the first subset fit ----
        nuniq = np.zeros(Ndata, dtype=np.int64)
        for i0, n, _, d_nsel, d_sel in chunks(mt.Nn * 8 + (0 if keep else sel_row) + 8, True):
            nsel = np.empty(n, dtype=np.int32)
            eng.dev_copy(nsel, d_nsel, nsel.nbytes)
            _refuse_no_node(nsel, i0, *thresh)
            eng.net_union(d_nsel, d_sel, *lists, self.NMODEL, nuniq[i0:i0 + n], n=n, nn=mt.Nn)
            _refuse_no_model(nuniq[i0:i0 + n], i0)
        W = max(int(nuniq.max()), 1) if Ndata else 1
        if W > _UNION_MAX:
            raise NotImplementedError("object %d: its selected nodes list %d different models; the union table of fz_knn_fit_predict "
                                      "holds at most FZ_KNN_WMAX = %d" % (int(np.argmax(nuniq)), W, _UNION_MAX))
        sf = self._sparse_rows(eng, mt, lists, chunks(W * 8 + (0 if keep else mt.Nn * 8 + sel_row), not keep), Ndata, W, opts,
                               track_scale, resident)
        if verbose:
            sys.stderr.write('\rFitting object {0}/{0}\n'.format(Ndata)); sys.stderr.flush()
        return sf

    def _sparse_rows(self, eng, mt, lists, chunks, Ndata, W, opts, track_scale, resident):
        """pass 2 of ``fit_sparse``: the tables and the subset likelihood, straight into rows [i0, i0 + n) of the (Ndata, W) outputs"""
        from .sparse import SparseFits
        free = track_scale and bool(opts.free_scale)
        if resident:
            new = lambda dt: eng.device_empty((Ndata, W), dt)
            nbr, cnt = new(np.int64), eng.device_empty((Ndata,), np.int64)
            lnl, lpb = new(np.float64), new(np.float64)
            lpr = chi2 = ndim = sc = se = None
        else:
            new = lambda dt: np.empty((Ndata, W), dtype=dt)
            nbr, cnt = new(np.int64), np.zeros(Ndata, dtype=np.int64)
            lnl, chi2, ndim = new(np.float64), new(np.float64), new(np.int64)
            sc, se = (new(np.float64), new(np.float64)) if free else (None, None)
        for i0, n, obj, d_nsel, d_sel in chunks:
            idx = eng.device_empty((n, W), np.int64)
            nu = eng.device_empty((n,), np.int64)
            eng.net_union(d_nsel, d_sel, *lists, self.NMODEL, nu, W, idx, n=n, nn=mt.Nn)
            eng.upload_models(self.models, self.models_err, self.models_mask)
            # (rows of an output: a view of a host array, the address of the row in a device array)
            rows = [a if a is None else a[i0:i0 + n] if isinstance(a, np.ndarray) else a.row_ptr(i0)
                    for a in (nbr, cnt, lnl, chi2, ndim, sc, se)]
            eng.knn_fit_predict(obj.x, obj.xe, obj.xm, idx, W, opts, None, *rows, n=n)
            obj.writeback()
        # ln-prior zero on the subset, so ln-prob = ln-like; lmap / levid: max and logsumexp of the rows, which fz_sparsify_logwt
        # forms of the FULL row it is given (here: the row of W entries, one of them kept)
        lmap, levid = np.zeros(Ndata), np.zeros(Ndata)
        if resident:
            if Ndata:
                eng.dev_copy(lpb, lnl, lnl.nbytes)
        else:
            lpb = lnl.copy()
            lpr = np.where(np.arange(W)[None, :] < cnt[:, None], 0.0, -np.inf)
            if track_scale and not free:                          # (a fixed scale: 1 and 0 throughout, as ``fit`` leaves them)
                sc, se = np.ones((Ndata, W)), np.zeros((Ndata, W))
        if Ndata:
            eng.sparsify_logwt(lpb, 1, -np.inf, eng.device_empty((Ndata, 1), np.int64), eng.device_empty((Ndata,), np.int64), lmap=lmap,
                               levid=levid, n=Ndata, M=W)
        return SparseFits(nbr, cnt, self.NMODEL, lmap, levid, levid.copy(), lpr, lnl, lpb, ndim, chi2, sc, se, device=self._device)

    # -- networks.py:938-1128 ----------------------------------------------------------------------------
    def predict(self, model_labels, model_label_errs, label_dict=None, label_grid=None, logwt=None, kde_args=None, kde_kwargs=None,
                return_gof=False, discrete=False, verbose=True):
        if logwt is None:
            logwt = self.fit_lnprob
        if label_dict is None and label_grid is None:
            raise ValueError("`label_dict` or `label_grid` must be specified.")
        if self.fit_lnprob is None and logwt is None:
            raise ValueError("Fits have not been computed and weights have not been provided.")
        eng = self._eng()
        N = self.NDATA
        lens = np.array([len(v) for v in logwt], dtype=np.int64)
        W = max(int(lens.max()), 1)
        lw = _padded(logwt, lens, N, W, -np.inf, np.float64)
        nb = _padded(np.zeros(N, dtype=np.int64) if self.nodes_only else self.neighbors, lens, N, W, 0, np.int64)
        if self.nodes_only:
            # stack the node PDFs by the relative weights of the stored node fits (networks.py:1113-1115)
            node_pdfs = np.ascontiguousarray(self.get_pdfs(model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs,
                                                           False, discrete, verbose))
            G = node_pdfs.shape[1]
            # columns = positions in the stored lists; `match` maps them to the nodes
            pdfs = np.empty((N, G)); lmap = np.empty(N); levid = np.empty(N)
            sel = np.ascontiguousarray(np.broadcast_to(np.arange(W, dtype=np.int32), (N, W)))
            for i in range(N):
                # (one object at a time: every object has its own column -> node map)
                mt = np.zeros(W, dtype=np.int32); mt[:lens[i]] = self.neighbors[i]
                eng.net_stack(np.ascontiguousarray(lw[i:i + 1]), lens[i:i + 1].astype(np.int32), sel[i:i + 1], mt, node_pdfs,
                              pdfs[i:i + 1], lmap[i:i + 1], levid[i:i + 1])
        else:
            ko, G = self._labels(eng, model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs)
            pdfs = np.empty((N, G)); lmap = np.empty(N); levid = np.empty(N)
            eng.knn_predict_logwt(lw, nb, lens, W, ko, pdfs, lmap, levid)
        if verbose:
            sys.stderr.write('\rGenerating PDF {0}/{0}\n'.format(N)); sys.stderr.flush()
        return (pdfs, (lmap, levid)) if return_gof else pdfs

    def _predict(self, model_labels, model_label_errs, node_pdfs=None, label_dict=None, label_grid=None, logwt=None, kde_args=None,
                 kde_kwargs=None):
        if self.nodes_only and node_pdfs is None:
            raise ValueError("Fits were only computed to nodes in the network but the relevant `node_pdfs` are not provided.")
        pdfs, (lmap, levid) = self.predict(model_labels, model_label_errs, label_dict, label_grid, logwt, kde_args, kde_kwargs, True,
                                           False, False)
        for i in range(len(pdfs)):
            yield pdfs[i], (lmap[i], levid[i])

    # -- networks.py:1130-1473 ---------------------------------------------------------------------------
    def fit_predict(self, data, data_err, data_mask, model_labels, model_label_errs, lprob_func=None, nodes_only=False, wt_thresh=1e-3,
                    cdf_thresh=2e-4, label_dict=None, label_grid=None, kde_args=None, kde_kwargs=None, lprob_args=None,
                    lprob_kwargs=None, return_gof=False, track_scale=False, discrete=False, verbose=True, save_fits=True):
        if label_dict is None and label_grid is None:
            raise ValueError("`label_dict` or `label_grid` must be specified.")
        res = self._run(data, data_err, data_mask, lprob_func, nodes_only, wt_thresh, cdf_thresh, lprob_args, lprob_kwargs, track_scale,
                        discrete, save_fits, (model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs))
        pdfs = np.array([r[3] for r in res]); lmap = np.array([r[4][0] for r in res]); levid = np.array([r[4][1] for r in res])
        if verbose:
            sys.stderr.write('\rGenerating PDF {0}/{0}\n'.format(len(data))); sys.stderr.flush()
        return (pdfs, (lmap, levid)) if return_gof else pdfs

    def _fit_predict(self, data, data_err, data_mask, model_labels, model_label_errs, lprob_func=None, node_pdfs=None, wt_thresh=1e-3,
                     cdf_thresh=2e-4, label_dict=None, label_grid=None, kde_args=None, kde_kwargs=None, lprob_args=None,
                     lprob_kwargs=None, track_scale=False, discrete=False, save_fits=True):
        for r in self._run(data, data_err, data_mask, lprob_func, node_pdfs is not None, wt_thresh, cdf_thresh, lprob_args, lprob_kwargs,
                           track_scale, discrete, save_fits, (model_labels, model_label_errs, label_dict, label_grid, kde_args, kde_kwargs)):
            yield r[3], r[4]


# ---- training of a self-organizing map (reference networks.py:38-118, 1490-1867) ----------------------------------------------------
# The schedules and neighbourhoods below keep the reference's signatures and arithmetic (the kernel is tested against its runs bit
# for bit).  The device path recognises them by identity, as _is_default does for logprob, and tabulates the learning rate and the
# sigma of every step up front; other callables go through _som_host_steps.

def learn_linear(t, start=0.5, end=0.1, *args, **kwargs):
    """Learning rate at run fraction ``t`` in [0, 1]: a straight line from ``start`` to ``end``."""
    return (1. - t) * start + t * end


def learn_geometric(t, start=0.5, end=0.1, *args, **kwargs):
    """Learning rate at run fraction ``t``: from ``start`` to ``end`` by a constant ratio (linear in the logarithm)."""
    return np.exp((1. - t) * np.log(start) + t * np.log(end))


def learn_harmonic(t, start=0.5, end=0.1, *args, **kwargs):
    """Learning rate at run fraction ``t``: its reciprocal runs linearly from 1 / ``start`` to 1 / ``end``."""
    return 1. / ((1. - t) / start + t / end)


_LEARN_RATES = {'linear': learn_linear, 'geometric': learn_geometric, 'harmonic': learn_harmonic}


def _schedule(rate):
    if rate not in _LEARN_RATES:
        raise ValueError("Provided `rate` is not supported.")
    return _LEARN_RATES[rate]


def neighbor_gauss(t, pos, positions, nside, start=0.7, end=0.02, rate='harmonic', *args, **kwargs):
    """Weights of the grid ``positions`` around ``pos``: a Gaussian in grid distance whose width runs from ``start * nside`` to
    ``end * nside`` on the ``rate`` schedule (``nside`` None: a square grid is assumed).  Returns ``(weights, sigma)``."""
    schedule = _schedule(rate)
    side = np.sqrt(len(positions)) if nside is None else nside
    d2 = np.sum((pos - positions)**2, axis=1)
    sigma = schedule(t, start=start, end=end) * side
    return np.exp(-0.5 * d2 / sigma**2), sigma


def neighbor_lorentz(t, pos, positions, nside, start=0.7, end=0.02, rate='harmonic', *args, **kwargs):
    """As ``neighbor_gauss`` with a Lorentzian profile, sigma^2 / (d^2 + sigma^2).  Returns ``(weights, sigma)``."""
    schedule = _schedule(rate)
    d2 = np.sum((pos - positions)**2, axis=1)
    sigma = schedule(t, start=start, end=end) * nside
    return sigma**2 / (d2 + sigma**2), sigma


def som_nodes_pos(nside, nproj):
    """(nside**nproj, nproj) float grid coordinates: coordinate i of node n is digit i of n written in base nside, most
    significant digit first (the layout of the reference's networks.py:1804-1810)."""
    n = np.arange(nside**nproj)
    return np.stack([(n // nside**(nproj - 1 - i)) % nside for i in range(nproj)], axis=1).astype(np.float64)


def _som_selection(w, wt_thresh, cdf_thresh):
    """indices of the nodes one step moves: weights above ``wt_thresh`` of the largest, or (``wt_thresh`` None) the smallest
    weights, taken in ascending order while their normalised running sum stays within 1 - ``cdf_thresh``"""
    if wt_thresh is not None:
        return np.flatnonzero(w > wt_thresh * np.max(w))
    order = np.argsort(w)
    running = np.cumsum((w / np.sum(w))[order])
    return order[running <= 1. - cdf_thresh]


_SOM_SEGMENT = 10000          # training steps per kernel launch (the map stays on the device between launches)


def _learn_table(func, times, args, kwargs):
    """func(t, *args, **kwargs) for every t.  The +-*/ forms give the same numbers on the whole array; anything else (np.exp / np.log
    in learn_geometric, the user's callable) is called per t."""
    if func is learn_linear or func is learn_harmonic:
        return np.broadcast_to(np.asarray(func(times, *args, **kwargs), dtype=np.float64), times.shape).copy()
    return np.array([func(t, *args, **kwargs) for t in times], dtype=np.float64)


def _sigma_table(func, times, nside, args, kwargs):
    """the sigma neighbor_gauss / neighbor_lorentz returns at every t"""
    import inspect
    b = inspect.signature(func).bind(0., None, None, nside, *args, **kwargs)
    b.apply_defaults()
    schedule = _schedule(b.arguments['rate'])
    return _learn_table(schedule, times, (), {'start': b.arguments['start'], 'end': b.arguments['end']}) * nside


def _draw_stream(rstate, nmodel, T):
    """the rows rstate.choice(Nmodel) draws at each of T steps: for the legacy RandomState one randint call of size T is the same
    stream; any other generator is asked T times"""
    if rstate is np.random or isinstance(rstate, np.random.RandomState):
        return np.ascontiguousarray(rstate.randint(0, nmodel, size=T), dtype=np.int64)
    return np.array([rstate.choice(nmodel) for _ in range(T)], dtype=np.int64)


def _clean_rows(x, xe, xm, rows):
    """pdf.py:309-311 on the given rows of the arrays, in place"""
    if not len(rows):
        return
    cx, ce = np.asarray(x[rows], dtype=np.float64), np.asarray(xe[rows], dtype=np.float64)
    bad = ~(np.isfinite(cx) & np.isfinite(ce) & (ce > 0.))
    if not bad.any():
        return
    sel = np.zeros(np.shape(x), dtype=bool)
    sel[rows] = bad
    x[sel], xe[sel], xm[sel] = 0., 1., False


def _given(value, default):
    return default if value is None else value


def _training_opts(lprob_kwargs, track_scale):
    """the likelihood options of a device training run; track_scale needs the scale back"""
    opts = like_opts(lprob_kwargs)
    if track_scale and not (opts.free_scale and lprob_kwargs.get('return_scale', False)):
        raise ValueError("track_scale=True needs a likelihood that returns the scale (free_scale=True, return_scale=True)")
    return opts


def _training_inputs(rstate, models, models_err, models_mask, T):
    """The inputs of a device training run: the rows drawn at the T steps (rstate.choice per step) and fp64 copies of the models
    cleaned up front (pdf.py:309-311).  The reference cleans every drawn row of the caller's arrays in place, and so do we, once,
    before the run."""
    draws = _draw_stream(rstate, len(models), T)
    x, xe, xm = (np.array(a, dtype=np.float64, order='C') for a in (models, models_err, models_mask))
    _clean_rows(x, xe, xm, np.arange(len(models)))
    _clean_rows(models, models_err, models_mask, np.unique(draws))
    return draws, x, xe, xm


def _device_arrays(device, arrays):
    """device copies of the training arrays (torch on this engine's GPU), so that the network stays on the device between launches;
    without torch the library stages the host arrays itself"""
    try:
        import torch
        if not torch.cuda.is_available():
            return arrays
    except ImportError:
        return arrays
    d = torch.device('cuda', device)
    return tuple(torch.from_numpy(a).to(d) for a in arrays)


class SelfOrganizingMap(Network):
    """The reference's ``SelfOrganizingMap``: ``train_network`` runs on the device (``fz_som_train``, one persistent workgroup per
    map, docs/som.md); inference is the inherited ``Network``."""

    def train_network(self, models=None, models_err=None, models_mask=None, nside=50, nproj=2, nodes_init=None, niter=2000,
                      nbatch=50, err_kernel=None, lprob_func=None, learn_func=None, neighbor_func=None, wt_thresh=1e-3,
                      cdf_thresh=2e-4, rstate=None, lprob_args=None, lprob_kwargs=None, track_scale=False, learn_args=None,
                      learn_kwargs=None, neighbor_args=None, neighbor_kwargs=None, verbose=True):
        """Fit ``nside**nproj`` nodes on an ``nproj``-dimensional grid to the models (by default the ones the map was built with)
        over ``niter * nbatch`` steps.  Keywords and defaults are the reference's (networks.py:1517-1681); afterwards ``nodes``,
        ``nodes_pos``, ``NSIDE``, ``NNODE``, ``NPROJ``, ``NITER`` and ``NBATCH`` hold the trained map."""
        models, models_err, models_mask = self._training_models(models, models_err, models_mask, err_kernel)
        steps = self._train_network(models, models_err, models_mask, lprob_func=lprob_func, nside=nside, nproj=nproj,
                                    nodes_init=nodes_init, learn_func=learn_func, neighbor_func=neighbor_func, niter=niter,
                                    nbatch=nbatch, wt_thresh=wt_thresh, cdf_thresh=cdf_thresh, rstate=rstate, lprob_args=lprob_args,
                                    lprob_kwargs=lprob_kwargs, track_scale=track_scale, learn_args=learn_args,
                                    learn_kwargs=learn_kwargs, neighbor_args=neighbor_args, neighbor_kwargs=neighbor_kwargs)
        for step, (_, _, rate, width) in enumerate(steps):
            if verbose and step % nbatch == 0:                            # once per batch, the reference's progress line
                sys.stderr.write('\rIteration %d/%d [learn=%6.3f, sigma=%6.3f]     ' % (step // nbatch + 1, niter, rate, width))
                sys.stderr.flush()
        if verbose:
            sys.stderr.write('\n')
            sys.stderr.flush()

    def _train_network(self, models, models_err, models_mask, lprob_func=None, nside=50, nproj=2, nodes_init=None, learn_func=None,
                       neighbor_func=None, niter=2000, nbatch=50, wt_thresh=1e-3, cdf_thresh=2e-4, rstate=None, lprob_args=None,
                       lprob_kwargs=None, track_scale=False, learn_args=None, learn_kwargs=None, neighbor_args=None,
                       neighbor_kwargs=None):
        """Generator of the training steps, ``(node_results, bmu, learn_rate, learn_sigma)`` each.  On the device path
        ``node_results`` is None: the (T, Nnode) likelihood rows are never formed (docs/deviations.md)."""
        lprob_func = _given(lprob_func, _pdf.logprob)
        lprob_args = _given(lprob_args, [])
        lprob_kwargs = _given(lprob_kwargs, {'free_scale': True, 'ignore_model_err': True})
        learn_func, learn_args, learn_kwargs = _given(learn_func, learn_harmonic), _given(learn_args, []), _given(learn_kwargs, {})
        neighbor_func = _given(neighbor_func, neighbor_gauss)
        neighbor_args, neighbor_kwargs = _given(neighbor_args, []), _given(neighbor_kwargs, {})
        rstate = _given(rstate, np.random)
        use_wt, wt, cdf = _selection_rule(wt_thresh, cdf_thresh)          # (neither given: no thresholding at all)
        T = niter * nbatch
        times = np.linspace(0., 1., T)
        self.NITER, self.NBATCH = niter, nbatch
        self.NSIDE, self.NNODE, self.NPROJ = nside, nside**nproj, nproj
        self.nodes_pos = som_nodes_pos(nside, nproj)
        # initial nodes: distinct model rows as they stand (before any cleaning), or nodes_init itself, which is then trained in place
        self.nodes = np.array(models[rstate.choice(len(models), size=self.NNODE, replace=False)]) if nodes_init is None else nodes_init

        if not (_is_default(lprob_func) and not lprob_args and neighbor_func in (neighbor_gauss, neighbor_lorentz)):
            for step in self._som_host_steps(models, models_err, models_mask, times, rstate, lprob_func, lprob_args, lprob_kwargs,
                                             learn_func, learn_args, learn_kwargs, neighbor_func, neighbor_args, neighbor_kwargs,
                                             wt if use_wt else None, cdf_thresh, track_scale):
                yield step
            return

        opts = _training_opts(lprob_kwargs, track_scale)
        draws, x, xe, xm = _training_inputs(rstate, models, models_err, models_mask, T)
        # the other tables of the whole run: learning rates, sigmas
        lr = _learn_table(learn_func, times, learn_args, learn_kwargs)
        sig = _sigma_table(neighbor_func, times, self.NSIDE, neighbor_args, neighbor_kwargs)
        nodes = np.array(self.nodes, dtype=np.float64, order='C')
        if nodes.shape != (self.NNODE, x.shape[1]):
            raise ValueError("nodes_init must have shape (nside**nproj, Nfilt) = %r" % ((self.NNODE, x.shape[1]),))
        pos = np.ascontiguousarray(self.nodes_pos, dtype=np.int32)
        bmus = np.zeros(T, dtype=np.int32)
        eng = self._eng()
        kind = 0 if neighbor_func is neighbor_gauss else 1
        dx, dxe, dxm, dnodes, dpos, ddraws, dlr, dsig, dbmus = _device_arrays(eng.device, (x, xe, xm, nodes, pos, draws, lr, sig, bmus))
        seg = max(1, int(_SOM_SEGMENT))
        for s0 in range(0, T, seg):
            s1 = min(T, s0 + seg)
            eng.som_train(dx, dxe, dxm, dnodes, dpos, ddraws, dlr, dsig, kind, use_wt, wt, cdf, opts, track_scale, s0, s1, dbmus)
            if dnodes is not nodes:
                nodes[...] = dnodes.cpu().numpy()
                bmus[s0:s1] = dbmus[s0:s1].cpu().numpy()
            if nodes_init is not None and isinstance(nodes_init, np.ndarray):
                nodes_init[...] = nodes                  # the reference trains nodes_init itself
                self.nodes = nodes_init
            else:
                self.nodes = nodes.copy()
            for i in range(s0, s1):
                yield None, int(bmus[i]), lr[i], sig[i]

    def _som_host_steps(self, models, models_err, models_mask, times, rstate, lprob_func, lprob_args, lprob_kwargs, learn_func,
                        learn_args, learn_kwargs, neighbor_func, neighbor_args, neighbor_kwargs, wt_thresh, cdf_thresh, track_scale):
        """The training steps with the user's callables, called with the arguments the reference passes them: one drawn model
        against the nodes as noiseless, unmasked models, then the schedule and the neighbourhood of the best node.  The map
        (``self.nodes``) is updated in place; the drawn row is read again after the likelihood call, which may clean it."""
        nodes, grid = self.nodes, self.nodes_pos
        noiseless, unmasked = np.zeros_like(nodes), np.ones_like(nodes, dtype='bool')
        for t in times:
            row = rstate.choice(len(models))
            fits = lprob_func(models[row], models_err[row], models_mask[row], nodes, noiseless, unmasked, *lprob_args, **lprob_kwargs)
            if track_scale:
                nodes *= fits[5][:, None]                                 # rescaled after the fit, before the update
            best = np.argmax(fits[2])
            rate = learn_func(t, *learn_args, **learn_kwargs)
            wts, width = neighbor_func(t, grid[best], grid, self.NSIDE, *neighbor_args, **neighbor_kwargs)
            moved = _som_selection(wts, wt_thresh, cdf_thresh)
            nodes[moved] += rate * wts[moved, None] * (models[row] - nodes[moved])
            yield fits, best, rate, width


# ---- training of a growing neural gas (reference networks.py:1870-2260) --------------------------------------------------------------
# The network is kept as plain arrays -- labels, positions, errors, ordered adjacency lists, edge ages -- on the device
# (fz_gng_train, docs/gng.md) and in the host loop alike; networkx is needed only for ``self.graph`` and ``graph_init``.

_GNG_MAX_DEGREE = 64          # neighbours per node the device's adjacency lists hold (the default-size reference run peaks at 18)
_GNG_MAX_NODES = 65536        # max(max_nodes, initial nodes) the device path takes (FZ_GNG_MAX_NODES)
_GNG_SEGMENT = 10000          # training steps per kernel launch (the network stays on the device between launches)
_GNG_NCNT = 16                # counters at the head of the integer state (include/frankenz_hip.h)


def _gng_state_sizes(cap, B, md, pcap, ecap):
    """(doubles, int32s) of the two state arrays of fz_gng_train"""
    return 2 * cap * B + cap + 2 * B, _GNG_NCNT + 2 * cap + 4 * cap * md + 3 * pcap + ecap


def _gng_read_graph(graph):
    """a networkx-style graph with ``pos``, ``error`` and ``age`` attributes -> labels, positions (the graph's own arrays), errors
    and per-node neighbour labels / ages, in the graph's node and adjacency order"""
    ids = list(graph.nodes())
    pos = [graph.nodes[n]['pos'] for n in ids]
    err = [graph.nodes[n]['error'] for n in ids]
    nbrs = [list(graph.neighbors(n)) for n in ids]
    ages = [[graph.edges[n, m]['age'] for m in nb] for n, nb in zip(ids, nbrs)]
    return ids, pos, err, nbrs, ages


def _gng_fill_graph(graph, ids, pos, err, off, nbr, age):
    """the arrays -> ``graph`` (emptied first): node attributes ``pos``, ``error``, ``count``, edge attribute ``age``, nodes and every
    node's neighbours in the given order.  The adjacency is written directly (``graph._adj``): no sequence of ``add_edge`` calls
    is known that leaves every node's neighbours in a prescribed order."""
    graph.clear()
    for k, n in enumerate(ids):
        graph.add_node(n, pos=pos[k], error=err[k], count=k)
    attrs = {}
    for k, n in enumerate(ids):
        for j in range(off[k], off[k + 1]):
            m = ids[nbr[j]]
            key = (k, nbr[j]) if k < nbr[j] else (nbr[j], k)
            if key not in attrs:
                attrs[key] = {'age': int(age[j])}
            graph._adj[n][m] = attrs[key]
    return graph


class GrowingNeuralGas(Network):
    """The reference's ``GrowingNeuralGas``: ``train_network`` runs on the device (``fz_gng_train``, one persistent workgroup per
    network, docs/gng.md); inference is the inherited ``Network``.  After training the network is held as plain arrays, in the
    reference's node order: ``graph_ids`` (labels), ``graph_pos`` (NNODE, Nfilt), ``graph_errors``, and the adjacency in neighbour
    order as CSR -- ``graph_adj_off`` (NNODE + 1), ``graph_adj_nbr`` (node indices), ``graph_adj_age``.  ``graph`` is the same
    network as a ``networkx.Graph`` with the reference's attributes (``pos``, ``error``, ``count``; ``age``), or None where networkx
    is not installed."""

    def __init__(self, models, models_err, models_mask, device=None):
        super(GrowingNeuralGas, self).__init__(models, models_err, models_mask, device=device)
        self.graph = _new_graph()
        self.graph_ids = self.graph_pos = self.graph_errors = self.graph_adj_off = self.graph_adj_nbr = self.graph_adj_age = None

    def train_network(self, models=None, models_err=None, models_mask=None, learn_best=0.2, learn_neighbor=0.005, max_age=15,
                      nbatch=50, new_err_dec=0.5, all_err_dec=5e-3, max_nodes=2500, niter=5000, graph_init=None, err_kernel=None,
                      lprob_func=None, rstate=None, lprob_args=None, lprob_kwargs=None, track_scale=False, verbose=True):
        """Grow a network of at most ``max_nodes`` nodes on the models (by default the ones the object was built with) over
        ``niter * nbatch`` steps.  Keywords and defaults are the reference's (networks.py:1898-2035); afterwards ``nodes``,
        ``NNODE``, ``graph`` and the ``graph_*`` arrays hold the trained network."""
        models, models_err, models_mask = self._training_models(models, models_err, models_mask, err_kernel)
        steps = self._train_network(models, models_err, models_mask, learn_best=learn_best, learn_neighbor=learn_neighbor,
                                    max_age=max_age, nbatch=nbatch, new_err_dec=new_err_dec, all_err_dec=all_err_dec,
                                    max_nodes=max_nodes, niter=niter, graph_init=graph_init, lprob_func=lprob_func, rstate=rstate,
                                    lprob_args=lprob_args, lprob_kwargs=lprob_kwargs, track_scale=track_scale)
        for i, (_, _, nnodes, nprune) in enumerate(steps):
            if i % nbatch == 0 and verbose:                               # once per batch, the reference's progress line
                sys.stderr.write('\rIteration {0}/{1} [nodes={2}, edges pruned={3}] '.format(int(i / nbatch) + 1, niter, nnodes, nprune))
                sys.stderr.flush()
        if verbose:
            sys.stderr.write('\n')
            sys.stderr.flush()

    def _train_network(self, models, models_err, models_mask, learn_best=0.2, learn_neighbor=0.005, max_age=15, nbatch=50,
                       new_err_dec=0.5, all_err_dec=5e-3, max_nodes=2500, niter=5000, graph_init=None, lprob_func=None, rstate=None,
                       lprob_args=None, lprob_kwargs=None, track_scale=False, verbose=True):
        """Generator of the training steps, ``(node_results, bmu, NNODE, nprune)`` each.  On the device path ``node_results`` is
        None: the (T, Nnode) likelihood rows are never formed (docs/deviations.md)."""
        lprob_func = _given(lprob_func, _pdf.logprob)
        lprob_args = _given(lprob_args, [])
        lprob_kwargs = _given(lprob_kwargs, {'free_scale': True, 'ignore_model_err': True})
        rstate = _given(rstate, np.random)
        Nmodel, B = len(models), np.shape(models)[1]
        T = int(niter) * int(nbatch)
        nbatches = (T - 1) // nbatch + 1 if T > 0 else 0
        device = _is_default(lprob_func) and not lprob_args
        nn0 = 2 if graph_init is None else graph_init.number_of_nodes()
        if device:
            # the device path's limits, refused before anything is drawn or touched
            if B > 32:
                raise NotImplementedError("GrowingNeuralGas.train_network: %d bands unsupported on the device (at most 32)" % B)
            if max(int(max_nodes), nn0) > _GNG_MAX_NODES:
                raise NotImplementedError("GrowingNeuralGas.train_network: max(max_nodes, initial nodes) = %d unsupported on the "
                                          "device (at most %d)" % (max(int(max_nodes), nn0), _GNG_MAX_NODES))
            if T >= 1 << 30:
                raise NotImplementedError("GrowingNeuralGas.train_network: %d steps unsupported on the device (below 2**30)" % T)
            opts = _training_opts(lprob_kwargs, track_scale)
        if nn0 < 2:
            raise ValueError("graph_init needs at least two nodes")

        if graph_init is None:
            i1, i2 = (int(v) for v in rstate.choice(Nmodel, size=2, replace=False))
            ids, pos, err = [0, 1], [models[i1], models[i2]], [0., 0.]    # the positions are views: training rewrites the two rows
            nbrs, ages = [[1], [0]], [[0], [0]]
            alias = (i1, i2)
        else:
            ids, pos, err, nbrs, ages = _gng_read_graph(graph_init)
            alias = (-1, -1)
            taken = set(ids)
            clash = [nn0 + k for k in range(nbatches) if nn0 + k in taken]
            if clash:
                # (the reference would silently overwrite that node's position and error with the new node's)
                raise ValueError("graph_init: the label %r of a node to be inserted is already in the graph" % (clash[0],))
        self.NNODE = nn0

        if device and graph_init is None:
            rows = np.array(alias)
            cx, ce = np.asarray(models[rows], dtype=np.float64), np.asarray(models_err[rows], dtype=np.float64)
            if not (np.isfinite(cx) & np.isfinite(ce) & (ce > 0.)).all():
                device = False           # cleaning such a row would reach into a node's position mid-run: the host loop does just that
        if not device:
            for step in self._gng_host_steps(ids, pos, err, nbrs, ages, models, models_err, models_mask, rstate, lprob_func, lprob_args,
                                             lprob_kwargs, learn_best, learn_neighbor, max_age, nbatch, new_err_dec, all_err_dec,
                                             max_nodes, T, track_scale, nn0, graph_init):
                yield step
            return

        draws, x, xe, xm = _training_inputs(rstate, models, models_err, models_mask, T)
        # ---- the state arrays (include/frankenz_hip.h) ----
        md = int(_GNG_MAX_DEGREE)
        cap = max(int(max_nodes), nn0)
        if max(len(v) for v in nbrs) > md:
            raise RuntimeError("graph_init: a node has more than %d neighbours (networks._GNG_MAX_DEGREE)" % md)
        slot = {n: k for k, n in enumerate(ids)}
        edge, adj = {}, np.zeros((2, cap, md, 2), dtype=np.int32)
        deg = np.zeros(cap, dtype=np.int32)
        edge_age = []
        for k, (nb, ag) in enumerate(zip(nbrs, ages)):
            deg[k] = len(nb)
            for j, (m, a_) in enumerate(zip(nb, ag)):
                key = (k, slot[m]) if k < slot[m] else (slot[m], k)
                if key not in edge:
                    edge[key] = len(edge_age); edge_age.append(int(a_))
                adj[0, k, j] = (slot[m], edge[key])
        pcap = max(2, min(int(nbatch) * md, 1 << 22))
        ecap = len(edge_age) + T + 2 * nbatches + 8
        nf, ni = _gng_state_sizes(cap, B, md, pcap, ecap)
        fst, ist = np.zeros(nf), np.zeros(ni, dtype=np.int32)
        p0 = np.array([np.asarray(p, dtype=np.float64) for p in pos])
        if p0.shape != (nn0, B):
            raise ValueError("graph_init: every node needs a position of %d values" % B)
        fst[:nn0 * B] = p0.ravel(); fst[cap * B:cap * B + nn0 * B] = p0.ravel()
        fst[2 * cap * B:2 * cap * B + nn0] = err
        if alias[0] >= 0:
            fst[2 * cap * B + cap:] = p0[:2].ravel()
        ist[:8] = [nn0, 0, len(edge_age), 0, 0, 0 if alias[0] >= 0 else -1, 1 if alias[0] >= 0 else -1, 0]
        o_adj = _GNG_NCNT + 2 * cap
        o_age = o_adj + 4 * cap * md + 3 * pcap
        ist[_GNG_NCNT:_GNG_NCNT + cap] = deg
        ist[o_adj:o_adj + 4 * cap * md] = adj.ravel()
        ist[o_age:o_age + len(edge_age)] = edge_age
        idv = np.zeros(cap, dtype=np.int64); idv[:nn0] = ids
        bmus, batch = np.zeros(max(T, 1), dtype=np.int64), np.zeros((max(nbatches, 1), 2), dtype=np.int32)
        eng = self._eng()
        dx, dxe, dxm, ddraws, dfst, dist, dids, dbmus, dbatch = _device_arrays(eng.device, (x, xe, xm, draws, fst, ist, idv, bmus, batch))
        host = lambda a_: a_ if isinstance(a_, np.ndarray) else a_.cpu().numpy()
        seg = max(1, int(_GNG_SEGMENT))
        for s0 in range(0, T, seg):
            s1 = min(T, s0 + seg)
            eng.gng_train(dx, dxe, dxm, ddraws, dfst, dist, dids, cap, md, pcap, ecap, nbatch, max_age, max_nodes, nn0, learn_best,
                          learn_neighbor, 1. - new_err_dec, 1. - all_err_dec, opts, track_scale, alias[0], alias[1], s0, s1, dbmus,
                          dbatch)
            bm, bt = host(dbmus[s0:s1]), host(dbatch)
            f, i_, idh = host(dfst), host(dist), host(dids)
            NN, cur = int(i_[0]), int(i_[7])
            dg = i_[_GNG_NCNT:_GNG_NCNT + NN]
            ad = i_[o_adj:o_adj + 4 * cap * md].reshape(2, cap, md, 2)[cur, :NN]
            keep = np.arange(md)[None, :] < dg[:, None]
            off = np.zeros(NN + 1, dtype=np.int64); np.cumsum(dg, out=off[1:])
            gpos = f[:cap * B].reshape(cap, B)[:NN].copy()
            fit = f[cap * B:2 * cap * B].reshape(cap, B)[:NN].copy() if track_scale else gpos.copy()
            plist = [p for p in gpos]
            if alias[0] >= 0:
                # the two rows the initial nodes were views of: what the nodes hold now (or held when they were removed)
                rows_now = f[2 * cap * B + cap:].reshape(2, B)
                for k in range(2):
                    models[alias[k]] = rows_now[k]
                    if i_[5 + k] >= 0 and isinstance(models, np.ndarray):
                        plist[int(i_[5 + k])] = models[alias[k]]
            self._gng_finish([int(v) for v in idh[:NN]], plist, gpos, f[2 * cap * B:2 * cap * B + NN].copy(), off, ad[..., 0][keep],
                             i_[o_age:][ad[..., 1][keep]], fit, graph_init)
            for i in range(s0, s1):
                yield None, int(bm[i - s0]), int(bt[i // nbatch, 0]), int(bt[i // nbatch, 1])

    def _gng_finish(self, ids, pos_list, pos, err, off, nbr, age, fit, graph_init):
        """the trained network into the attributes (class docstring); ``graph_init`` is refilled in place, as the reference trains it"""
        self.graph_ids, self.graph_pos, self.graph_errors = np.array(ids), pos, np.asarray(err, dtype=np.float64)
        self.graph_adj_off, self.graph_adj_nbr = np.asarray(off, dtype=np.int64), np.asarray(nbr, dtype=np.int64)
        self.graph_adj_age = np.asarray(age, dtype=np.int64)
        self.nodes, self.NNODE = fit, len(ids)
        graph = graph_init if graph_init is not None else _new_graph()
        if graph is not None:
            _gng_fill_graph(graph, ids, pos_list, [float(e) for e in err], self.graph_adj_off, self.graph_adj_nbr, self.graph_adj_age)
        self.graph = graph

    def _gng_host_steps(self, ids, pos, err, nbrs, ages, models, models_err, models_mask, rstate, lprob_func, lprob_args, lprob_kwargs,
                        learn_best, learn_neighbor, max_age, nbatch, new_err_dec, all_err_dec, max_nodes, T, track_scale, nn0,
                        graph_init):
        """The reference's loop (networks.py:2158-2260) with the user's likelihood, on ordered dictionaries in place of the networkx
        graph: ``nodes[label] = [pos, error]`` in node order, ``adj[label][neighbour] = [age]`` in neighbour order (the age cell is
        shared by the two directions of an edge).  Positions are updated in place, so the two initial nodes keep rewriting the
        caller's rows they are views of."""
        import heapq
        nodes = {n: [p, e] for n, p, e in zip(ids, pos, err)}
        adj = {n: {} for n in ids}
        for n, nb, ag in zip(ids, nbrs, ages):
            for m, a_ in zip(nb, ag):
                adj[n][m] = adj[m][n] if n in adj[m] else [a_]
        order = list(nodes)
        count = {n: k for k, n in enumerate(order)}
        y = np.array([nodes[n][0] for n in order])
        self.nodes = y
        prune, nprune = [], 0
        Nmodel = len(models)
        for i in range(T):
            idx = rstate.choice(Nmodel)
            x, xe, xm = models[idx], models_err[idx], models_mask[idx]
            res = lprob_func(x, xe, xm, y, np.zeros_like(y), np.ones_like(y, dtype='bool'), *lprob_args, **lprob_kwargs)
            lnp, chi2 = res[2], res[4]
            if track_scale:
                y *= res[5][:, None]                                      # the fit copy is rescaled, the graph positions are not
            yb, yb2 = heapq.nlargest(2, range(len(lnp)), key=lnp.__getitem__)
            bmu, bmu2 = order[yb], order[yb2]
            resid = x - nodes[bmu][0]
            y[yb] += learn_best * resid
            nodes[bmu][0] += learn_best * resid
            nodes[bmu][1] += chi2[yb]
            if bmu2 in adj[bmu]:
                adj[bmu][bmu2][0] = 0
            else:
                adj[bmu][bmu2] = adj[bmu2][bmu] = [0]
            for n in list(adj[bmu]):
                resid = x - nodes[n][0]
                y[count[n]] += learn_neighbor * resid
                nodes[n][0] += learn_neighbor * resid
                cell = adj[bmu][n]
                cell[0] += 1
                if cell[0] == max_age:
                    prune.append((bmu, n))
            if i % nbatch == 0:
                nprune = len(prune)
                for e1, e2 in prune:
                    if e1 in adj and e2 in adj[e1]:
                        del adj[e1][e2], adj[e2][e1]
                        for e in (e1, e2):
                            if not adj[e]:
                                del adj[e], nodes[e]
                prune = []
                if len(nodes) < max_nodes:
                    keys = list(nodes)
                    e1 = keys[int(np.argmax([nodes[n][1] for n in keys]))]
                    e1_nbrs = list(adj[e1])
                    e2 = e1_nbrs[int(np.argmax([nodes[n][1] for n in e1_nbrs]))]
                    nodes[e1][1] *= (1. - new_err_dec)
                    nodes[e2][1] *= (1. - new_err_dec)
                    new = nn0 + int(i / nbatch)
                    nodes[new] = [0.5 * (nodes[e1][0] + nodes[e2][0]), nodes[e1][1]]
                    del adj[e1][e2], adj[e2][e1]
                    adj[new] = {}
                    adj[new][e1] = adj[e1][new] = [0]
                    adj[new][e2] = adj[e2][new] = [0]
                order = list(nodes)
                count = {n: k for k, n in enumerate(order)}
                y = np.array([nodes[n][0] for n in order])
                self.nodes, self.NNODE = y, len(order)
            for n in nodes:
                nodes[n][1] *= (1. - all_err_dec)
            if i == T - 1:
                self._gng_publish(nodes, adj, y, graph_init)
            yield res, bmu, len(order), nprune

    def _gng_publish(self, nodes, adj, y, graph_init):
        order = list(nodes)
        count = {n: k for k, n in enumerate(order)}
        off = np.zeros(len(order) + 1, dtype=np.int64)
        np.cumsum([len(adj[n]) for n in order], out=off[1:])
        nbr = [count[m] for n in order for m in adj[n]]
        age = [adj[n][m][0] for n in order for m in adj[n]]
        plist = [nodes[n][0] for n in order]
        self._gng_finish(order, plist, np.array(plist, dtype=np.float64), [nodes[n][1] for n in order], off, nbr, age, y, graph_init)


def _new_graph():
    """an empty networkx.Graph, or None without networkx"""
    try:
        import networkx as nx
    except ImportError:
        return None
    return nx.Graph()
