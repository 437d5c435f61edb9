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
the selection, the unions and the PDFs still run on the device.
"""
import sys

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
    if wt_thresh is None and cdf_thresh is None:
        wt_thresh = -np.inf
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    Nnodes, Nmodels = len(nodes), len(models)
    eng = get_engine(device)
    eng.upload_models(nodes, np.zeros_like(nodes), np.ones_like(nodes))     # networks.py:305-307
    obj = HostObjects(models, models_err, models_mask)
    opts = like_opts(lpnet_kwargs)
    free = bool(opts.free_scale)
    lnprob = np.empty((Nmodels, Nnodes))
    scale = np.ones((Nmodels, Nnodes)); scale_err = np.zeros((Nmodels, Nnodes))
    want_scale = track_scale and free
    eng.fit(obj.x, obj.xe, obj.xm, opts, lnprob, None, None, scale if want_scale else None,
            scale_err if want_scale else None)
    obj.writeback()
    if track_scale and not free:
        raise ValueError("track_scale=True needs a likelihood that returns the scale (free_scale=True)")
    return _lists_from_plane(lnprob, scale, scale_err, wt_thresh, cdf_thresh, track_scale, eng)


def _select(eng, lnprob, wt_thresh, cdf_thresh, match=None, csr_off=None, want_stats=False):
    """fz_net_select on a host plane: (nsel, sel[, rawlen][, lmap, levid])"""
    n, nn = lnprob.shape
    nsel = np.zeros(n, dtype=np.int32); sel = np.zeros((n, nn), dtype=np.int32)
    rawlen = np.zeros(n, dtype=np.int64) if csr_off is not None else None
    lmap = np.zeros(n) if want_stats else None; levid = np.zeros(n) if want_stats else None
    use_wt = wt_thresh is not None
    eng.net_select(lnprob, use_wt, wt_thresh if use_wt else 0.0, 0.5 if use_wt or cdf_thresh is None else cdf_thresh, match, csr_off,
                   nsel, sel, rawlen, lmap, levid)
    return nsel, sel, rawlen, lmap, levid


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
    lens = np.array([len(v) for v in lists], dtype=np.int64)
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    items = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists]) if off[-1] else np.zeros(1, dtype=np.int64)
    return off, np.ascontiguousarray(items)


def _is_default(func):
    return func is None or func is _pdf.logprob


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
        if lpnet_func is None:
            lpnet_func = _pdf.logprob
        if lpnet_args is None:
            lpnet_args = []
        if lpnet_kwargs is None:
            lpnet_kwargs = {'free_scale': True, 'ignore_model_err': True, 'return_scale': True}
        if wt_thresh is None and cdf_thresh is None:
            wt_thresh = -np.inf
        self.lpnet_func, self.lpnet_args, self.lpnet_kwargs = lpnet_func, lpnet_args, lpnet_kwargs
        if _is_default(lpnet_func) and not lpnet_args:
            m = populate_network(self.nodes, self.models, self.models_err, self.models_mask, lpnet_kwargs=lpnet_kwargs, wt_thresh=wt_thresh,
                                 cdf_thresh=cdf_thresh, track_scale=track_scale, device=self._device)
        else:
            # the user's node likelihood: called per model as networks.py:310-312 does; selection and lists as above
            y, ye, ym = self.nodes, np.zeros_like(self.nodes), np.ones_like(self.nodes, dtype='bool')
            lnprob = np.empty((self.NMODEL, self.NNODE)); sc = np.ones_like(lnprob); se = np.zeros_like(lnprob)
            for i, (x, xe, xm) in enumerate(zip(self.models, self.models_err, self.models_mask)):
                r = lpnet_func(x, xe, xm, y, ye, ym, *lpnet_args, **lpnet_kwargs)
                lnprob[i] = r[2]
                if track_scale:
                    sc[i], se[i] = r[5], r[6]
            m = _lists_from_plane(lnprob, sc, se, wt_thresh, cdf_thresh, track_scale, self._eng())
        self.nodes_idxs, self.nodes_logwts, self.nodes_bmus = m.nodes_idxs, m.nodes_logwts, m.nodes_bmus
        self.nodes_scales, self.nodes_scales_err, self.nodes_Nmatch = m.nodes_scales, m.nodes_scales_err, m.nodes_Nmatch
        self.models_lmap, self.models_levid = m.models_lmap, m.models_levid
        for r in m.results:
            yield r

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
        nbr = np.zeros((self.NNODE, W), dtype=np.int64); lwt = np.full((self.NNODE, W), -np.inf)
        for i, v in enumerate(lists):
            nbr[i, :len(v)] = v
            lwt[i, :len(v)] = 0.0 if discrete else self.nodes_logwts[i]
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
        lprob_args = lprob_args or []
        lprob_kwargs = lprob_kwargs or {}
        if wt_thresh is None and cdf_thresh is None:
            wt_thresh = -np.inf
        eng = self._eng()
        Ndata = len(data)
        match_sel = np.arange(self.NNODE)[self.nodes_Nmatch > 0]
        match32 = np.ascontiguousarray(match_sel, dtype=np.int32)
        y = np.ascontiguousarray(self.nodes[match_sel]); Nn = len(y)
        self.nodes_only = nodes_only
        if save_fits:
            self.NDATA = Ndata
            self.Nneighbors = np.zeros(Ndata, dtype='int'); self.neighbors = []
            self.fit_lnprior, self.fit_lnlike, self.fit_lnprob, self.fit_Ndim, self.fit_chi2 = [], [], [], [], []
            self.fit_scale, self.fit_scale_err = [], []
        node_pdfs = None
        ko = G = None
        if predict is not None:
            labels, label_errs, label_dict, label_grid, kde_args, kde_kwargs = predict
            if nodes_only:
                node_pdfs = np.ascontiguousarray(self.get_pdfs(labels, label_errs, label_dict, label_grid, kde_args, kde_kwargs,
                                                               False, discrete, False))
                G = node_pdfs.shape[1]
        off, items = _csr(self.nodes_bmus if discrete else self.nodes_idxs)
        lp_default = _is_default(self.lpnet_func) and not self.lpnet_args
        host_lprob = not (_is_default(lprob_func) and not lprob_args)
        out = []
        for i0 in range(0, Ndata, _NET_CHUNK):
            sl = slice(i0, min(i0 + _NET_CHUNK, Ndata)); n = sl.stop - sl.start
            obj = HostObjects(data[sl], data_err[sl], data_mask[sl])
            # node likelihoods (networks.py:880-882): the matched nodes as noiseless, unmasked models
            lnp = np.empty((n, Nn)); chi2 = np.empty((n, Nn)); ndim = np.empty((n, Nn), dtype=np.int64)
            sc = np.ones((n, Nn)); se = np.zeros((n, Nn))
            if lp_default:
                eng.upload_models(y, np.zeros_like(y), np.ones_like(y))
                nopts = like_opts(self.lpnet_kwargs)
                free = bool(nopts.free_scale)
                eng.fit(obj.x, obj.xe, obj.xm, nopts, lnp, chi2, ndim, sc if free else None, se if free else None)
                obj.writeback()
                nres = [np.zeros((n, Nn)), lnp, lnp, ndim, chi2, sc, se]
            else:
                ye, ym = np.zeros_like(y), np.ones_like(y, dtype='bool')
                rows = [self.lpnet_func(x, xe, xm, y, ye, ym, *self.lpnet_args, **self.lpnet_kwargs)
                        for x, xe, xm in zip(data[sl], data_err[sl], data_mask[sl])]
                nres = [np.ascontiguousarray(np.array([r[k] for r in rows])) for k in range(len(rows[0]))]
                lnp = np.ascontiguousarray(nres[2], dtype=np.float64)
            nsel, sel, rawlen, _, _ = _select(eng, lnp, wt_thresh, cdf_thresh, match32, None if nodes_only else off)
            if not nsel.all():
                # (the reference fails here too, in np.max of nothing; a padded table would quietly fit model 0: docs/deviations.md)
                k = int(np.argmin(nsel != 0))
                raise ValueError("object %d selects no node of the network (%d of %d objects in this call do): its node ln-probabilities "
                                 "hold a nan, or none passes the threshold (wt_thresh=%r, cdf_thresh=%r)"
                                 % (i0 + k, int((nsel == 0).sum()), n, wt_thresh, cdf_thresh))
            if nodes_only:
                W = max(int(nsel.max()), 1)
                res = []
                for k, pl in enumerate(nres):
                    pl = np.ascontiguousarray(pl)
                    if pl.dtype not in (np.float64, np.int64):
                        pl = pl.astype(np.float64)
                    g = np.empty((n, W), dtype=pl.dtype)
                    eng.net_gather(pl, nsel, sel, W, 0, g)
                    res.append(g)
                nb = np.empty((n, W), dtype=np.int64)
                eng.net_gather(np.ascontiguousarray(np.broadcast_to(match_sel.astype(np.int64), (n, Nn))), nsel, sel, W, -99, nb)
                nn_ = nsel.astype(np.int64)
                pdfs = lmap = levid = None
                if predict is not None:
                    pdfs = np.empty((n, G)); lmap = np.empty(n); levid = np.empty(n)
                    eng.net_stack(lnp, nsel, sel, match32, node_pdfs, pdfs, lmap, levid)
            else:
                W = max(int(rawlen.max()), 1)
                if not rawlen.all():
                    # (`discrete`: a matched node need not be any model's best one; the reference fails in np.max of nothing)
                    raise ValueError("object %d: the nodes it selects list no model" % (i0 + int(np.argmin(rawlen != 0))))
                if W > _UNION_MAX:
                    raise NotImplementedError("object %d: its selected nodes list %d models before repeats are removed; the union table "
                                              "of fz_knn_fit_predict holds at most %d (this is not the limit of %d matched nodes)"
                                              % (i0 + int(np.argmax(rawlen)), W, _UNION_MAX, _NODES_MAX))
                idx = np.empty((n, W), dtype=np.int64)
                eng.net_table(nsel, sel, match32, off, items, W, idx)
                nb = np.empty((n, W), dtype=np.int64); nn_ = np.empty(n, dtype=np.int64)
                eng.upload_models(self.models, self.models_err, self.models_mask)
                pdfs = lmap = levid = None
                if predict is not None:
                    ko, G = self._labels(eng, labels, label_errs, label_dict, label_grid, kde_args, kde_kwargs)
                    pdfs = np.empty((n, G)); lmap = np.empty(n); levid = np.empty(n)
                opts = like_opts({} if host_lprob else lprob_kwargs)
                lnl = np.empty((n, W)); c2 = np.empty((n, W)); nd = np.empty((n, W), dtype=np.int64)
                s_ = np.empty((n, W)); se_ = np.empty((n, W))
                eng.knn_fit_predict(obj.x, obj.xe, obj.xm, idx, W, opts, ko, nb, nn_, lnl, c2, nd, s_, se_,
                                    None if host_lprob else pdfs, None if host_lprob else lmap, None if host_lprob else levid)
                obj.writeback()
                if host_lprob:
                    # the user's likelihood on each object's model subset (networks.py:925-928), the PDFs from its ln-posteriors
                    lw = np.full((n, W), -np.inf)
                    rows = []
                    for k in range(n):
                        ii = nb[k, :nn_[k]]
                        r = lprob_func(data[sl][k], data_err[sl][k], data_mask[sl][k], self.models[ii], self.models_err[ii],
                                       self.models_mask[ii], *lprob_args, **lprob_kwargs)
                        rows.append(r); lw[k, :nn_[k]] = r[2]
                    if predict is not None:
                        # (the user's function may have used this device's context itself -- the package's own logprob does: the model and
                        #  label sets are put back before the PDFs are stacked)
                        ko, G = self._labels(eng, labels, label_errs, label_dict, label_grid, kde_args, kde_kwargs)
                        eng.knn_predict_logwt(lw, nb, nn_, W, ko, pdfs, lmap, levid)
                    res = rows
                else:
                    res = [np.zeros((n, W)), lnl, lnl, nd, c2, s_, se_]
            for k in range(n):
                m = int(nn_[k])
                idxs = nb[k, :m].copy()
                if isinstance(res, list) and len(res) and isinstance(res[0], tuple):
                    results = res[k]
                else:
                    results = [r[k, :m].copy() for r in res]
                    # (pdf.logprob returns seven arrays with return_scale, else five: pdf.py:404-411)
                    seven = (len(nres) > 5 and (not lp_default or self.lpnet_kwargs.get('return_scale', False))) if nodes_only \
                        else bool(lprob_kwargs.get('return_scale', False))
                    if not seven:
                        results = results[:5]
                if save_fits:
                    self.Nneighbors[i0 + k] = m
                    self.neighbors.append(np.array(idxs))
                    self.fit_lnprior.append(results[0]); self.fit_lnlike.append(results[1]); self.fit_lnprob.append(results[2])
                    self.fit_Ndim.append(results[3]); self.fit_chi2.append(results[4])
                    if track_scale:
                        self.fit_scale.append(results[5]); self.fit_scale_err.append(results[6])
                if predict is not None:
                    out.append((idxs, m, results, pdfs[k], (lmap[k], levid[k])))
                else:
                    out.append((idxs, m, results))
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
        for r in self._run(data, data_err, data_mask, lprob_func, nodes_only, wt_thresh, cdf_thresh, lprob_args, lprob_kwargs,
                           track_scale, discrete, save_fits):
            yield r

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
        from .sparse import SparseFits
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
        nopts = like_opts(self.lpnet_kwargs)
        if wt_thresh is None and cdf_thresh is None:
            wt_thresh = -np.inf
        use_wt = wt_thresh is not None
        sel_args = (use_wt, wt_thresh if use_wt else 0.0, 0.5 if use_wt or cdf_thresh is None else cdf_thresh)
        eng = self._eng()
        Ndata, M = len(data), self.NMODEL
        match_sel = np.arange(self.NNODE)[self.nodes_Nmatch > 0]
        match32 = np.ascontiguousarray(match_sel, dtype=np.int32)
        y = np.ascontiguousarray(self.nodes[match_sel]); Nn = len(y)
        off, items = _csr(self.nodes_bmus if discrete else self.nodes_idxs)
        d_match, d_off, d_items = eng.device_array(match32), eng.device_array(off), eng.device_array(items)
        # Objects per device call: the (n, Nn) node plane, sel (n, Nn) int32, nsel and the counts inside a quarter of the workspace
        # budget.  The selection of the counting pass stays on the device for the fitting pass while all of it fits another quarter;
        # otherwise the fitting pass forms it again, chunk by chunk.
        limit = eng.workspace_limit()
        sel_row = Nn * 4 + 4
        keep = Ndata * sel_row <= limit // 4
        nc1 = int(max(1, min(_NET_CHUNK, (limit // 4) // (Nn * 8 + (0 if keep else sel_row) + 8))))

        def select(i0, n, d_nsel, d_sel):
            """the node likelihoods of objects [i0, i0 + n) (cleaned in place, written back) and their selection, on the device"""
            obj = HostObjects(data[i0:i0 + n], data_err[i0:i0 + n], data_mask[i0:i0 + n])
            plane = eng.device_empty((n, Nn), np.float64)
            eng.upload_models(y, np.zeros_like(y), np.ones_like(y))
            eng.fit(obj.x, obj.xe, obj.xm, nopts, plane, n=n)
            obj.writeback()
            eng.net_select(plane, *sel_args, None, None, d_nsel, d_sel)
            return obj

        # ---- pass 1: the selections and the sizes of the unions; every refusal falls here, before the first subset fit ----
        nuniq = np.zeros(Ndata, dtype=np.int64)
        if keep and Ndata:
            all_nsel, all_sel = eng.device_empty((Ndata,), np.int32), eng.device_empty((Ndata, Nn), np.int32)
        for i0 in range(0, Ndata, nc1):
            n = min(nc1, Ndata - i0)
            if keep:
                d_nsel, d_sel = all_nsel.data_ptr() + i0 * 4, all_sel.data_ptr() + i0 * Nn * 4
                hold = None
            else:
                hold = (eng.device_empty((n,), np.int32), eng.device_empty((n, Nn), np.int32))
                d_nsel, d_sel = hold[0].data_ptr(), hold[1].data_ptr()
            select(i0, n, d_nsel, d_sel)
            nsel = np.empty(n, dtype=np.int32)
            eng.dev_copy(nsel, d_nsel, nsel.nbytes)
            if not nsel.all():
                k = int(np.argmin(nsel != 0))
                raise ValueError("object %d selects no node of the network (%d of %d objects in this call do): its node ln-probabilities "
                                 "hold a nan, or none passes the threshold (wt_thresh=%r, cdf_thresh=%r)"
                                 % (i0 + k, int((nsel == 0).sum()), n, wt_thresh, cdf_thresh))
            eng.net_union(d_nsel, d_sel, d_match, d_off, d_items, M, nuniq[i0:i0 + n], n=n, nn=Nn)
            if not nuniq[i0:i0 + n].all():
                raise ValueError("object %d: the nodes it selects list no model" % (i0 + int(np.argmin(nuniq[i0:i0 + n] != 0))))
        W = max(int(nuniq.max()), 1) if Ndata else 1
        if W > _UNION_MAX:
            raise NotImplementedError("object %d: its selected nodes list %d different models; the union table of fz_knn_fit_predict "
                                      "holds at most FZ_KNN_WMAX = %d" % (int(np.argmax(nuniq)), W, _UNION_MAX))

        # ---- pass 2: the tables and the subset likelihood, straight into rows [i0, i0 + n) of the (Ndata, W) outputs ----
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

        def rows(a, i0, n, width=W):
            """rows [i0, i0 + n) of an output: a view of a host array, a raw pointer into a device array"""
            if a is None:
                return None
            return a[i0:i0 + n] if isinstance(a, np.ndarray) else a.data_ptr() + i0 * width * 8

        nc2 = int(max(1, min(_NET_CHUNK, (limit // 4) // (W * 8 + (0 if keep else Nn * 8 + sel_row)))))
        for i0 in range(0, Ndata, nc2):
            n = min(nc2, Ndata - i0)
            if keep:
                d_nsel, d_sel = all_nsel.data_ptr() + i0 * 4, all_sel.data_ptr() + i0 * Nn * 4
                obj = HostObjects(data[i0:i0 + n], data_err[i0:i0 + n], data_mask[i0:i0 + n])
            else:
                hold = (eng.device_empty((n,), np.int32), eng.device_empty((n, Nn), np.int32))
                d_nsel, d_sel = hold[0].data_ptr(), hold[1].data_ptr()
                obj = select(i0, n, d_nsel, d_sel)
            idx = eng.device_empty((n, W), np.int64)
            nu = eng.device_empty((n,), np.int64)
            eng.net_union(d_nsel, d_sel, d_match, d_off, d_items, M, nu, W, idx, n=n, nn=Nn)
            eng.upload_models(self.models, self.models_err, self.models_mask)
            eng.knn_fit_predict(obj.x, obj.xe, obj.xm, idx, W, opts, None, rows(nbr, i0, n), rows(cnt, i0, n, 1), rows(lnl, i0, n),
                                rows(chi2, i0, n), rows(ndim, i0, n), rows(sc, i0, n), rows(se, i0, n), n=n)
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
        if verbose:
            sys.stderr.write('\rFitting object {0}/{0}\n'.format(Ndata)); sys.stderr.flush()
        return SparseFits(nbr, cnt, M, lmap, levid, levid.copy(), lpr, lnl, lpb, ndim, chi2, sc, se, device=self._device)

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
        lw = np.full((N, W), -np.inf); nb = np.zeros((N, W), dtype=np.int64)
        for i in range(N):
            lw[i, :lens[i]] = logwt[i]
            nb[i, :lens[i]] = self.neighbors[i] if not self.nodes_only else 0
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
        if wt_thresh is None and cdf_thresh is None:
            wt_thresh = -np.inf                                           # no thresholding at all
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
                                             wt_thresh, cdf_thresh, track_scale):
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
        use_wt = wt_thresh is not None
        dx, dxe, dxm, dnodes, dpos, ddraws, dlr, dsig, dbmus = _device_arrays(eng.device, (x, xe, xm, nodes, pos, draws, lr, sig, bmus))
        seg = max(1, int(_SOM_SEGMENT))
        for s0 in range(0, T, seg):
            s1 = min(T, s0 + seg)
            eng.som_train(dx, dxe, dxm, dnodes, dpos, ddraws, dlr, dsig, kind, use_wt, wt_thresh if use_wt else 0.,
                          0.5 if use_wt else cdf_thresh, opts, track_scale, s0, s1, dbmus)
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
