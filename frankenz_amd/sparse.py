"""
``SparseFits`` -- what ``BruteForce.fit_sparse`` and ``pdf.sparsify_logwt`` return: per object the exact ``Nkeep`` models of largest
ln-posterior of an exhaustive fit, in the layout ``NearestNeighbors.fit`` leaves (``neighbors`` / ``Nneighbors`` beside padded
``fit_*`` rows), so that every consumer of sparse rows runs on a brute-force fit.  An extension with no reference counterpart;
docs/sparse_fits.md states the law.
"""
import sys

import numpy as np

from .engine import get_engine, kde_opts, merge_kde_args, pinned_empty
from .rows import RowConsumers

__all__ = ["SparseFits", "WMAX", "LMAX"]

WMAX = 4096          # FZ_SPARSE_WMAX: most entries kept per object
LMAX = 1 << 20       # FZ_DRAW_LMAX: longest row


def check_keep(Nkeep, wt_thresh, Nmodel=None):
    """-> ``(W, lncut)`` of a ``fit_sparse`` / ``sparsify_logwt`` call; the refusals of the C side, raised before any device call"""
    if isinstance(Nkeep, bool) or int(Nkeep) != Nkeep or Nkeep < 1:
        raise ValueError("`Nkeep` must be a whole number >= 1 (got %r)" % (Nkeep,))
    if wt_thresh is None:
        wt_thresh = 0.
    wt_thresh = float(wt_thresh)
    if not (0. <= wt_thresh < 1.):
        raise ValueError("`wt_thresh` must lie in [0, 1) (got %r)" % (wt_thresh,))
    if Nkeep > WMAX:
        raise NotImplementedError("Nkeep = %d exceeds FZ_SPARSE_WMAX = %d" % (Nkeep, WMAX))
    if Nmodel is not None and Nmodel > LMAX:
        raise NotImplementedError("rows of %d entries exceed FZ_DRAW_LMAX = %d" % (Nmodel, LMAX))
    return int(Nkeep), (np.log(wt_thresh) if wt_thresh > 0. else -np.inf)


class SparseFits(RowConsumers):
    """Sparse rows of an exhaustive fit.  ``neighbors`` (Ndata, Nkeep) int64 model indices, best first, padded with -99 (after
    ``Network.fit_sparse``: in ascending model order; no consumer of the rows looks at their order);
    ``Nneighbors`` (Ndata); the ``fit_*`` arrays (Ndata, Nkeep) padded as ``NearestNeighbors`` pads them (one that was not asked for
    is None); ``lmap`` / ``levid`` of the FULL rows; ``lnkept`` the logsumexp of the kept ln-posteriors; ``NMODEL``."""

    def __init__(self, neighbors, Nneighbors, NMODEL, lmap, levid, lnkept, fit_lnprior=None, fit_lnlike=None, fit_lnprob=None,
                 fit_Ndim=None, fit_chi2=None, fit_scale=None, fit_scale_err=None, device=None):
        self.neighbors, self.Nneighbors, self.NMODEL = neighbors, Nneighbors, int(NMODEL)
        self.lmap, self.levid, self.lnkept = lmap, levid, lnkept
        self.fit_lnprior, self.fit_lnlike, self.fit_lnprob = fit_lnprior, fit_lnlike, fit_lnprob
        self.fit_Ndim, self.fit_chi2, self.fit_scale, self.fit_scale_err = fit_Ndim, fit_chi2, fit_scale, fit_scale_err
        self.NDATA, self.NKEEP = (int(v) for v in neighbors.shape)
        self._device = device
        self.philox_key = None      # key of the last sample() call with draws='device'

    def cover(self):
        """the share of each object's posterior the sparse row holds: ``exp(lnkept - levid)`` (nan without a posterior)"""
        with np.errstate(invalid='ignore'):
            return np.exp(self.lnkept - self.levid)

    def _rows(self, logwt):
        if logwt is None:
            logwt = self.fit_lnprob
        if logwt is None:
            raise ValueError("Fits have not been computed and weights have not been provided.")
        lw = logwt if hasattr(logwt, "data_ptr") else np.ascontiguousarray(logwt, dtype=np.float64)
        if tuple(lw.shape) != (self.NDATA, self.NKEEP):
            raise ValueError("`logwt` has shape %s; expected (Ndata, Nkeep) = (%d, %d) like `neighbors`"
                             % (tuple(lw.shape), self.NDATA, self.NKEEP))
        return lw

    def predict(self, model_labels, model_label_errs, label_dict=None, label_grid=None, logwt=None, kde_args=None, kde_kwargs=None,
                return_gof=False, verbose=True):
        """PDFs from the sparse rows, as ``NearestNeighbors.predict`` forms them from its own (``Engine.knn_predict_logwt``)."""
        kde_kwargs = merge_kde_args(kde_args, kde_kwargs, label_dict is not None)
        if label_dict is None and label_grid is None:
            raise ValueError("`label_dict` or `label_grid` must be specified.")
        lw = self._rows(logwt)
        if len(model_labels) != self.NMODEL:
            raise ValueError("%d labels for %d models" % (len(model_labels), self.NMODEL))
        eng = get_engine(self._device)
        Nx = eng.set_labels(model_labels, model_label_errs, label_dict, label_grid, kde_kwargs)
        ko = kde_opts(kde_kwargs)
        Ndata = self.NDATA
        pdfs = pinned_empty((Ndata, Nx))
        lmap, levid = np.zeros(Ndata), np.zeros(Ndata)
        eng.knn_predict_logwt(lw, self.neighbors, self.Nneighbors, self.NKEEP, ko, pdfs, lmap, levid, n=Ndata)
        if verbose:
            sys.stderr.write('\rGenerating PDF {0}/{0}\n'.format(Ndata))
            sys.stderr.flush()
        return (pdfs, (lmap, levid)) if return_gof else pdfs

    # sample, weight_sampler, weight_em, moments, predict_bins, predict_cdf, predict_quantiles: rows.RowConsumers, over the sparse rows
    def _row_source(self, logwt, shaped=False, use_scale=False):
        if use_scale and self.fit_scale is None:
            raise ValueError("the scale rows were not kept (`track_scale=True`)")
        return self._rows(logwt), self.neighbors, self.Nneighbors

    def _lnlike_rows(self):
        if self.fit_lnlike is None:
            raise ValueError("the ln-likelihood rows were not kept")
        return self.fit_lnlike, self.neighbors, self.Nneighbors, self.NMODEL

    def _check_labels(self, model_labels):
        if len(model_labels) != self.NMODEL:
            raise ValueError("%d labels for %d models" % (len(model_labels), self.NMODEL))

    def predict_phot(self, models, models_err, models_mask, logwt=None):
        """Extension (docs/predictive.md): posterior-predictive photometry ``(phot_mean, phot_var, share)``, each ``(Ndata, Nfilt)``:
        mean and variance of ``scale * model flux`` per band under the rows, the model errors added as the law of total variance,
        masked model bands left out per band (``share``: the weight that was not).  The fitted scales are used when they are kept."""
        if len(models) != self.NMODEL:
            raise ValueError("%d models for fits over %d" % (len(models), self.NMODEL))
        return self._predict_phot(models, models_err, models_mask, logwt)
