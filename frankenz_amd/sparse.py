"""
``SparseFits`` -- what ``BruteForce.fit_sparse`` and ``pdf.sparsify_logwt`` return: per object the exact ``Nkeep`` models of largest
ln-posterior of an exhaustive fit, in the layout ``NearestNeighbors.fit`` leaves (``neighbors`` / ``Nneighbors`` beside padded
``fit_*`` rows), so that every consumer of sparse rows runs on a brute-force fit.  An extension with no reference counterpart;
docs/sparse_fits.md states the law.
"""
import sys

import numpy as np

from .engine import get_engine, kde_opts, merge_kde_args, pinned_empty

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


class SparseFits(object):
    """Sparse rows of an exhaustive fit.  ``neighbors`` (Ndata, Nkeep) int64 model indices, best first, padded with -99;
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

    def sample(self, Nsamples, logwt=None, rstate=None, draws='device', return_gof=False):
        """``Nsamples`` posterior draws (model indices) per object from the sparse rows (``Engine.draw_logwt`` with ``neighbors`` /
        ``nnbr``); ``draws`` / ``rstate`` as in ``BruteForce.sample``.  ``lmap`` / ``levid`` returned are those of the sparse rows."""
        from .bruteforce import _check_nsamples, _draw_outputs, _draw_uniforms
        S = _check_nsamples(Nsamples)
        lw = self._rows(logwt)
        u, key = _draw_uniforms(rstate, draws, self.NDATA, S)
        self.philox_key = key
        eng = get_engine(self._device)
        idx, lmap, levid = _draw_outputs(eng, None, self.NDATA, S, like=lw)
        if self.NDATA:
            eng.draw_logwt(lw, S, idx, u=u, key=key, neighbors=self.neighbors, nnbr=self.Nneighbors, lmap=lmap, levid=levid, n=self.NDATA,
                           W=self.NKEEP)
        return (idx, (lmap, levid)) if return_gof else idx

    def weight_sampler(self):
        """a ``samplers.model_weight_sampler`` over the sparse ``fit_lnlike`` rows (device-resident arrays are used in place)"""
        from .samplers import model_weight_sampler
        if self.fit_lnlike is None:
            raise ValueError("the ln-likelihood rows were not kept")
        return model_weight_sampler(self.fit_lnlike, neighbors=self.neighbors, Nneighbors=self.Nneighbors, Nmodels=self.NMODEL,
                                    device=self._device)

    def weight_em(self):
        """Extension: a ``samplers.model_weight_em`` over the same rows as ``weight_sampler()``: the maximum-likelihood / MAP weights of
        the training set and the marginal ln-likelihood of a weight vector (docs/model_weights.md)."""
        from .samplers import model_weight_em
        if self.fit_lnlike is None:
            raise ValueError("the ln-likelihood rows were not kept")
        return model_weight_em(self.fit_lnlike, neighbors=self.neighbors, Nneighbors=self.Nneighbors, Nmodels=self.NMODEL,
                               device=self._device)

    def moments(self, values, value_errs=None, value_mask=None, logwt=None, use_scale=False):
        """Extension (docs/predictive.md): posterior mean and variance of any per-model quantity -- ``moments(z_train, z_err)`` is a
        posterior mean redshift without a grid -- from the sparse rows (``pdf.posterior_moments``).  ``use_scale`` multiplies each
        entry's values by its fitted ``fit_scale``."""
        from .pdf import posterior_moments
        if use_scale and self.fit_scale is None:
            raise ValueError("the scale rows were not kept (`track_scale=True`)")
        return posterior_moments(self._rows(logwt), values, value_errs, value_mask, scale=self.fit_scale if use_scale else None,
                                 neighbors=self.neighbors, Nneighbors=self.Nneighbors, device=self._device)

    def predict_bins(self, model_labels, model_label_errs, label_bins, logwt=None, wt_thresh=1e-3, normalize=True, return_outside=False,
                     out=None):
        """Extension (docs/bins.md): probability per bin of ``label_bins`` (the edges) from the sparse rows, each model a Gaussian
        ``N(model_labels, model_label_errs)`` integrated exactly between the edges (``pdf.posterior_bins``): the ``(Ndata, Nbins)``
        stack ``samplers.population_sampler`` and ``hierarchical_sampler`` take, without a grid."""
        from .pdf import posterior_bins
        if len(model_labels) != self.NMODEL:
            raise ValueError("%d labels for %d models" % (len(model_labels), self.NMODEL))
        return posterior_bins(self._rows(logwt), model_labels, model_label_errs, label_bins, neighbors=self.neighbors,
                              Nneighbors=self.Nneighbors, wt_thresh=wt_thresh, normalize=normalize, return_outside=return_outside, out=out,
                              device=self._device)

    def predict_cdf(self, model_labels, model_label_errs, points, logwt=None, wt_thresh=1e-3):
        """Extension (docs/bins.md): the mixture CDF of the same kernel at ``points`` (``pdf.posterior_cdf``); one point per object,
        ``(Ndata,)``, is the PIT of a validation sample."""
        from .pdf import posterior_cdf
        if len(model_labels) != self.NMODEL:
            raise ValueError("%d labels for %d models" % (len(model_labels), self.NMODEL))
        return posterior_cdf(self._rows(logwt), model_labels, model_label_errs, points, neighbors=self.neighbors,
                             Nneighbors=self.Nneighbors, wt_thresh=wt_thresh, device=self._device)

    def predict_phot(self, models, models_err, models_mask, logwt=None):
        """Extension (docs/predictive.md): posterior-predictive photometry ``(phot_mean, phot_var, share)``, each ``(Ndata, Nfilt)``:
        mean and variance of ``scale * model flux`` per band under the rows, the model errors added as the law of total variance,
        masked model bands left out per band (``share``: the weight that was not).  The fitted scales are used when they are kept."""
        from .pdf import posterior_moments
        if len(models) != self.NMODEL:
            raise ValueError("%d models for fits over %d" % (len(models), self.NMODEL))
        return posterior_moments(self._rows(logwt), models, models_err, models_mask, scale=self.fit_scale, neighbors=self.neighbors,
                                 Nneighbors=self.Nneighbors, return_share=True, device=self._device)
