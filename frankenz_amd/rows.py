"""
``RowConsumers`` -- the methods that ``BruteForce``, ``NearestNeighbors`` and ``SparseFits`` share: everything that consumes rows of
ln-weights after a fit (posterior draws, the model-weight samplers, moments, bin masses, CDFs, quantiles, predictive photometry).  The fitters
differ in where the rows come from, in whether they come with ``neighbors`` / ``Nneighbors``, and in what they say when there are
none; each says so in two hooks:

``_row_source(logwt, shaped=False, use_scale=False)`` -> ``(rows, neighbors, Nneighbors)``
    the given ``logwt`` or the stored ln-posterior rows (dense rows: ``None, None`` beside them), refused in the fitter's own words.
    ``shaped``: the rows are about to be drawn from and come back as an array with a ``shape``; ``use_scale``: ``fit_scale`` is
    about to be used.
``_lnlike_rows()`` -> ``(rows, neighbors, Nneighbors, Nmodels)``
    the stored ln-likelihood rows of the weight samplers.

``_check_labels(model_labels)`` may refuse a label table of the wrong length, and ``_draw_rows`` may be replaced.
"""
from .engine import get_engine

__all__ = ["RowConsumers"]


class RowConsumers(object):
    """Mixin of the fitters: the consumers of rows of ln-weights.  Needs ``_device``, ``fit_scale`` and the hooks above."""

    def _check_labels(self, model_labels):
        pass

    def _draw_rows(self, lw, neighbors, Nneighbors, S, u, key):
        """``S`` draws per row of ``lw`` -> ``(idx, lmap, levid)``"""
        from .bruteforce import _draw_outputs
        Ndata, W = (int(v) for v in lw.shape)
        eng = get_engine(self._device)
        idx, lmap, levid = _draw_outputs(eng, None, Ndata, S, like=lw)
        if Ndata:
            eng.draw_logwt(lw, S, idx, u=u, key=key, neighbors=neighbors, nnbr=Nneighbors, lmap=lmap, levid=levid, n=Ndata, W=W)
        return idx, lmap, levid

    def sample(self, Nsamples, logwt=None, rstate=None, draws='device', return_gof=False):
        """Extension, the analogue of ``predict``: ``Nsamples`` posterior draws (model indices) per object from the stored fits
        (``fit_lnprob``, beside ``neighbors`` / ``Nneighbors`` where the fits are sparse) or from the given rows of ln-weights of the
        same layout (NumPy or a device array).  ``fit()`` followed by ``sample()`` gives what ``fit_sample`` gives.  ``lmap`` /
        ``levid`` returned with ``return_gof`` are those of the rows drawn from."""
        from .bruteforce import _check_nsamples, _draw_uniforms
        S = _check_nsamples(Nsamples)
        lw, nb, nn = self._row_source(logwt, shaped=True)
        u, key = _draw_uniforms(rstate, draws, int(lw.shape[0]) if nb is None else self.NDATA, S)
        self.philox_key = key
        idx, lmap, levid = self._draw_rows(lw, nb, nn, S, u, key)
        return (idx, (lmap, levid)) if return_gof else idx

    def weight_sampler(self):
        """Extension: a ``samplers.model_weight_sampler`` over the stored ``fit_lnlike`` rows (beside ``neighbors`` / ``Nneighbors``
        where the fits are sparse; device-resident arrays are used in place), for hierarchical re-weighting of the training set
        (docs/model_weights.md).  Dense rows are for model sets that fit as ``(Ndata, Nmodel)``."""
        from .samplers import model_weight_sampler
        rows, nb, nn, M = self._lnlike_rows()
        return model_weight_sampler(rows, neighbors=nb, Nneighbors=nn, Nmodels=M, device=self._device)

    def weight_em(self):
        """Extension: a ``samplers.model_weight_em`` over the same rows as ``weight_sampler()``: the maximum-likelihood / MAP weights of
        the training set and the marginal ln-likelihood of a weight vector (docs/model_weights.md)."""
        from .samplers import model_weight_em
        rows, nb, nn, M = self._lnlike_rows()
        return model_weight_em(rows, neighbors=nb, Nneighbors=nn, Nmodels=M, device=self._device)

    def moments(self, values, value_errs=None, value_mask=None, logwt=None, use_scale=False):
        """Extension (docs/predictive.md): posterior mean and variance of any per-model quantity -- ``moments(z_train, z_err)`` is a
        posterior mean redshift without a grid -- under the stored fits or the given rows of the same layout
        (``pdf.posterior_moments``).  ``use_scale`` multiplies each entry's values by its fitted ``fit_scale``."""
        from .pdf import posterior_moments
        lw, nb, nn = self._row_source(logwt, use_scale=use_scale)
        return posterior_moments(lw, values, value_errs, value_mask, scale=self.fit_scale if use_scale else None, neighbors=nb,
                                 Nneighbors=nn, device=self._device)

    def predict_bins(self, model_labels, model_label_errs, label_bins, logwt=None, wt_thresh=1e-3, normalize=True, return_outside=False,
                     out=None):
        """Extension (docs/bins.md): probability per bin of ``label_bins`` (the edges) under the stored fits or the given rows of the
        same layout, each model a Gaussian ``N(model_labels, model_label_errs)`` integrated exactly between the edges
        (``pdf.posterior_bins``): the ``(Ndata, Nbins)`` stack ``samplers.population_sampler`` and ``hierarchical_sampler`` take,
        without a grid."""
        from .pdf import posterior_bins
        self._check_labels(model_labels)
        lw, nb, nn = self._row_source(logwt)
        return posterior_bins(lw, model_labels, model_label_errs, label_bins, neighbors=nb, Nneighbors=nn, wt_thresh=wt_thresh,
                              normalize=normalize, return_outside=return_outside, out=out, device=self._device)

    def predict_cdf(self, model_labels, model_label_errs, points, logwt=None, wt_thresh=1e-3):
        """Extension (docs/bins.md): the mixture CDF of the same kernel at ``points`` (``pdf.posterior_cdf``); one point per object,
        ``(Ndata,)``, is the PIT of a validation sample."""
        from .pdf import posterior_cdf
        self._check_labels(model_labels)
        lw, nb, nn = self._row_source(logwt)
        return posterior_cdf(lw, model_labels, model_label_errs, points, neighbors=nb, Nneighbors=nn, wt_thresh=wt_thresh,
                             device=self._device)

    def predict_quantiles(self, model_labels, model_label_errs, q=(0.025, 0.16, 0.5, 0.84, 0.975), logwt=None, wt_thresh=1e-3, out=None):
        """Extension (docs/quantiles.md): the quantiles of that mixture CDF at the probabilities ``q`` (``pdf.posterior_quantiles``):
        by default the median and the 68 % and 95 % credible intervals of the label per object, ``(Ndata, 5)``, without a grid."""
        from .pdf import posterior_quantiles
        self._check_labels(model_labels)
        lw, nb, nn = self._row_source(logwt)
        return posterior_quantiles(lw, model_labels, model_label_errs, q, neighbors=nb, Nneighbors=nn, wt_thresh=wt_thresh, out=out,
                                   device=self._device)

    def predict_scores(self, model_labels, model_label_errs, points, logwt=None, wt_thresh=1e-3, want=('lnpdf', 'crps', 'sqnorm')):
        """Extension (docs/scores.md): the scoring rules of that mixture at ``points`` in closed form (``pdf.posterior_scores``): with
        the true labels of a validation sample, ``(Ndata,)``, the log score ``lnpdf``, the ``crps`` and the squared norm ``sqnorm``
        of the CDE loss per object, as a dict; ``want`` may also name ``spread`` and ``ninc``."""
        from .pdf import posterior_scores
        self._check_labels(model_labels)
        lw, nb, nn = self._row_source(logwt)
        return posterior_scores(lw, model_labels, model_label_errs, points, neighbors=nb, Nneighbors=nn, wt_thresh=wt_thresh, want=want,
                                device=self._device)

    def _predict_phot(self, models, models_err, models_mask, logwt):
        from .pdf import posterior_moments
        lw, nb, nn = self._row_source(logwt)
        return posterior_moments(lw, models, models_err, models_mask, scale=self.fit_scale, neighbors=nb, Nneighbors=nn,
                                 return_share=True, device=self._device)

    def predict_phot(self, logwt=None):
        """Extension (docs/predictive.md): posterior-predictive photometry ``(phot_mean, phot_var, share)``, each ``(Ndata, Nfilt)``:
        mean and variance of ``scale * model flux`` per band under the stored fits, the model errors added as the law of total
        variance, masked model bands left out per band (``share``: the weight that was not)."""
        return self._predict_phot(self.models, self.models_err, self.models_mask, logwt)
