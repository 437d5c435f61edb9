"""
Zero-point calibration of a catalogue against a model set (extension, no reference counterpart; docs/predictive.md): per-band
multiplicative offsets found by iterating fit -> posterior-predictive photometry -> offset.  The fits, the predicted fluxes
(``predict_phot``) and the per-band sums (``phot_sums``) run on the GPU; only ``(Nfilt,)`` vectors are handled here.
"""
import sys

import numpy as np

from .engine import get_engine
from .pdf import _rows_arg

__all__ = ["PhotSums", "ZeropointResult", "phot_sums", "zeropoint_offsets"]


class PhotSums(object):
    """Per-band sums of a catalogue against its predicted photometry: ``A = sum w x p``, ``B = sum w p^2``, ``C = sum w (x - p)^2``
    with ``w = 1 / (xe^2 + var)``, ``n`` the object-bands counted, ``nclip`` those left out by the clip, and ``factor = A / B`` the
    weighted least-squares factor of the predictions onto the data (nan for a band without an object)."""

    def __init__(self, A, B, C, n, nclip):
        self.A, self.B, self.C, self.n, self.nclip = A, B, C, n, nclip
        with np.errstate(divide='ignore', invalid='ignore'):
            self.factor = A / B


class ZeropointResult(object):
    """``offsets`` (Nfilt,), ``trace`` (iterations, Nfilt) the offsets after each iteration, ``sums`` the ``PhotSums`` of the last
    iteration, ``converged``."""

    def __init__(self, offsets, trace, sums, converged):
        self.offsets, self.trace, self.sums, self.converged = offsets, trace, sums, converged


def phot_sums(data, data_err, data_mask, phot_mean, phot_var, clip=None, device=None):
    """The sums of ``PhotSums`` over the objects with ``data_mask != 0`` and finite data, error, predicted mean and variance, in a
    fixed summation order (``fz_phot_sums``).  ``clip``: an object-band with ``w (x - p)^2 > clip^2`` is left out and counted in
    ``nclip``.  Every array is ``(Ndata, Nfilt)``, NumPy or a device array."""
    arrs = [_rows_arg(a, np.float64, n) for a, n in ((data, "data"), (data_err, "data_err"), (data_mask, "data_mask"),
                                                     (phot_mean, "phot_mean"), (phot_var, "phot_var"))]
    shape = tuple(arrs[0].shape)
    if len(shape) != 2 or any(tuple(a.shape) != shape for a in arrs):
        raise ValueError("data, errors, mask and predictions must share one (Ndata, Nfilt) shape")
    if clip is not None and not clip > 0.:
        raise ValueError("`clip` must be positive or None")
    sums, counts = get_engine(device).phot_sums(arrs[0], arrs[1], arrs[2], arrs[3], arrs[4], shape[0], shape[1],
                                                0. if clip is None else float(clip))
    return PhotSums(sums[0], sums[1], sums[2], counts[0], counts[1])


def zeropoint_offsets(fitter, data, data_err, data_mask, Niter=10, tol=1e-4, ref_band=None, clip=None, Nkeep=256, wt_thresh=1e-3,
                      lprob_kwargs=None, fit_kwargs=None, rstate=None, verbose=True):
    """Per-band zero-point offsets ``a`` of a catalogue relative to the model set of ``fitter`` (a ``BruteForce`` or a
    ``NearestNeighbors``).

    Sign convention: the catalogue is ``a_b`` times the models' system in band ``b``; corrected fluxes are ``data / a`` (and
    ``data_err / a``).

    From ``a = 1``, each iteration fits COPIES ``data / a``, ``data_err / a`` (the caller's arrays are never written) --
    ``fit_sparse(track_scale=True)`` with ``Nkeep`` / ``wt_thresh`` for a ``BruteForce``, ``fit(track_scale=True)`` for a
    ``NearestNeighbors`` --, forms the posterior-predictive photometry (``predict_phot``) and its ``phot_sums`` against the
    corrected catalogue, and multiplies ``a`` by ``f = A / B`` (divided by ``f[ref_band]`` when a reference band is given, which
    then stays at 1).  A band without a counted object keeps its offset.  It stops when ``max |f - 1| < tol``.  With
    ``free_scale`` the overall scale is degenerate with the offsets, so ``ref_band`` is required.  Returns a ``ZeropointResult``."""
    from .bruteforce import BruteForce
    lprob_kwargs = dict(lprob_kwargs or {})
    fit_kwargs = dict(fit_kwargs or {})
    if lprob_kwargs.get("free_scale", False) and ref_band is None:
        raise ValueError("with `free_scale` the overall scale is degenerate with the offsets: give `ref_band`")
    x0, xe0 = np.array(data, dtype=np.float64), np.array(data_err, dtype=np.float64)
    xm0 = np.array(data_mask, dtype=np.float64)
    if x0.ndim != 2 or xe0.shape != x0.shape or xm0.shape != x0.shape:
        raise ValueError("data, errors and mask must share one (Ndata, Nfilt) shape")
    B = x0.shape[1]
    if ref_band is not None and not 0 <= int(ref_band) < B:
        raise ValueError("`ref_band` outside [0, %d)" % B)
    sparse = isinstance(fitter, BruteForce)
    a = np.ones(B)
    trace, sums, converged = [], None, False
    for it in range(int(Niter)):
        xs, xes = x0 / a, xe0 / a
        if sparse:
            fits = fitter.fit_sparse(xs.copy(), xes.copy(), xm0.copy(), Nkeep=min(int(Nkeep), fitter.NMODEL), wt_thresh=wt_thresh,
                                     lprob_kwargs=lprob_kwargs, track_scale=True, verbose=False, **fit_kwargs)
            pm, pv, _ = fits.predict_phot(fitter.models, fitter.models_err, fitter.models_mask)
        else:
            fitter.fit(xs.copy(), xes.copy(), xm0.copy(), rstate=rstate, lprob_kwargs=lprob_kwargs, track_scale=True, verbose=False,
                       **fit_kwargs)
            pm, pv, _ = fitter.predict_phot()
        sums = phot_sums(xs, xes, xm0, pm, pv, clip=clip, device=getattr(fitter, "_device", None))
        f = np.where(sums.n > 0, sums.factor, 1.)
        if ref_band is not None:
            f = np.where(sums.n > 0, f / f[int(ref_band)], 1.)
        a = a * f
        trace.append(a.copy())
        if verbose:
            sys.stderr.write('\rZero-point iteration {0}: max |f - 1| = {1:.3e}'.format(it + 1, np.max(np.abs(f - 1.))))
            sys.stderr.flush()
        if np.max(np.abs(f - 1.)) < tol:
            converged = True
            break
    if verbose:
        sys.stderr.write('\n')
        sys.stderr.flush()
    return ZeropointResult(a, np.array(trace).reshape(-1, B), sums, converged)
