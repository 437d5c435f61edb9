"""
``frankenz.samplers`` on the GPU (reference frankenz/samplers.py): the population log-likelihood ``loglike_nz``, the
redshift-assignment step ``nz_assign``, the stacked n(z) ``stack_nz``, and the two MCMC drivers ``population_sampler``
(Metropolis-Hastings-in-Gibbs over random pairs of bins) and ``hierarchical_sampler`` (Gibbs with a Dirichlet hyper-prior) with
the reference's interface.  The PDF stack is uploaded once per sampler and stays on the device; nothing of the size of the
catalogue crosses the bus inside a chain.  docs/samplers.md.
"""
import sys

import numpy as np

from .engine import get_engine

__all__ = ["loglike_nz", "nz_assign", "stack_nz", "population_sampler", "hierarchical_sampler"]

_NZ_SEGMENT = 8            # saved samples of the population chain per library call (the state stays on the device in between)


def loglike_nz(nz, pdfs, overlap=None, return_overlap=False, pair=None, pair_step=None, device=None):
    """ln-likelihood of a population n(z) given individual PDFs (samplers.py:23-86):
    ``sum(log(pdfs @ nz + pair_step * (pdfs[:, i] - pdfs[:, j])))``; ``-inf`` (and zero
    overlaps) when ``nz`` has a negative or non-finite entry.  ``pdfs`` may be a device
    tensor; a precomputed ``overlap`` is used as is, like the reference."""
    nz = np.ascontiguousarray(nz, dtype=np.float64)
    n = len(pdfs)
    if np.any(~np.isfinite(nz) | (nz < 0.)):
        lnlike, out = -np.inf, np.zeros(n)
        return (lnlike, out) if return_overlap else lnlike
    if overlap is not None:
        perturb = 0.
        if pair is not None and pair_step is not None:
            i, j = pair
            perturb = pair_step * (np.asarray(pdfs)[:, i] - np.asarray(pdfs)[:, j])
        out = overlap + perturb
        lnlike = np.sum(np.log(out))
        return (lnlike, out) if return_overlap else lnlike
    if isinstance(pdfs, np.ndarray):
        pdfs = np.ascontiguousarray(pdfs, dtype=np.float64)
    out = np.empty(n)
    use_pair = pair is not None and pair_step is not None
    lnlike = get_engine(device).overlap_nz(pdfs, nz, pair if use_pair else None, pair_step if use_pair else 0.0, out, n=n)
    return (lnlike, out) if return_overlap else lnlike


def nz_assign(nz, pdfs, u=None, rstate=None, return_bins=False, device=None):
    """One categorical draw per object from ``pdfs[i] * nz / dot(pdfs[i], nz)`` and the number of objects per
    bin -- ``np.sum([rstate.multinomial(1, p * pos / np.dot(p, pos)) for p in pdfs], axis=0)`` of
    samplers.py:498-499 / 519-520, the N x G inner step of every Gibbs sweep.  The draw is the inverse CDF of
    one uniform per object (``u``, or ``rstate.rand(N)``): the same distribution as the reference's
    ``multinomial(1, ...)``, which consumes its random stream differently (one binomial per bin), so the
    realisation for a given seed differs.  ``pdfs`` may be a device tensor.  Returns ``counts`` (G, int64)
    [and ``bins`` (N, int64; -1 for a row without mass)]."""
    nz = np.ascontiguousarray(nz, dtype=np.float64)
    n = len(pdfs)
    if u is None:
        u = (np.random if rstate is None else rstate).rand(n)
    u = np.ascontiguousarray(u, dtype=np.float64)
    if u.shape != (n,) or np.any(~(u >= 0.) | ~(u < 1.)):
        raise ValueError("`u` must hold one uniform in [0, 1) per object")
    if isinstance(pdfs, np.ndarray):
        pdfs = np.ascontiguousarray(pdfs, dtype=np.float64)
        if pdfs.shape != (n, len(nz)):
            raise ValueError("`pdfs` must have shape (Nobj, len(nz))")
    counts = np.zeros(len(nz), dtype=np.int64)
    bins = np.empty(n, dtype=np.int64)
    get_engine(device).nz_assign(pdfs, nz, u, bins, counts, n=n)
    return (counts, bins) if return_bins else counts


# ---- the resident stack -----------------------------------------------------------------------------------------------
def _resident_stack(pdfs, eng):
    """``pdfs`` as a float64 (N, G) array on the engine's GPU: a NumPy stack is uploaded (once per sampler), a device tensor is
    used as it is"""
    if isinstance(pdfs, np.ndarray):
        if pdfs.ndim != 2:
            raise ValueError("`pdfs` must have shape (Nobj, Nbins)")
        return eng.device_array(np.ascontiguousarray(pdfs, dtype=np.float64))
    if not hasattr(pdfs, "data_ptr") or len(pdfs.shape) != 2:
        raise TypeError("`pdfs` must be a NumPy array or a 2-d float64 tensor on the GPU")
    if hasattr(pdfs, "element_size") and pdfs.element_size() != 8:
        raise TypeError("a device `pdfs` must be float64")
    return pdfs


def stack_nz(pdfs, device=None):
    """The stacked n(z): ``pdfs.sum(axis=0) / pdfs.sum()``, the samplers' default starting position, summed on the GPU in a fixed
    order.  ``pdfs`` may be a device tensor."""
    eng = get_engine(device)
    n, G = pdfs.shape
    if isinstance(pdfs, np.ndarray):
        pdfs = np.ascontiguousarray(pdfs, dtype=np.float64)
    col = np.empty(G)
    eng.pdfs_colsum(pdfs, G, col, n=n)
    return col / np.sum(col)


def _check_start(pos, G):
    pos = np.array(pos, dtype=np.float64)
    if pos.shape != (G,):
        raise ValueError("`pos_init` must have one entry per bin")
    if np.any(~np.isfinite(pos) | (pos < 0.)):
        raise ValueError("`pos_init` has a negative or non-finite entry (the reference's chain would stay at lnpost = -inf)")
    return pos


# ---- random streams -----------------------------------------------------------------------------------------------------
def _predraw_population(rstate, Ndim, Niter, thin, mh_steps):
    """The reference's random stream of ``Niter`` saved samples, drawn ahead with its own calls in its own order: per sample
    ``thin`` pairs ``rstate.choice(Ndim, size=2, replace=False)``, then per pair and proposal one ``rstate.randn()`` followed by
    one ``rstate.exponential()``.  The number of draws does not depend on the data.  Returns ``pairs (Niter * thin, 2) int64``,
    ``normals`` and ``expo`` ``(Niter * thin, mh_steps)``."""
    pairs = np.empty((Niter * thin, 2), dtype=np.int64)
    normals = np.empty((Niter * thin, mh_steps))
    expo = np.empty((Niter * thin, mh_steps))
    for i in range(Niter):
        for t in range(thin):
            pairs[i * thin + t] = rstate.choice(Ndim, size=2, replace=False)
        for t in range(thin):
            for k in range(mh_steps):
                normals[i * thin + t, k] = rstate.randn()
                expo[i * thin + t, k] = rstate.exponential()
    return pairs, normals, expo


def _philox4x32(key, counter):
    """Philox4x32-10 (Salmon et al., SC'11): ``key`` two 32-bit words, ``counter`` an (n, 4) array of 32-bit words; returns the
    (n, 4) output words.  The NumPy twin of csrc/fz_philox.h."""
    c = [np.array(counter[:, k], dtype=np.uint64) & np.uint64(0xFFFFFFFF) for k in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


def _philox_uniform(key, sweep, n):
    """The uniforms in [0, 1) the device draws for objects ``0 .. n-1`` in sweep ``sweep`` under ``key`` (``draws='device'`` of
    ``hierarchical_sampler``): Philox4x32-10 at the counter (object lo, object hi, sweep lo, sweep hi), the double made of the first
    two output words as NumPy makes one: ``((a >> 5) * 2**26 + (b >> 6)) / 2**53``."""
    idx = np.arange(n, dtype=np.uint64)
    sw = np.uint64(sweep)
    ctr = np.stack([idx & np.uint64(0xFFFFFFFF), idx >> np.uint64(32), np.full(n, sw & np.uint64(0xFFFFFFFF)), np.full(n, sw >> np.uint64(32))],
                   axis=1)
    out = _philox4x32(key, ctr)
    a, b = out[:, 0] >> np.uint32(5), out[:, 1] >> np.uint32(6)
    return (a * 67108864.0 + b) / 9007199254740992.0


class population_sampler(object):
    """
    Sampler for drawing redshift population distributions given a set of individual redshift PDFs (reference
    samplers.py:83-308), with the chain on the GPU.  ``pdfs`` is a NumPy array or a float64 tensor on the engine's GPU.

    With the default flat prior a whole segment of saved samples runs on the device without a host synchronisation; the random
    stream is the reference's (drawn ahead on the host), so that a chain follows the reference's for the same ``rstate`` to the
    rounding of its sums.  With a user ``logprior_nz`` the host takes every decision and the device evaluates the sums.
    After ``sample`` / ``run_mcmc``, ``chain_accept`` (pairs, mh_steps) and ``chain_gscale`` (pairs) hold the accept flag of every
    proposal and the proposal scale of every pair of the last call.
    """

    def __init__(self, pdfs, device=None):
        self.pdfs = pdfs
        self.device = device
        self.samples = []
        self.samples_lnp = []
        self.chain_accept = np.zeros((0, 0), dtype=np.int32)
        self.chain_gscale = np.zeros(0)
        self._dev = None

    def reset(self):
        """Re-initialize the sampler."""
        self.samples = []
        self.samples_lnp = []

    @property
    def results(self):
        """Return samples."""
        return np.array(self.samples), np.array(self.samples_lnp)

    def _stack(self, eng):
        if self._dev is None or self._dev[0] is not self.pdfs:
            self._dev = (self.pdfs, _resident_stack(self.pdfs, eng))
        return self._dev[1]

    def run_mcmc(self, Niter, logprior_nz=None, pos_init=None, thin=400, mh_steps=3, rstate=None, verbose=True,
                 prior_args=[], prior_kwargs={}):
        """Sample the distribution using MH-in-Gibbs MCMC: ``Niter`` saved samples, ``thin`` random pairs of bins per sample,
        ``mh_steps`` proposals per pair; they are appended to ``samples`` / ``samples_lnp``.  As in the reference, ``pos_init``
        is handed on to ``sample`` as given: a second ``run_mcmc`` without ``pos_init`` restarts from the stacked PDFs, not from
        the last sample.  ``verbose`` writes the reference's progress line to stderr."""
        for i, (x, lnp) in enumerate(self.sample(Niter, logprior_nz=logprior_nz, pos_init=pos_init, thin=thin, mh_steps=mh_steps,
                                                 rstate=rstate, prior_args=prior_args, prior_kwargs=prior_kwargs)):
            self.samples.append(np.array(x))
            self.samples_lnp.append(lnp)
            if verbose:
                sys.stderr.write('\r Sample {:d}/{:d} [lnpost = {:6.3f}]      '.format(i + 1, Niter, lnp))
                sys.stderr.flush()

    def sample(self, Niter, logprior_nz=None, pos_init=None, thin=400, mh_steps=3, rstate=None, prior_args=[], prior_kwargs={}):
        """Generator over the saved samples ``(pos, lnpost)``.  ``pos_init=None`` starts from the stacked PDFs (``stack_nz``); a
        ``pos_init`` with a negative or non-finite entry raises ``ValueError``."""
        eng = get_engine(self.device)
        dp = self._stack(eng)
        Nobs, Ndim = dp.shape
        if Ndim < 2:
            raise ValueError("the population sampler moves mass between pairs of bins: it needs at least two")
        if rstate is None:
            rstate = np.random
        Niter, thin, mh_steps = int(Niter), int(thin), int(mh_steps)
        if thin < 1 or mh_steps < 1:
            raise ValueError("`thin` and `mh_steps` must be at least 1")
        pos = stack_nz(dp, eng.device) if pos_init is None else _check_start(pos_init, Ndim)
        overlap, dcol = eng.device_empty(Nobs), eng.device_array(np.zeros(Nobs))
        lnlike = eng.overlap_nz(dp, pos, None, 0., overlap, n=Nobs)
        self.chain_accept = np.zeros((0, mh_steps), dtype=np.int32)
        self.chain_gscale = np.zeros(0)
        self._overlap = overlap                                   # the chain's overlap integrals, on the device
        if logprior_nz is not None:
            for out in self._sample_host_prior(eng, dp, Nobs, Ndim, pos, lnlike, overlap, dcol, Niter, logprior_nz, thin, mh_steps,
                                               rstate, prior_args, prior_kwargs):
                yield out
            return
        lnpost = np.array([lnlike + 0.])
        seg = max(1, int(_NZ_SEGMENT))
        for s0 in range(0, Niter, seg):
            ns = min(seg, Niter - s0)
            pairs, normals, expo = _predraw_population(rstate, Ndim, ns, thin, mh_steps)
            samples, slnp = np.empty((ns, Ndim)), np.empty(ns)
            accept, gscale = np.zeros((ns * thin, mh_steps), dtype=np.int32), np.empty(ns * thin)
            eng.nz_pairs(dp, Nobs, Ndim, pos, overlap, dcol, lnpost, pairs, normals, expo, ns, thin, mh_steps, 0, ns, samples, slnp,
                         accept, gscale)
            self.chain_accept = np.concatenate([self.chain_accept, accept])
            self.chain_gscale = np.concatenate([self.chain_gscale, gscale])
            for k in range(ns):
                yield samples[k], slnp[k]

    def _sample_host_prior(self, eng, dp, Nobs, Ndim, pos, lnlike, overlap, dcol, Niter, logprior_nz, thin, mh_steps, rstate,
                           prior_args, prior_kwargs):
        """The reference's loop (samplers.py:257-308) with the user's ln-prior called with exactly its arguments; every sum over
        the objects is one library call on the resident stack (fz_nz_pair_eval), and an accepted step travels back with the next
        call.  No column of the stack is touched on the host."""
        lnpost = lnlike + logprior_nz(pos, *prior_args, **prior_kwargs)
        pend = None                                             # the accepted step not yet applied to the device's overlap
        accepts, gscales = [], []
        for i in range(Niter):
            pairs = [rstate.choice(Ndim, size=2, replace=False) for _ in range(thin)]
            for pair in pairs:
                t = np.zeros_like(pos)
                t[pair] = (1, -1)
                scale = 1e-4 * np.min(np.append(pos[pair], 1. - pos[pair]))
                sums = eng.nz_pair_eval(dp, Nobs, Ndim, overlap, dcol, 0, pair, pend, scale / 2.)
                pend = None
                lnp1 = sums[0] + logprior_nz(pos + t * scale / 2., *prior_args, **prior_kwargs)
                lnp2 = sums[1] + logprior_nz(pos - t * scale / 2., *prior_args, **prior_kwargs)
                grad = (lnp1 - lnp2) / scale
                if grad != 0.:
                    gscale = min(abs(1. / grad), abs(scale * 1e4))
                else:
                    gscale = abs(scale)
                gscales.append(gscale)
                acc = []
                for k in range(mh_steps):
                    z = rstate.randn() * gscale
                    pos_new = pos + (t * z)
                    if np.any(~np.isfinite(pos_new) | (pos_new < 0.)):
                        lnlike_new = -np.inf
                    else:
                        lnlike_new = eng.nz_pair_eval(dp, Nobs, Ndim, overlap, dcol, 1, None, pend, z)[0]
                        pend = None
                    lnpost_new = lnlike_new + logprior_nz(pos_new, *prior_args, **prior_kwargs)
                    ok = bool(-rstate.exponential() < lnpost_new - lnpost)
                    if ok:
                        pos, lnpost, pend = pos_new, lnpost_new, z
                    acc.append(int(ok))
                accepts.append(acc)
            if pend is not None:                                  # a saved sample leaves the overlap up to date
                eng.nz_pair_eval(dp, Nobs, Ndim, overlap, dcol, 2, None, pend, 0.)
                pend = None
            self.chain_accept = np.array(accepts, dtype=np.int32).reshape(-1, mh_steps)
            self.chain_gscale = np.array(gscales)
            yield pos, lnpost


class hierarchical_sampler(object):
    """
    Sampler for jointly drawing redshift population distributions and individual redshift predictions given a set of individual
    redshift PDFs, which must be *likelihoods* (reference samplers.py:311-535); assumes a Dirichlet hyper-prior.  The N x G step
    of every sweep -- one categorical draw per object from ``pdfs[i] * pos`` -- runs on the GPU over the resident stack; the
    G-sized steps (Dirichlet, reference sample, ln-posterior) are the reference's own calls on the host.

    ``draws='device'`` (default): the objects' uniforms are made inside the kernel by Philox4x32-10, under a key of two 32-bit
    words drawn from ``rstate`` once per ``sample`` call, at the counter (object, sweep); ``_philox_uniform(key, sweep, n)``
    reproduces them.  ``draws='host'``: ``rstate.rand(N)`` per sweep, drawn before the Dirichlet.  In both modes the law is the
    reference's and the realisation for a given seed is not (its ``multinomial(1, ...)`` per object consumes the stream
    differently).  ``sweep_counts`` holds the counts of every sweep of the last ``sample`` call and ``philox_key`` its key.
    """

    def __init__(self, pdfs, device=None):
        self.pdfs = pdfs
        self.device = device
        self.samples = []
        self.samples_lnp = []
        self.sweep_counts = []
        self.philox_key = None
        self._dev = None

    def reset(self):
        """Re-initialize the sampler (unlike the reference's, this also clears ``samples``)."""
        self.samples = []
        self.samples_lnp = []
        self.samples_prior = []
        self.samples_counts = []

    @property
    def results(self):
        """Return samples."""
        return np.array(self.samples), np.array(self.samples_lnp)

    _stack = population_sampler._stack

    def run_mcmc(self, Niter, alpha=None, pos_init=None, thin=5, ref_sample=None, beta=None, rstate=None, verbose=True,
                 draws='device'):
        """Sample the joint distribution using Gibbs MCMC: ``Niter`` saved samples of ``thin`` sweeps each, appended to
        ``samples`` / ``samples_lnp``.  As in the reference, ``pos_init`` is handed on to ``sample`` as given: a second call
        without it restarts from the stacked PDFs."""
        for i, (x, lnp) in enumerate(self.sample(Niter, alpha=alpha, beta=beta, pos_init=pos_init, thin=thin, ref_sample=ref_sample,
                                                 rstate=rstate, draws=draws)):
            self.samples.append(np.array(x))
            self.samples_lnp.append(lnp)
            if verbose:
                sys.stderr.write('\r Sample {:d}/{:d} [lnpost = {:6.3f}]      '.format(i + 1, Niter, lnp))
                sys.stderr.flush()

    def sample(self, Niter, alpha=None, pos_init=None, thin=5, ref_sample=None, beta=None, rstate=None, draws='device'):
        """Generator over the saved samples ``(pos, lnpost)``."""
        from scipy import stats
        if draws not in ('device', 'host'):
            raise ValueError("`draws` must be 'device' or 'host'")
        eng = get_engine(self.device)
        dp = self._stack(eng)
        Nobs, Ndim = dp.shape
        if rstate is None:
            rstate = np.random
        if alpha is None:
            alpha = np.ones(Ndim)
        if beta is None:
            beta = np.ones(Ndim)
        if ref_sample is not None:
            ref_counts = np.array(ref_sample)
            ref_norm = ref_sample + beta
            ref_norm = ref_norm / ref_norm.sum()
            Nref = sum(ref_counts)
        else:
            ref_counts = np.zeros(Ndim)
            Nref = 0
        pos = stack_nz(dp, eng.device) if pos_init is None else _check_start(pos_init, Ndim)
        key = None
        if draws == 'device':
            key = rstate.randint(0, 2**32, size=2, dtype=np.uint32)
        self.philox_key = key
        self.sweep_counts = []
        counts = np.zeros(Ndim, dtype=np.int64)
        lnpriorref = 0.
        sweep = 0

        def one_sweep(pos, ref_counts, lnpriorref, sweep):
            # redshifts (the device), population, reference set, posterior: the reference's order of rstate calls
            if key is None:
                eng.nz_sweep(dp, Nobs, pos, counts, u=np.ascontiguousarray(rstate.rand(Nobs)))
            else:
                eng.nz_sweep(dp, Nobs, pos, counts, key=key, sweep=sweep)
            cnt = counts.copy()
            self.sweep_counts.append(cnt)
            pos = rstate.dirichlet(alpha + cnt + ref_counts)
            if ref_sample is not None:
                pcounts = ref_sample + beta + Nobs * pos
                ref_counts = rstate.multinomial(Nref, pcounts / pcounts.sum())
                lnpriorref = stats.multinomial.logpmf(ref_counts, Nref, ref_norm)
            # (an object without mass under pos is left out of the counts: the trials are the objects counted)
            lnlike = stats.multinomial.logpmf(cnt, int(cnt.sum()), pos)
            lnprior = stats.dirichlet.logpdf(pos, alpha + ref_counts)
            return pos, ref_counts, lnpriorref, lnlike + lnprior + lnpriorref

        pos, ref_counts, lnpriorref, lnpost = one_sweep(np.ascontiguousarray(pos, dtype=np.float64), ref_counts, lnpriorref, sweep)
        for i in range(int(Niter)):
            for j in range(int(thin)):
                sweep += 1
                pos, ref_counts, lnpriorref, lnpost = one_sweep(pos, ref_counts, lnpriorref, sweep)
            yield pos, lnpost
