"""
``frankenz.samplers`` on the GPU (reference frankenz/samplers.py): the population log-likelihood ``loglike_nz``, the
redshift-assignment step ``nz_assign``, the stacked n(z) ``stack_nz``, and the two MCMC drivers ``population_sampler``
(Metropolis-Hastings-in-Gibbs over random pairs of bins) and ``hierarchical_sampler`` (Gibbs with a Dirichlet hyper-prior) with
the reference's interface.  The PDF stack is uploaded once per sampler and stays on the device; nothing of the size of the
catalogue crosses the bus inside a chain.  docs/samplers.md.  ``model_weight_sampler`` (Gibbs) and ``model_weight_em`` (EM: point estimate and
marginal ln-likelihood) are the extension over the weights of the training objects themselves, docs/model_weights.md.
"""
import sys

import numpy as np

from .engine import get_engine

__all__ = ["loglike_nz", "nz_assign", "stack_nz", "population_sampler", "hierarchical_sampler", "model_weight_sampler",
           "model_weight_em"]

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


_MW_KEY_XOR = 0x6D775F67      # second key word of the gamma draws (csrc/fz_mw.h: FZ_MW_KEY_XOR)
_MW_TRIES = 64
_MW_BOOST_SLOT = 128


def _philox_gamma(key, sweep, shape, return_attempts=False):
    """The ``Gamma(shape[j], 1)`` draws the device makes for models ``j = 0 .. len(shape)-1`` in sweep ``sweep`` under ``key``
    (``fz_mw_dirichlet`` / ``fz_mw_chain``; the NumPy twin of csrc/fz_mw.h: mw_gamma).  Marsaglia & Tsang (2000) without the squeeze;
    Philox4x32-10 under the key ``(key[0], key[1] ^ 0x6D775F67)`` -- a domain disjoint from the sweep's uniforms, which use ``key``
    itself -- at the counter ``(j, slot, sweep lo, sweep hi)``: slot ``2 a`` gives attempt ``a`` its normal (Box-Muller of
    ``u1 = 1 - U(words 0, 1)`` and ``u2 = U(words 2, 3)``), slot ``2 a + 1`` its acceptance uniform ``1 - U(words 0, 1)``, slot 128
    the uniform of the shape + 1 boost for ``shape < 1``, applied in log space.  At most 64 attempts (``RuntimeError`` beyond).
    ``return_attempts``: also the number of the attempt that was accepted."""
    shape = np.ascontiguousarray(shape, dtype=np.float64)
    n = len(shape)
    if np.any(~np.isfinite(shape) | (shape <= 0.)):
        raise ValueError("gamma shapes must be finite and positive")
    gkey = (int(key[0]) & 0xFFFFFFFF, (int(key[1]) & 0xFFFFFFFF) ^ _MW_KEY_XOR)
    sw = int(sweep)

    def words(idx, slot):
        ctr = np.stack([idx.astype(np.uint64), np.full(len(idx), slot, dtype=np.uint64), np.full(len(idx), sw & 0xFFFFFFFF, dtype=np.uint64),
                        np.full(len(idx), sw >> 32, dtype=np.uint64)], axis=1)
        return _philox4x32(gkey, ctr)

    def u53(a, b):
        return ((a >> np.uint32(5)) * 67108864.0 + (b >> np.uint32(6))) / 9007199254740992.0

    boost = shape < 1.
    a = np.where(boost, shape + 1., shape)
    d = a - 1. / 3.
    c = 1. / np.sqrt(9. * d)
    g = np.full(n, -1.)
    att = np.full(n, -1, dtype=np.int64)
    todo = np.arange(n)
    for t in range(_MW_TRIES):
        if not len(todo):
            break
        o = words(todo, 2 * t)
        u1, u2 = 1. - u53(o[:, 0], o[:, 1]), u53(o[:, 2], o[:, 3])
        x = np.sqrt(-2. * np.log(u1)) * np.cos(6.283185307179586 * u2)
        v1 = 1. + c[todo] * x
        q = words(todo, 2 * t + 1)
        ua = 1. - u53(q[:, 0], q[:, 1])
        pos = v1 > 0.
        v = np.where(pos, v1 * v1 * v1, 1.)
        dd = d[todo]
        acc = pos & (np.log(ua) < 0.5 * x * x + dd - dd * v + dd * np.log(v))
        g[todo[acc]] = (dd * v)[acc]
        att[todo[acc]] = t
        todo = todo[~acc]
    if len(todo):
        raise RuntimeError("a gamma draw was not accepted within %d attempts" % _MW_TRIES)
    if boost.any():
        jb = np.nonzero(boost)[0]
        o = words(jb, _MW_BOOST_SLOT)
        ub = 1. - u53(o[:, 0], o[:, 1])
        g[jb] = np.exp(np.log(g[jb]) + np.log(ub) / shape[jb])
    return (g, att) if return_attempts else g


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


# ---- Gibbs over the weights of the training objects (docs/model_weights.md) -------------------------------------------------------
def _is_torch(a):
    return hasattr(a, "data_ptr") and hasattr(a, "detach")


def _mw_host(a):
    """a host NumPy copy of an array that may live on the device (a DeviceArray or a tensor)"""
    if isinstance(a, np.ndarray):
        return a
    if _is_torch(a):
        return a.detach().cpu().numpy()
    return a.numpy()


def _mw_lnpost(counts, pos, alpha):
    """multinomial ln-pmf of ``counts`` under ``pos`` (the counted objects are the trials) + Dirichlet ln-pdf of ``pos`` under
    ``alpha``: the values of ``scipy.stats.multinomial.logpmf`` / ``dirichlet.logpdf``, written out so that an exact zero in ``pos``
    gives an infinity and not an exception"""
    from scipy.special import gammaln, xlogy
    cnt = np.asarray(counts, dtype=np.float64)
    lnlike = gammaln(cnt.sum() + 1.) - gammaln(cnt + 1.).sum() + xlogy(cnt, pos).sum()
    lnprior = gammaln(alpha.sum()) - gammaln(alpha).sum() + xlogy(alpha - 1., pos).sum()
    return lnlike + lnprior


def _mw_fixed_sum(a):
    """the sum of ``a`` in the order of ``k_mw_gsum`` (csrc/fz_mw.h): blocks of 256 summed by a halving tree, thread ``t`` of one block
    adds the block sums ``t, t + 256, ...`` in order, then the same tree"""
    def tree(v):                                    # (..., 256) -> (...)
        n = 256
        while n > 1:
            n //= 2
            v = v[..., :n] + v[..., n:2 * n]
        return v[..., 0]
    a = np.asarray(a, dtype=np.float64)
    nblk = (len(a) + 255) // 256
    pad = np.zeros(nblk * 256); pad[:len(a)] = a
    part = tree(pad.reshape(nblk, 256))
    acc = np.zeros(256)
    for k in range(0, nblk, 256):
        acc[:len(part[k:k + 256])] += part[k:k + 256]
    return float(tree(acc))


def _mw_em_lnw(w, M):
    """``ln w - ln sum(w)`` (the fixed-order sum) of a weight vector that is finite, non-negative and has a positive sum"""
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (M,) or not np.isfinite(w).all() or (w < 0.).any() or not w.sum() > 0.:
        raise ValueError("`w` must hold one finite non-negative weight per model, with a positive sum")
    with np.errstate(divide='ignore'):
        return np.log(w) - np.log(_mw_fixed_sum(w))


class _model_weight_rows(object):
    """What ``model_weight_sampler`` and ``model_weight_em`` share: the checks of the rows, their one upload, the marginal
    ln-likelihood of a weight vector and what the weights are for (``logwt``, ``population_pdfs``)."""

    def __init__(self, lnlike, neighbors=None, Nneighbors=None, Nmodels=None, device=None):
        if (neighbors is None) != (Nneighbors is None):
            raise ValueError("`neighbors` and `Nneighbors` come together")
        if len(lnlike.shape) != 2:
            raise ValueError("`lnlike` must have shape (Nobj, Nmodels) or (Nobj, K*k)")
        N, W = (int(v) for v in lnlike.shape)
        if neighbors is None:
            if Nmodels is not None and int(Nmodels) != W:
                raise ValueError("dense rows have one entry per model")
            Nmodels = W
        else:
            if Nmodels is None:
                raise ValueError("`Nmodels` must be given beside `neighbors`")
            if tuple(neighbors.shape) != (N, W) or tuple(Nneighbors.shape) != (N,):
                raise ValueError("`neighbors` must have the shape of `lnlike` and `Nneighbors` one entry per object")
        if N < 1 or W < 1 or int(Nmodels) < 1:
            raise ValueError("the sampler needs at least one object and one model")
        self.lnlike, self.neighbors, self.Nneighbors = lnlike, neighbors, Nneighbors
        self.NOBJ, self.W, self.NMODEL = N, W, int(Nmodels)
        self.device = device
        self._dev = None

    def _resident(self, eng):
        """the rows (and neighbour tables) on the engine's GPU: uploaded once, or the caller's device arrays themselves"""
        if self._dev is not None:
            return self._dev
        # only what is UPLOADED needs room: arrays already on the device are used where they lie
        parts = [a for a in (self.lnlike, self.neighbors, self.Nneighbors) if isinstance(a, np.ndarray)]
        need = sum(int(a.size) * 8 for a in parts)
        if need > eng.workspace_limit():
            raise MemoryError("%s: the rows need %d bytes of device memory, the workspace limit is %d (nothing is "
                              "spilled)" % (type(self).__name__, need, eng.workspace_limit()))

        def put(a, dt):
            if a is None:
                return None
            if isinstance(a, np.ndarray):
                try:
                    return eng.device_array(np.ascontiguousarray(a, dtype=dt))
                except MemoryError:
                    raise MemoryError("%s: the rows need %d bytes of device memory" % (type(self).__name__, need))
            if not hasattr(a, "data_ptr"):
                raise TypeError("rows must be NumPy arrays or arrays on the GPU")
            # a device array is read as raw C-contiguous memory of 8-byte items: anything else is refused
            if hasattr(a, "element_size") and a.element_size() != 8:
                raise TypeError("device rows must be float64 and device neighbour tables int64")
            kind = getattr(a, "dtype", None)
            if kind is not None and not str(kind).endswith(np.dtype(dt).name):
                raise TypeError("a device array of dtype %s where %s is needed" % (kind, np.dtype(dt).name))
            if hasattr(a, "is_contiguous") and not a.is_contiguous():
                raise ValueError("device arrays must be C-contiguous (a strided view would be read as raw memory)")
            return a

        self._dev = (put(self.lnlike, np.float64), put(self.neighbors, np.int64), put(self.Nneighbors, np.int64))
        return self._dev

    def _marginal(self, w):
        """(sum_i ln sum_j L_ij w_j over the objects with a posterior, objects skipped) for one weight vector, normalised with the
        fixed-order sum: one ``fz_mw_loglike`` call on the rows where they are (host rows are staged in chunks, no index is built)"""
        lnw = _mw_em_lnw(self._weights(w), self.NMODEL)
        eng = get_engine(self.device)
        rows, nb, nn = self._dev if self._dev is not None else (self.lnlike, self.neighbors, self.Nneighbors)
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows, dtype=np.float64)
            nb = None if nb is None else np.ascontiguousarray(nb, dtype=np.int64)
            nn = None if nn is None else np.ascontiguousarray(nn, dtype=np.int64)
        return eng.mw_loglike(rows, self.NOBJ, self.W, self.NMODEL, lnw, neighbors=nb, nnbr=nn)

    # ---- what the weights are for -------------------------------------------------------------------------------------------------
    def _weights(self, w):
        if w is None:
            w = self._default_weights(False)
        w = np.asarray(w, dtype=np.float64)
        if w.shape[-1] != self.NMODEL:
            raise ValueError("`w` must have one entry per model")
        return w

    def logwt(self, w=None):
        """``(N, W)`` rows ``lnlike + ln w[neighbors]`` (dense: ``lnlike + ln w``): the objects' ln-posterior rows under the inferred
        population, for the fitter's ``predict(logwt=)`` / ``sample(logwt=)``.  ``w`` defaults to the mean of the samples.  Entries
        past ``Nneighbors[i]`` keep the row's own padding.  NumPy, or torch when the rows are tensors."""
        w = self._weights(w)
        if w.ndim != 1:
            raise ValueError("`w` must be one weight vector")
        with np.errstate(divide='ignore'):
            lnw = np.log(w)
        if _is_torch(self.lnlike):
            import torch
            r = self.lnlike
            t = torch.as_tensor(lnw, dtype=r.dtype, device=r.device)
            if self.neighbors is None:
                return r + t[None, :]
            nb, nn = torch.as_tensor(self.neighbors, device=r.device), torch.as_tensor(self.Nneighbors, device=r.device)
            valid = torch.arange(self.W, device=r.device)[None, :] < nn[:, None]
            return torch.where(valid, r + t[torch.where(valid, nb, torch.zeros_like(nb))], r)
        r = np.asarray(_mw_host(self.lnlike), dtype=np.float64)
        if self.neighbors is None:
            return r + lnw[None, :]
        nb, nn = _mw_host(self.neighbors), np.asarray(_mw_host(self.Nneighbors))
        valid = np.arange(self.W)[None, :] < nn[:, None]
        with np.errstate(invalid='ignore'):
            return np.where(valid, r + lnw[np.where(valid, nb, 0)], r)

    def population_pdfs(self, model_labels, model_label_errs, label_dict=None, label_grid=None, kde_kwargs=None, w=None):
        """The weight samples as population distributions of a label: ``(Niter, G)`` n(label) samples, row ``s`` the KDE of the
        models' labels weighted by ``w[s]`` (the reference's ``gauss_kde_dict`` / ``gauss_kde`` with ``y_wt = w[s]``, normalised
        unless ``kde_kwargs`` says otherwise).  ``w`` defaults to all the samples.  The KDE clips weights below ``wt_thresh`` (1e-3)
        of the largest: pass ``kde_kwargs={'wt_thresh': 0}`` if no weight is to be clipped."""
        from .engine import kde_opts
        if label_dict is None and label_grid is None:
            raise ValueError("`label_dict` or `label_grid` must be specified.")
        w = self._default_weights(True) if w is None else self._weights(w)
        w = np.ascontiguousarray(np.atleast_2d(w), dtype=np.float64)
        if w.shape[1] != self.NMODEL or len(model_labels) != self.NMODEL:
            raise ValueError("`w` and the labels must have one entry per model")
        eng = get_engine(self.device)
        Nx = eng.set_labels(model_labels, model_label_errs, label_dict, label_grid, kde_kwargs)
        pdfs = np.empty((len(w), Nx))
        if len(w):
            eng.predict_logwt(w, kde_opts(kde_kwargs), pdfs, is_log=False, n=len(w))
        return pdfs


class model_weight_sampler(_model_weight_rows):
    """
    Hierarchical re-weighting of a training set: Gibbs sampling of population weights ``w`` over the ``M`` training objects (models)
    under a Dirichlet hyper-prior, given every object's ln-likelihood rows.  The law is the reference's ``hierarchical_sampler``
    (samplers.py:311-535) on dense rows with the models in the place of the label grid: per sweep every object's assignment is
    redrawn, ``j_i ~ exp(lnlike_ij) w_j``, and the weights are redrawn from ``Dirichlet(alpha + counts)``.  The realisation for a
    seed is not the reference's.  ``ref_sample`` and ``beta`` are not taken: a reference sample of counts per training object has no
    use here.  docs/model_weights.md.

    ``lnlike``: ``(N, M)`` dense rows -- only for model sets that fit as ``(N, M)`` --, or ``(N, W)`` rows beside ``neighbors``
    ``(N, W)`` int64, ``Nneighbors`` ``(N)`` and ``Nmodels`` (what ``NearestNeighbors.fit`` leaves; entries past ``Nneighbors[i]`` are
    never read).  NumPy arrays are uploaded once, when the first chain starts; arrays already on the engine's GPU are used in place
    (C-contiguous float64 rows and int64 tables) by every sweep -- the default start and ``logwt()`` alone read them back, see ``sample``.
    Rows that do not fit the workspace limit or the device raise ``MemoryError`` with the bytes needed: nothing is spilled.

    An object without a posterior under the current weights (a nan, a maximum that is not finite -- all of its neighbours at weight
    0 included --, no neighbour) is left out of that sweep's counts.

    ``draws='device'`` (default): every random number is made on the device by Philox4x32-10 under a key of two 32-bit words drawn
    from ``rstate`` once per ``sample`` call (``philox_key``); a saved sample is ONE library call of ``thin`` sweeps, and only the
    weights and the counts come back.  ``_philox_uniform(key, sweep, N)`` and ``_philox_gamma(key, sweep, alpha + counts)`` reproduce
    them.  ``draws='host'``: per sweep ``rstate.rand(N)``, then ``rstate.dirichlet(alpha + counts)`` on the host -- reproducible from
    the seed with NumPy alone.  ``sweep_counts`` holds the counts of every sweep of the last ``sample`` call.
    """

    def __init__(self, lnlike, neighbors=None, Nneighbors=None, Nmodels=None, device=None):
        _model_weight_rows.__init__(self, lnlike, neighbors, Nneighbors, Nmodels, device)
        self.samples = []
        self.samples_lnp = []
        self.sweep_counts = []
        self.philox_key = None

    def reset(self):
        """Re-initialize the sampler."""
        self.samples = []
        self.samples_lnp = []

    @property
    def results(self):
        """Return samples: ``(samples (Niter, M), samples_lnp (Niter))``."""
        return np.array(self.samples), np.array(self.samples_lnp)

    def _stack_start(self):
        """the analogue of ``stack_nz``: ``pos_j`` proportional to ``sum_i exp(r_ij - logsumexp_j' r_ij')``, a scatter-add of the
        normalised rows (once per chain, on the host)"""
        from scipy.special import logsumexp
        M = self.NMODEL
        r = np.asarray(_mw_host(self.lnlike), dtype=np.float64)
        pos = np.zeros(M)
        step = max(1, (1 << 24) // self.W)
        nb = None if self.neighbors is None else _mw_host(self.neighbors)
        nn = None if self.neighbors is None else np.asarray(_mw_host(self.Nneighbors))
        for lo in range(0, self.NOBJ, step):
            rr = r[lo:lo + step]
            if nb is not None:
                valid = np.arange(self.W)[None, :] < nn[lo:lo + step, None]
                rr = np.where(valid, rr, -np.inf)
            with np.errstate(invalid='ignore', divide='ignore'):
                p = np.exp(rr - logsumexp(rr, axis=1, keepdims=True))
            p[~np.isfinite(p).all(axis=1)] = 0.
            if nb is None:
                pos += p.sum(axis=0)
            else:
                np.add.at(pos, np.where(valid, nb[lo:lo + step], 0).ravel(), np.where(valid, p, 0.).ravel())
        if not pos.sum() > 0.:
            raise ValueError("no object has a posterior over the models: give `pos_init`")
        return pos / pos.sum()

    def run_mcmc(self, Niter, alpha=None, pos_init=None, thin=5, rstate=None, verbose=True, draws='device'):
        """Sample the weights using Gibbs MCMC: ``Niter`` saved samples of ``thin`` sweeps each, appended to ``samples`` /
        ``samples_lnp``.  As in ``hierarchical_sampler``, a second call without ``pos_init`` restarts from the stacked rows."""
        for i, (x, lnp) in enumerate(self.sample(Niter, alpha=alpha, pos_init=pos_init, thin=thin, rstate=rstate, draws=draws)):
            self.samples.append(np.array(x))
            self.samples_lnp.append(lnp)
            if verbose:
                sys.stderr.write('\r Sample {:d}/{:d} [lnpost = {:6.3f}]      '.format(i + 1, Niter, lnp))
                sys.stderr.flush()

    def sample(self, Niter, alpha=None, pos_init=None, thin=5, rstate=None, draws='device'):
        """Generator over the saved samples ``(pos, lnpost)``: ``pos`` the weights (M), ``lnpost`` the multinomial ln-pmf of the
        sweep's counts under ``pos`` plus the Dirichlet ln-pdf of ``pos`` under ``alpha``.  One sweep runs ahead of the loop, as in
        the reference's sampler.  ``pos_init=None`` starts from the stacked normalised rows, which are formed ON THE HOST once per
        ``sample`` call: rows (and neighbour tables) that live on the device are copied back for it, all N x W of them (about
        8 GB at 1e6 objects and ``K k`` = 500) -- give ``pos_init`` (a flat ``np.full(M, 1. / M)`` will do) to keep device-resident
        rows where they are.  A start with a negative or non-finite entry, or an ``alpha`` that is not positive and finite,
        raises ``ValueError``."""
        if draws not in ('device', 'host'):
            raise ValueError("`draws` must be 'device' or 'host'")
        N, W, M = self.NOBJ, self.W, self.NMODEL
        Niter, thin = int(Niter), int(thin)
        if thin < 1:
            raise ValueError("`thin` must be at least 1")
        alpha = np.ones(M) if alpha is None else np.ascontiguousarray(alpha, dtype=np.float64)
        if alpha.shape != (M,) or np.any(~np.isfinite(alpha) | (alpha <= 0.)):
            raise ValueError("`alpha` must hold one finite positive entry per model")
        pos = self._stack_start() if pos_init is None else _check_start(pos_init, M)
        if rstate is None:
            rstate = np.random
        eng = get_engine(self.device)
        d_rows, d_nb, d_nn = self._resident(eng)
        with np.errstate(divide='ignore'):
            lnw = np.log(pos)
        self.sweep_counts = []
        counts = np.zeros(M, dtype=np.int64)
        if draws == 'host':
            self.philox_key = None

            def sweep():
                eng.mw_sweep(d_rows, N, W, M, lnw, counts, u=np.ascontiguousarray(rstate.rand(N)), neighbors=d_nb, nnbr=d_nn)
                self.sweep_counts.append(counts.copy())
                p = rstate.dirichlet(alpha + counts)
                with np.errstate(divide='ignore'):
                    return p, np.log(p)

            pos, lnw = sweep()
            for i in range(Niter):
                for j in range(thin):
                    pos, lnw = sweep()
                yield pos, _mw_lnpost(self.sweep_counts[-1], pos, alpha)
            return
        key = rstate.randint(0, 2**32, size=2, dtype=np.uint32)
        self.philox_key = key
        d_alpha, d_lnw = eng.device_array(alpha), eng.device_array(lnw)
        pos = np.empty(M)
        eng.mw_chain(d_rows, N, W, M, d_alpha, d_lnw, key, 0, 1, counts, pos, neighbors=d_nb, nnbr=d_nn)
        self.sweep_counts.append(counts.copy())
        for i in range(Niter):
            call = np.empty((thin, M), dtype=np.int64)
            eng.mw_chain(d_rows, N, W, M, d_alpha, d_lnw, key, 1 + i * thin, thin, counts, pos, neighbors=d_nb, nnbr=d_nn, counts_all=call)
            self.sweep_counts.extend(call)
            yield pos.copy(), _mw_lnpost(counts, pos, alpha)

    def _default_weights(self, many):
        if many:
            return np.array(self.samples)
        if not len(self.samples):
            raise ValueError("no samples yet: run the sampler or give `w`")
        return np.mean(self.samples, axis=0)

    def marginal_lnlike(self, w=None):
        """``(lnlike, nskip)``: the marginal ln-likelihood ``sum_i ln sum_j L_ij w_j`` of one weight vector (default: the mean of the
        samples) over the objects with a posterior under it, and how many have none -- ``model_weight_em.loglike``, one
        ``fz_mw_loglike`` call.  Unlike ``samples_lnp`` it does not depend on a draw."""
        return self._marginal(w)


# ---- EM over the weights of the training objects (docs/model_weights.md, "EM") ------------------------------------------------------
class model_weight_em(_model_weight_rows):
    """
    Maximum-likelihood / MAP population weights ``w`` over the ``M`` training objects by expectation-maximisation, and the marginal
    ln-likelihood ``L(w) = sum_i ln sum_j L_ij w_j`` of any weight vector: the expectation form of ``model_weight_sampler``'s Gibbs
    sweep (the reference's ``hierarchical_sampler``, samplers.py:311-535, with every entry's responsibility added where the sweep
    draws one and counts).  Arguments, checks and the one upload of the rows are ``model_weight_sampler``'s.

    One iteration from ``w``: ``ell_i = logsumexp_k (lnlike_ik + ln w[nbr_ik])``; ``lnpost = sum_i ell_i + sum_j (alpha_j - 1) ln w_j``;
    ``c_j = sum exp(lnlike_ik + ln w_j - ell_i)`` over the entries of model ``j``; ``w'_j`` proportional to ``c_j + (alpha_j - 1)``.
    ``alpha`` must be finite and ``>= 1`` (below 1 there is no maximum).  An object without a posterior under ``w`` (a nan, a maximum
    that is not finite, no neighbour) is skipped and counted.  Every sum has one fixed order: a result is a function of its inputs.

    Sparse rows are read a second time through an inverted index (per model the entries that list it, in object order), built on the
    device at the first ``step`` / ``run`` and kept: 12 bytes per counted entry, which must fit the workspace limit
    (``MemoryError`` names them).  ``loglike`` needs neither the index nor resident rows.
    """

    def __init__(self, lnlike, neighbors=None, Nneighbors=None, Nmodels=None, device=None):
        _model_weight_rows.__init__(self, lnlike, neighbors, Nneighbors, Nmodels, device)
        self.pos = self.lnw = self.counts = None
        self.lnpost_trace = np.zeros(0)
        self.nskip_trace = np.zeros(0, dtype=np.int64)
        self.niter = 0
        self.converged = False
        self._index = None

    def _default_weights(self, many):
        if self.pos is None:
            raise ValueError("no weights yet: run the iteration or give `w`")
        return self.pos

    def _alpha(self, alpha):
        M = self.NMODEL
        alpha = np.ones(M) if alpha is None else np.ascontiguousarray(alpha, dtype=np.float64)
        if alpha.shape != (M,) or np.any(~np.isfinite(alpha) | (alpha < 1.)):
            raise ValueError("`alpha` must hold one finite entry >= 1 per model (below 1 the posterior has no maximum)")
        return alpha

    def loglike(self, w=None):
        """``(lnlike, nskip)``: ``sum_i ln sum_j L_ij w_j`` over the objects with a posterior under ``w`` (default ``pos``), and
        the number of objects without one."""
        return self._marginal(w)

    def _problem(self, eng):
        """the resident rows and, for sparse rows, the inverted index (built once)"""
        d_rows, d_nb, d_nn = self._resident(eng)
        if d_nb is not None and self._index is None:
            N, W, M = self.NOBJ, self.W, self.NMODEL
            E, nbytes = eng.mw_em_index_bytes(N, W, M, d_nn)
            if nbytes > eng.workspace_limit():
                raise MemoryError("model_weight_em: the inverted index needs %d bytes of device memory, the workspace limit is %d "
                                  "(nothing is spilled)" % (nbytes, eng.workspace_limit()))
            from .engine import DeviceArray
            try:
                idx = (DeviceArray(eng, (M + 1,), np.int64), DeviceArray(eng, (max(E, 1),), np.int32),
                       DeviceArray(eng, (max(E, 1),), np.float64))
            except MemoryError:
                raise MemoryError("model_weight_em: the inverted index needs %d bytes of device memory" % nbytes)
            eng.mw_em_index(d_rows, N, W, M, d_nb, d_nn, E, *idx)
            self._index = (E, idx)
        return d_rows, d_nb, d_nn

    def _iterate(self, eng, d_alpha, d_lnw, niter):
        """``niter`` iterations in ONE library call -> (pos, counts, trace (niter), nskip (niter)); ``d_lnw`` moves on"""
        N, W, M = self.NOBJ, self.W, self.NMODEL
        d_rows, d_nb, d_nn = self._problem(eng)
        E, idx = self._index if self._index is not None else (0, None)
        pos, counts = np.empty(M), np.empty(M)
        trace, nskip = np.empty(niter), np.empty(niter, dtype=np.int64)
        eng.mw_em(d_rows, N, W, M, d_alpha, d_lnw, niter, pos, counts, trace, nskip, neighbors=d_nb, nnbr=d_nn, index=idx, entries=E)
        return pos, counts, trace, nskip

    def step(self, w, alpha=None):
        """One iteration from ``w`` -> ``(w_new, lnpost_of_w, counts)``: the ln-posterior is that of ``w`` itself, ``counts`` the
        expected counts ``c`` under it (``counts.sum()`` is the number of objects with a posterior)."""
        alpha = self._alpha(alpha)
        lnw = _mw_em_lnw(w, self.NMODEL)
        eng = get_engine(self.device)
        pos, counts, trace, _ = self._iterate(eng, alpha, eng.device_array(lnw), 1)
        return pos, float(trace[0]), counts

    def run(self, maxiter=500, alpha=None, pos_init=None, tol=1e-6, check_every=10, verbose=True):
        """Iterate from ``pos_init`` (default: uniform weights) until the ln-posterior grows by at most ``tol`` nats in one
        iteration, or ``maxiter`` iterations.  One library call runs ``check_every`` iterations without a host synchronisation;
        the trace is read after each call, so the iteration stops at the end of the call in which the increase first fell to
        ``tol``.  Sets ``pos``, ``lnw``, ``counts`` (of the last iteration), ``lnpost_trace[t]`` (the ln-posterior of the weights
        going into iteration ``t``), ``nskip_trace``, ``niter`` and ``converged``.  Returns ``pos``."""
        maxiter, check_every, M = int(maxiter), int(check_every), self.NMODEL
        if maxiter < 1 or check_every < 1:
            raise ValueError("`maxiter` and `check_every` must be at least 1")
        alpha = self._alpha(alpha)
        lnw0 = np.full(M, -np.log(float(M))) if pos_init is None else _mw_em_lnw(pos_init, M)
        eng = get_engine(self.device)
        d_alpha, d_lnw = eng.device_array(alpha), eng.device_array(lnw0)
        traces, skips, done, last = [], [], 0, None
        self.converged = False
        while done < maxiter and not self.converged:
            n = min(check_every, maxiter - done)
            pos, counts, trace, nskip = self._iterate(eng, d_alpha, d_lnw, n)
            inc = np.diff(np.concatenate(([last] if last is not None else [], trace)))
            self.converged = bool((inc <= tol).any())
            traces.append(trace); skips.append(nskip)
            done += n
            last = trace[-1]
            if verbose:
                sys.stderr.write('\r Iteration {:d}/{:d} [lnpost = {:6.3f}]      '.format(done, maxiter, last))
                sys.stderr.flush()
        self.pos, self.counts, self.lnw = pos, counts, d_lnw.numpy()
        self.lnpost_trace, self.nskip_trace, self.niter = np.concatenate(traces), np.concatenate(skips), done
        return self.pos
