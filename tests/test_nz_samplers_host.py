"""The n(z) samplers, host side (no GPU): the random tables the device chain is handed, a NumPy restatement of the reference's
population chain fed from those tables, the Philox generator's NumPy twin, the interfaces, and the hierarchical restatement, all
against G16 (tests/golden/g16_nz_samplers.npz, made by tests/golden/make_golden_nz.py from the reference).  The helpers here are
shared with the golden generator and with tests/test_hip_nz_samplers.py."""
import inspect
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
import frankenz_oracle as fo  # noqa: E402

G16 = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g16_nz_samplers.npz')

# population cases: stack (seed, N, G, zero_tails), Niter, thin, mh_steps, extras; the RandomState seed of a case is G16's `<tag>_seed`
POP = {
    'a': dict(stack=(1601, 2000, 40, False), Niter=6, thin=30, mh_steps=3),
    'b': dict(stack=(1602, 20000, 120, False), Niter=4, thin=60, mh_steps=3),
    'c': dict(stack=(1603, 2000, 40, False), Niter=5, thin=40, mh_steps=1, pos_init=16031),
    'd': dict(stack=(1604, 200, 40, True), Niter=5, thin=40, mh_steps=3),
    'e': dict(stack=(1605, 2000, 40, False), Niter=4, thin=30, mh_steps=3, prior=16051),
    'f': dict(stack=(1606, 2000, 40, False), Niter=3, thin=30, mh_steps=3, twice=True),
}
# hierarchical cases: stack, hyper-prior seed, with a reference sample or not
HIER = {'h': dict(stack=(1611, 2000, 30, False), hyper=16111, ref=False),
        'r': dict(stack=(1612, 2000, 30, False), hyper=16121, ref=True)}
HIER_NITER, HIER_THIN, HIER_BATCHES = 400, 5, 20


def nz_stack(seed, N, G, zero_tails=False):
    """Gaussian PDFs on the bin grid plus a small floor, row-normalised; zero_tails: no floor and exact zeros beyond 3.5 sigma"""
    rs = np.random.RandomState(seed)
    cen = rs.beta(2., 3., N)[:, None] * (G - 1)
    sig = rs.uniform(0.6, 0.06 * G + 1., N)[:, None]
    x = (np.arange(G)[None, :] - cen) / sig
    p = np.exp(-0.5 * x * x)
    if zero_tails:
        p[np.abs(x) > 3.5] = 0.
    else:
        p += 1e-4
    return p / p.sum(axis=1)[:, None]


def case_stack(g, tag, spec):
    """the case's stack, checked against what G16 recorded of it (its sum of squares and first rows)"""
    p = nz_stack(*spec)
    np.testing.assert_allclose(np.sum(p * p), g[tag + '_stack_ss'], rtol=1e-13)
    np.testing.assert_array_equal(p[:2], g[tag + '_stack_head'])
    return p


def ln_dirichlet(pos, alpha):
    """case e's user prior: ln of a Dirichlet density (nan outside the simplex's interior, which rejects)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.sum((alpha - 1.) * np.log(pos)) + math.lgamma(np.sum(alpha)) - sum(math.lgamma(a) for a in alpha))


def case_extras(tag, G):
    """(pos_init, logprior_nz, prior_args) of a population case"""
    c = POP[tag]
    pos_init = np.random.RandomState(c['pos_init']).dirichlet(np.full(G, 2.)) if 'pos_init' in c else None
    if 'prior' in c:
        return pos_init, ln_dirichlet, [np.random.RandomState(c['prior']).uniform(1., 3., G)]
    return pos_init, None, []


def hier_extras(tag, G):
    """(alpha, ref_sample, beta) of a hierarchical case"""
    c = HIER[tag]
    rs = np.random.RandomState(c['hyper'])
    alpha = rs.uniform(0.5, 2., G)
    if not c['ref']:
        return alpha, None, None
    return alpha, rs.multinomial(300, rs.dirichlet(np.full(G, 3.))).astype(np.float64), rs.uniform(0.5, 1.5, G)


def sum_plain(x):
    return np.sum(x)


def sum_longdouble(x):
    return float(np.sum(x.astype(np.longdouble)))


def sum_reversed_chunks(x, chunk=1000):
    s = 0.
    for k in range((len(x) - 1) // chunk * chunk, -1, -chunk):
        s += float(np.sum(x[k:k + chunk][::-1]))
    return s


def restated_population(pdfs, pos, pairs, normals, expo, thin, logprior=None, prior_args=(), total=sum_plain):
    """The population chain (Metropolis-Hastings-in-Gibbs over pairs of bins) fed from pre-drawn tables.  Returns samples,
    samples_lnp, the accept flag and the margin |lnpost_new - lnpost + exponential| of every proposal, gscale of every pair, and the
    final overlap."""
    prior = (lambda p: 0.) if logprior is None else (lambda p: logprior(p, *prior_args))
    pos = np.array(pos, dtype=np.float64)
    npair, mh = normals.shape
    overlap = np.dot(pdfs, pos)
    with np.errstate(invalid='ignore', divide='ignore'):
        lnpost = total(np.log(overlap)) + prior(pos)
        samples, lnps, acc, margin, gscales = [], [], np.zeros((npair, mh), dtype=np.int32), np.zeros((npair, mh)), np.zeros(npair)
        for p in range(npair):
            i, j = pairs[p]
            d = pdfs[:, i] - pdfs[:, j]
            t = np.zeros_like(pos)
            t[i], t[j] = 1., -1.
            scale = 1e-4 * np.min([pos[i], pos[j], 1. - pos[i], 1. - pos[j]])
            lnp1 = total(np.log(overlap + (scale / 2.) * d)) + prior(pos + t * scale / 2.)
            lnp2 = total(np.log(overlap + (-scale / 2.) * d)) + prior(pos - t * scale / 2.)
            grad = (lnp1 - lnp2) / scale
            gscale = min(abs(1. / grad), abs(scale * 1e4)) if grad != 0. else abs(scale)
            gscales[p] = gscale
            for k in range(mh):
                z = normals[p, k] * gscale
                pos_new = pos + t * z
                if np.any(~np.isfinite(pos_new) | (pos_new < 0.)):
                    lnl_new, ov_new = -np.inf, None
                else:
                    ov_new = overlap + z * d
                    lnl_new = total(np.log(ov_new))
                lnpost_new = lnl_new + prior(pos_new)
                diff = lnpost_new - lnpost
                margin[p, k] = abs(diff + expo[p, k])
                if -expo[p, k] < diff:
                    pos, lnpost, overlap = pos_new, lnpost_new, ov_new
                    acc[p, k] = 1
            if (p + 1) % thin == 0:
                samples.append(pos.copy())
                lnps.append(lnpost)
    return np.array(samples), np.array(lnps), acc, margin, gscales, overlap


def restated_hierarchical(pdfs, Niter, thin, alpha, ref_sample, beta, rstate, uniforms, pos_init=None, clearance=None):
    """The hierarchical Gibbs chain with the oracle's inverse-CDF assignment; ``uniforms(sweep)`` gives a sweep's uniforms (called
    before the sweep's Dirichlet draw).  Returns the saved (pos, lnpost) and the counts of every sweep; ``clearance`` (a list)
    collects every sweep's smallest relative distance of a target to a CDF edge."""
    from scipy import stats
    N, G = pdfs.shape
    beta = np.ones(G) if beta is None else beta
    if ref_sample is not None:
        ref_counts = np.array(ref_sample)
        ref_norm = (ref_sample + beta) / (ref_sample + beta).sum()
        Nref = sum(ref_counts)
    else:
        ref_counts, Nref = np.zeros(G), 0
    pos = pdfs.sum(axis=0) / pdfs.sum() if pos_init is None else pos_init
    out, all_counts, lnpriorref = [], [], 0.
    for sweep in range(Niter * thin + 1):
        u = uniforms(sweep)
        if clearance is not None:
            clearance.append(cdf_edge_clearance(pdfs, pos, u))
        counts = fo.nz_assign(pos, pdfs, u)[0]
        all_counts.append(counts)
        pos = rstate.dirichlet(alpha + counts + ref_counts)
        if ref_sample is not None:
            pc = ref_sample + beta + N * pos
            ref_counts = rstate.multinomial(Nref, pc / pc.sum())
            lnpriorref = stats.multinomial.logpmf(ref_counts, Nref, ref_norm)
        lnpost = stats.multinomial.logpmf(counts, int(counts.sum()), pos) + stats.dirichlet.logpdf(pos, alpha + ref_counts) + lnpriorref
        if sweep > 0 and sweep % thin == 0:
            out.append((pos, lnpost))
    return out, all_counts


def cdf_edge_clearance(pdfs, pos, u):
    """smallest relative distance of a target u * total to an edge of the row's running sum"""
    cdf = np.cumsum(pdfs * pos, axis=1)
    tot = cdf[:, -1:]
    return float(np.min(np.abs(cdf - u[:, None] * tot) / tot))


def batch_means(x, nb=HIER_BATCHES):
    """mean and batch-means standard error along axis 0"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x) // nb * nb
    b = x[:n].reshape((nb, n // nb) + x.shape[1:]).mean(axis=1)
    return x.mean(axis=0), b.std(axis=0, ddof=1) / np.sqrt(nb)


@pytest.fixture(scope='module')
def g():
    return dict(np.load(G16))


@pytest.fixture(scope='module')
def samplers():
    from frankenz_amd import samplers
    return samplers


@pytest.mark.parametrize('tag', list(POP))
def test_predrawn_tables_are_the_references_stream(g, samplers, tag):
    c = POP[tag]
    G = c['stack'][2]
    rs = np.random.RandomState(int(g[tag + '_seed']))
    runs = 2 if c.get('twice') else 1
    got = [samplers._predraw_population(rs, G, c['Niter'], c['thin'], c['mh_steps']) for _ in range(runs)]
    for k, name in enumerate(('pairs', 'normals', 'expo')):
        np.testing.assert_array_equal(np.concatenate([r[k] for r in got]), g['%s_%s' % (tag, name)])


@pytest.mark.parametrize('tag', list(POP))
def test_restated_population_chain_equals_the_reference(g, tag):
    c = POP[tag]
    pdfs = case_stack(g, tag, c['stack'])
    pos_init, prior, pargs = case_extras(tag, pdfs.shape[1])
    pairs, normals, expo = g[tag + '_pairs'], g[tag + '_normals'], g[tag + '_expo']
    runs = 2 if c.get('twice') else 1
    n = len(pairs) // runs
    smp, lnp, acc, gs = [], [], [], []
    for r in range(runs):                                       # (case f: the second run_mcmc restarts from the stacked PDFs)
        pos0 = pdfs.sum(axis=0) / pdfs.sum() if pos_init is None else pos_init
        sl = slice(r * n, (r + 1) * n)
        out = restated_population(pdfs, pos0, pairs[sl], normals[sl], expo[sl], c['thin'], prior, pargs)
        smp.append(out[0]); lnp.append(out[1]); acc.append(out[2]); gs.append(out[4])
    np.testing.assert_array_equal(np.concatenate(smp), g[tag + '_samples'])
    np.testing.assert_array_equal(np.concatenate(lnp), g[tag + '_samples_lnp'])
    np.testing.assert_array_equal(np.concatenate(acc), g[tag + '_accept'])
    np.testing.assert_array_equal(np.concatenate(gs), g[tag + '_gscale'])
    assert float(g[tag + '_min_margin']) >= 30 * float(g[tag + '_sens_lnp'])


def test_philox_known_answers(samplers):
    """Philox4x32-10 known answers (Random123's kat_vectors; Salmon et al., SC'11)"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        out = samplers._philox4x32(key, np.array([ctr], dtype=np.uint64))
        assert tuple(int(v) for v in out[0]) == want


def test_philox_uniforms(samplers):
    key = (0x12345678, 0x9abcdef0)
    u = samplers._philox_uniform(key, 3, 1000000)
    assert u.dtype == np.float64 and u.min() >= 0. and u.max() < 1.
    n = len(u)
    assert abs(u.mean() - 0.5) < 5 * math.sqrt(1. / 12 / n)
    assert abs(u.var() - 1. / 12) < 5 * math.sqrt(1. / 180 / n)                 # var of (u - 1/2)^2 is 1/180
    # the counter is (object, sweep): the 64 bits of one draw, by hand
    o = samplers._philox4x32(key, np.array([[5, 0, 3, 0]], dtype=np.uint64))[0]
    assert u[5] == ((int(o[0]) >> 5) * 2**26 + (int(o[1]) >> 6)) / 2.**53
    assert not np.array_equal(u[:1000], samplers._philox_uniform(key, 4, 1000))
    assert not np.array_equal(u[:1000], samplers._philox_uniform((key[0], key[1] + 1), 3, 1000))
    np.testing.assert_array_equal(u[:1000], samplers._philox_uniform(key, 3, 1000))


def _sig(fn, drop=()):
    ps = [p for n, p in inspect.signature(fn).parameters.items() if n not in drop]
    return str(inspect.Signature(ps))


@pytest.mark.parametrize('cls,extra', [('population_sampler', {}), ('hierarchical_sampler', {'run_mcmc': ('draws',), 'sample': ('draws',)})])
def test_interfaces_are_the_references(g, samplers, cls, extra):
    """constructor, reset, run_mcmc and sample take the reference's arguments with its defaults; additive: device= on the
    constructors, draws= on the hierarchical sampler"""
    klass = getattr(samplers, cls)
    for m in ('__init__', 'reset', 'run_mcmc', 'sample'):
        drop = ('device',) if m == '__init__' else extra.get(m, ())
        assert _sig(getattr(klass, m), drop) == str(g['sig_%s_%s' % (cls, m)]), m
        for name in drop:
            assert name in inspect.signature(getattr(klass, m)).parameters
    assert isinstance(klass.results, property)


@pytest.mark.parametrize('tag', list(HIER))
def test_hierarchical_restatement_is_finite_and_reproducible(g, tag):
    c = HIER[tag]
    pdfs = case_stack(g, tag, c['stack'])
    alpha, ref, beta = hier_extras(tag, pdfs.shape[1])

    def run():
        rs = np.random.RandomState(77)
        return restated_hierarchical(pdfs, 6, 2, alpha, ref, beta, rs, lambda sweep: rs.rand(len(pdfs)))
    a, ca = run()
    b, cb = run()
    assert len(a) == 6 and len(ca) == 13
    for (p1, l1), (p2, l2) in zip(a, b):
        assert np.isfinite(l1) and l1 == l2
        np.testing.assert_array_equal(p1, p2)
        assert abs(p1.sum() - 1.) < 1e-12 and (p1 >= 0).all()
    assert all(int(x.sum()) == len(pdfs) for x in ca)
