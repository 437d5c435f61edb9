"""population_sampler and hierarchical_sampler on the device (fz_nz_pairs, fz_nz_pair_eval, fz_nz_sweep, fz_pdfs_colsum) against
G16, the reference's own chains (tests/golden/make_golden_nz.py), and against the NumPy restatements of
tests/test_nz_samplers_host.py."""
import os
import sys

import numpy as np
import pytest

from frankenz_amd import samplers
from conftest import DevArray
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_nz_samplers_host as th  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return dict(np.load(th.G16))


def run_population(pdfs, c, seed, pos_init=None, prior=None, pargs=(), runs=1, verbose=False):
    s = samplers.population_sampler(pdfs)
    rs = np.random.RandomState(seed)
    acc, gs = [], []
    for _ in range(runs):
        s.run_mcmc(c['Niter'], logprior_nz=prior, pos_init=pos_init, thin=c['thin'], mh_steps=c['mh_steps'], rstate=rs, verbose=verbose,
                   prior_args=list(pargs))
        acc.append(s.chain_accept); gs.append(s.chain_gscale)
    smp, lnp = s.results
    return smp, lnp, np.concatenate(acc), np.concatenate(gs), s


@pytest.mark.parametrize('tag', list(th.POP))
def test_population_chain_follows_the_reference(g, tag):
    """Every G16 case: the accept flag of every proposal equals the reference's; samples within 10 x sens_pos x max(pos), ln-posteriors
    within 10 x sens_lnp, where sens_* is how far the reference's own chain moves under a reordered sum (measured by the generator).
    gscale = min(|1 / grad|, 1e4 scale): a sum's noise dl enters grad as 2 dl / scale, so gscale moves by at most a relative
    gscale * 2 dl / scale <= 2e4 dl; dl is taken as 10 x sens_lnp like the ln-posterior's.  Case e runs the host-prior route, case f
    calls run_mcmc twice (the second restarts from the stacked PDFs, as the reference's does)."""
    c = th.POP[tag]
    pdfs = th.case_stack(g, tag, c['stack'])
    pos_init, prior, pargs = th.case_extras(tag, pdfs.shape[1])
    smp, lnp, acc, gs, _ = run_population(pdfs, c, int(g[tag + '_seed']), pos_init, prior, pargs, runs=2 if c.get('twice') else 1)
    ref_s, ref_l = g[tag + '_samples'], g[tag + '_samples_lnp']
    sens_pos, sens_lnp = float(g[tag + '_sens_pos']), float(g[tag + '_sens_lnp'])
    print('%s: flags differing %d of %d; max|dpos|/max(pos) %.3g (sens %.3g); max|dlnp| %.3g (sens %.3g); max rel dgscale %.3g' %
          (tag, int((acc != g[tag + '_accept']).sum()), acc.size, np.max(np.abs(smp - ref_s)) / np.max(ref_s), sens_pos,
           np.max(np.abs(lnp - ref_l)), sens_lnp, np.max(np.abs(gs / g[tag + '_gscale'] - 1.))))
    np.testing.assert_array_equal(acc, g[tag + '_accept'])
    assert smp.shape == ref_s.shape and lnp.shape == ref_l.shape
    assert np.max(np.abs(smp - ref_s)) <= 10 * sens_pos * np.max(ref_s)
    assert np.max(np.abs(lnp - ref_l)) <= 10 * sens_lnp
    np.testing.assert_allclose(gs, g[tag + '_gscale'], rtol=2e4 * 10 * sens_lnp)


def test_population_chain_is_reproducible_and_segment_independent(g, monkeypatch):
    pdfs = th.case_stack(g, 'a', th.POP['a']['stack'])
    c = dict(Niter=9, thin=10, mh_steps=3)
    base = run_population(pdfs, c, 424)
    again = run_population(pdfs, c, 424)
    for a, b in zip(base[:4], again[:4]):
        np.testing.assert_array_equal(a, b)
    for seg in (1, 7, 100):
        monkeypatch.setattr(samplers, '_NZ_SEGMENT', seg)
        out = run_population(pdfs, c, 424)
        for a, b in zip(base[:4], out[:4]):
            np.testing.assert_array_equal(a, b)
    assert base[2].shape == (90, 3) and base[3].shape == (90,) and 0 < base[2].sum() < 270


def test_zero_prior_through_the_host_route_equals_the_device_route(g):
    pdfs = th.case_stack(g, 'a', th.POP['a']['stack'])
    c = dict(Niter=3, thin=20, mh_steps=3)
    calls = []

    def flat(pos, *args, **kw):
        calls.append((len(pos), args, kw))
        return 0.
    dev = run_population(pdfs, c, 77)
    s = samplers.population_sampler(pdfs)
    s.run_mcmc(3, logprior_nz=flat, thin=20, mh_steps=3, rstate=np.random.RandomState(77), verbose=False, prior_args=[1, 2],
               prior_kwargs={'k': 3})
    np.testing.assert_array_equal(s.results[0], dev[0])
    np.testing.assert_array_equal(s.results[1], dev[1])
    np.testing.assert_array_equal(s.chain_accept, dev[2])
    np.testing.assert_array_equal(s.chain_gscale, dev[3])
    assert len(calls) == 1 + 60 * 5 and calls[0] == (40, (1, 2), {'k': 3})
    # the host route keeps the device's overlap up to date as well
    pos = s.results[0][-1]
    np.testing.assert_allclose(s._overlap.numpy(), pdfs @ pos, rtol=1e-12)


def test_stack_as_numpy_and_as_device_arrays(g):
    """a stack already in device memory -- allocated outside the library (DevArray) or by the engine (DeviceArray) -- is used as it
    is and gives the chains of the NumPy stack"""
    from frankenz_amd.engine import get_engine
    pdfs = th.case_stack(g, 'a', th.POP['a']['stack'])
    c = dict(Niter=2, thin=15, mh_steps=3)
    base = run_population(pdfs, c, 5)
    for dev in (DevArray(pdfs), get_engine().device_array(pdfs)):
        out = run_population(dev, c, 5)
        for a, b in zip(base[:4], out[:4]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(samplers.stack_nz(dev), samplers.stack_nz(pdfs))
        h1, h2 = samplers.hierarchical_sampler(pdfs), samplers.hierarchical_sampler(dev)
        for h in (h1, h2):
            h.run_mcmc(3, thin=2, rstate=np.random.RandomState(9), verbose=False)
        np.testing.assert_array_equal(h1.results[0], h2.results[0])
    np.testing.assert_allclose(samplers.stack_nz(pdfs), pdfs.sum(axis=0) / pdfs.sum(), rtol=1e-13)


def test_population_full_size():
    """1e6 x 701, Niter=2, thin=20 (120 proposals): pos stays a distribution and the incrementally updated overlap stays at
    pdfs @ pos.  The bound on the overlap's drift is the NumPy restatement's own at 2e4 objects under the same settings (its final
    overlap against np.dot(pdfs, pos): 1.8e-15 relative when this test was written; it is measured again here), scaled by
    sqrt(1e6 / 2e4)."""
    from frankenz_amd.engine import get_engine
    small = th.nz_stack(1620, 20000, 701)
    rs = np.random.RandomState(1621)
    tabs = samplers._predraw_population(rs, 701, 2, 20, 3)
    out = th.restated_population(small, small.sum(axis=0) / small.sum(), tabs[0], tabs[1], tabs[2], 20)
    drift_small = np.max(np.abs(out[5] / np.dot(small, out[0][-1]) - 1.))
    print('restatement at 2e4 objects: accepted %d of 120, overlap drift %.3g' % (out[2].sum(), drift_small))
    assert out[2].sum() >= 10 and 0 < drift_small < 1e-14
    N, G = 1000000, 701
    pdfs = get_engine().device_empty((N, G))
    rs = np.random.RandomState(1622)
    for r0 in range(0, N, 100000):                                 # the stack is made on the host in pieces and stays on the device
        cen = rs.uniform(0., G - 1., 100000)[:, None]
        x = (np.arange(G)[None, :] - cen) / rs.uniform(5., 45., 100000)[:, None]
        p = np.exp(-0.5 * x * x) + 1e-4
        pdfs.set_rows(r0, p / p.sum(axis=1)[:, None])
    del x, p
    s = samplers.population_sampler(pdfs)
    s.run_mcmc(2, thin=20, rstate=np.random.RandomState(1623), verbose=False)
    smp, lnp = s.results
    assert smp.shape == (2, G) and np.isfinite(lnp).all() and s.chain_accept.sum() >= 10
    assert (smp >= 0.).all() and np.max(np.abs(smp.sum(axis=1) - 1.)) < 1e-9
    lnl, ov = samplers.loglike_nz(smp[-1], pdfs, return_overlap=True)
    drift = np.max(np.abs(s._overlap.numpy() / ov - 1.))
    print('1e6 x 701: accepted %d of 120, overlap drift %.3g (bound %.3g), lnpost %.6f vs recomputed %.6f' %
          (s.chain_accept.sum(), drift, drift_small * np.sqrt(N / 2e4), lnp[-1], lnl))
    assert drift <= drift_small * np.sqrt(N / 2e4)
    assert abs(lnp[-1] - lnl) <= 1e-9 * abs(lnl)


def hier_stack(seed, N, G):
    rs = np.random.RandomState(seed)
    cen = rs.uniform(0.05, 0.95, N)[:, None] * G
    p = np.exp(-0.5 * ((np.arange(G)[None, :] - cen) / rs.uniform(1.5, 0.08 * G + 2., N)[:, None]) ** 2)
    p[p < 1e-12] = 0.
    return p / p.sum(axis=1)[:, None]


def hier_hyper(seed, G, ref):
    rs = np.random.RandomState(seed)
    alpha = rs.uniform(0.5, 2., G)
    if not ref:
        return alpha, None, None
    return alpha, rs.multinomial(500, rs.dirichlet(np.full(G, 3.))).astype(np.float64), rs.uniform(0.5, 1.5, G)


@pytest.mark.parametrize('draws', ['host', 'device'])
@pytest.mark.parametrize('ref', [False, True])
@pytest.mark.parametrize('N,G,seed', [(3000, 50, 1631), (600, 1537, 1632)])
def test_hierarchical_chain_equals_the_restatement(draws, ref, N, G, seed):
    """counts of every sweep, pos and lnpost equal the restatement built on the oracle's nz_assign and the same RandomState, fed by
    rstate.rand(N) (draws='host') or by _philox_uniform (draws='device'); 13 sweeps.  Precondition, asserted on the CPU side: no
    target u * total within 1e-9 (relative) of an edge of the row's running sum, where the device's summation order could flip a bin.
    G = 1537 is beyond the LDS staging of the weighted rows."""
    pdfs = hier_stack(seed, N, G)
    alpha, refs, beta = hier_hyper(seed + 100, G, ref)
    rs = np.random.RandomState(seed + 200)
    clear = []
    if draws == 'host':
        want, wcounts = th.restated_hierarchical(pdfs, 4, 3, alpha, refs, beta, rs, lambda sweep: rs.rand(N), clearance=clear)
    else:
        key = rs.randint(0, 2**32, size=2, dtype=np.uint32)
        want, wcounts = th.restated_hierarchical(pdfs, 4, 3, alpha, refs, beta, rs, lambda sweep: samplers._philox_uniform(key, sweep, N),
                                                 clearance=clear)
    assert min(clear) > 1e-9, min(clear)
    s = samplers.hierarchical_sampler(pdfs)
    s.run_mcmc(4, alpha=alpha, thin=3, ref_sample=refs, beta=beta, rstate=np.random.RandomState(seed + 200), verbose=False, draws=draws)
    assert len(s.sweep_counts) == 13
    for a, b in zip(s.sweep_counts, wcounts):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(s.results[0], np.array([w[0] for w in want]))
    np.testing.assert_array_equal(s.results[1], np.array([w[1] for w in want]))
    if draws == 'device':
        np.testing.assert_array_equal(s.philox_key, key)
        assert any(not np.array_equal(s.sweep_counts[k], s.sweep_counts[k + 1]) for k in range(12))
        k1 = s.philox_key.copy()
        rs2 = np.random.RandomState(seed + 200)
        gen = s.sample(1, alpha=alpha, thin=1, rstate=rs2)
        next(gen); gen.close()
        gen = s.sample(1, alpha=alpha, thin=1, rstate=rs2)                # the same stream, further on: a new key
        next(gen)
        assert not np.array_equal(s.philox_key, k1)
    else:
        assert s.philox_key is None


@pytest.mark.parametrize('draws', ['host', 'device'])
@pytest.mark.parametrize('tag', list(th.HIER))
def test_hierarchical_law_against_the_reference_chain(g, tag, draws):
    """device chains of the G16 hierarchical cases, same length as the reference's: per bin |mean - mean_ref| <= 5 sqrt(se^2 +
    se_ref^2) with batch-means standard errors (20 batches); bins with fewer than 10 expected objects pooled; the same for lnpost."""
    c = th.HIER[tag]
    pdfs = th.case_stack(g, tag, c['stack'])
    N = len(pdfs)
    alpha, ref, beta = th.hier_extras(tag, pdfs.shape[1])
    s = samplers.hierarchical_sampler(pdfs)
    s.run_mcmc(th.HIER_NITER, alpha=alpha, thin=th.HIER_THIN, ref_sample=ref, beta=beta, rstate=np.random.RandomState(1640 + ord(tag)),
               verbose=False, draws=draws)
    smp, lnp = s.results
    assert smp.shape == (th.HIER_NITER, pdfs.shape[1]) and np.isfinite(lnp).all()
    mean, se = th.batch_means(smp)
    rmean, rse = g[tag + '_pos_mean'], g[tag + '_pos_se']
    rare = rmean * N < 10
    dev = np.abs(mean - rmean) / np.sqrt(se**2 + rse**2)
    print('%s %s: largest per-bin deviation %.2f sigma, %d bins pooled' % (tag, draws, dev[~rare].max(), rare.sum()))
    assert (dev[~rare] <= 5.).all()
    if rare.any():
        pm, pse = th.batch_means(smp[:, rare].sum(axis=1))
        assert abs(pm - rmean[rare].sum()) <= 5 * np.sqrt(pse**2 + np.sum(rse[rare]**2)) + 10. / N
    lm, lse = th.batch_means(lnp)
    print('%s %s: lnpost %.3f +- %.3f, reference %.3f +- %.3f' % (tag, draws, lm, lse, float(g[tag + '_lnp_mean']), float(g[tag + '_lnp_se'])))
    assert abs(lm - float(g[tag + '_lnp_mean'])) <= 5 * np.sqrt(lse**2 + float(g[tag + '_lnp_se'])**2)


@pytest.mark.parametrize('draws', ['host', 'device'])
def test_hierarchical_rows_without_mass(draws):
    """objects whose PDF has no mass where pos has any (bin -1 of nz_assign; the reference raises from multinomial on the nan row) are
    left out of that sweep's counts; the chain goes on"""
    pdfs = hier_stack(1650, 2000, 40)
    pdfs[:7] = 0.
    pdfs[:7, 3] = 1.
    pdfs[7:, 3] = 0.
    pdfs[7:] /= pdfs[7:].sum(axis=1)[:, None]
    pos0 = pdfs[7:].sum(axis=0) / pdfs[7:].sum()
    assert pos0[3] == 0.
    s = samplers.hierarchical_sampler(pdfs)
    s.run_mcmc(5, pos_init=pos0, thin=2, rstate=np.random.RandomState(3), verbose=False, draws=draws)
    assert s.sweep_counts[0].sum() == 1993 and s.sweep_counts[0][3] == 0
    assert all(c.sum() == 2000 and c[3] == 7 for c in s.sweep_counts[1:])
    assert np.isfinite(s.results[1]).all() and np.isfinite(s.results[0]).all()


def test_population_two_bins_and_bad_start():
    """G = 2: every pair is (0, 1) or (1, 0); the flags equal the restatement's.  A start with a negative or non-finite entry, which
    freezes the reference's chain at lnpost = -inf, is refused."""
    rs = np.random.RandomState(1660)
    a = rs.beta(2., 2., 5000)
    pdfs = np.stack([a, 1. - a], axis=1)
    c = dict(Niter=4, thin=10, mh_steps=3)
    smp, lnp, acc, gs, s = run_population(pdfs, c, 1661)
    tabs = samplers._predraw_population(np.random.RandomState(1661), 2, 4, 10, 3)
    assert set(map(tuple, tabs[0])) <= {(0, 1), (1, 0)}
    want = th.restated_population(pdfs, pdfs.sum(axis=0) / pdfs.sum(), tabs[0], tabs[1], tabs[2], 10)
    if want[3][np.isfinite(want[3])].min() > 1e-6:                       # (no decision within summation noise)
        np.testing.assert_array_equal(acc, want[2])
        np.testing.assert_allclose(smp, want[0], rtol=1e-6)
    assert np.max(np.abs(smp.sum(axis=1) - 1.)) < 1e-12
    for bad in ([-0.1, 1.1], [np.nan, 1.], [np.inf, 0.]):
        with pytest.raises(ValueError):
            s.run_mcmc(1, pos_init=np.array(bad), thin=2, rstate=rs, verbose=False)
    with pytest.raises(ValueError):
        samplers.population_sampler(pdfs[:, :1].copy()).run_mcmc(1, thin=2, verbose=False)


def test_bookkeeping_and_progress_line(g, capsys):
    pdfs = th.case_stack(g, 'a', th.POP['a']['stack'])
    for s, kw in ((samplers.population_sampler(pdfs), dict(thin=5)), (samplers.hierarchical_sampler(pdfs), dict(thin=2))):
        assert s.results[0].shape == (0,)
        s.run_mcmc(3, rstate=np.random.RandomState(1), **kw)
        err = capsys.readouterr().err
        assert err.count('\r Sample ') == 3 and ' Sample 3/3 [lnpost = ' in err
        assert s.results[0].shape == (3, 40) and s.results[1].shape == (3,)
        s.run_mcmc(2, rstate=np.random.RandomState(1), verbose=False, **kw)
        assert capsys.readouterr().err == ''
        assert s.results[0].shape == (5, 40)
        np.testing.assert_array_equal(s.results[0][3:], s.results[0][:2])      # the second run restarts from the stacked PDFs
        s.reset()
        assert s.samples == [] and s.samples_lnp == [] and s.results[0].shape == (0,)
    assert s.samples_prior == [] and s.samples_counts == []
