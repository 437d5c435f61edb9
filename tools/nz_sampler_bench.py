"""The n(z) samplers at the headline size (1e6 objects x 701 bins): wall clock and kernel time per Gibbs sweep
(hierarchical_sampler) and per saved sample (population_sampler), each against the same chain written as a Python loop over the
public pieces that existed before the samplers did (samplers.nz_assign / samplers.loglike_nz).  Prints one JSON line per sampler.

    timeout -k 10 600 python tools/nz_sampler_bench.py [--objects 1000000] [--grid 701] [--repeat 3] [--only population|hierarchical]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_stack(rs, n, G):
    cen = rs.uniform(0., G - 1., n)[:, None]
    x = (np.arange(G)[None, :] - cen) / rs.uniform(5., 45., n)[:, None]
    p = np.exp(-0.5 * x * x) + 1e-4
    return p / p.sum(axis=1)[:, None]


def timed(eng, fn):
    eng.timing_reset()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0, eng.timing()['ms_other'] * 1e-3


def bench_hierarchical(eng, samplers, d_pdfs, N, G, repeat, thin=5, niter=3):
    sweeps = niter * thin + 1
    out = {'metric': 'nz_hierarchical_sweep', 'objects': N, 'grid': G, 'sweeps_timed': sweeps}
    alpha = np.ones(G)
    for draws in ('device', 'host'):
        s = samplers.hierarchical_sampler(d_pdfs)
        s.run_mcmc(1, thin=1, rstate=np.random.RandomState(0), verbose=False, draws=draws)           # warm-up
        res = [timed(eng, lambda: s.run_mcmc(niter, thin=thin, rstate=np.random.RandomState(r), verbose=False, draws=draws))
               for r in range(repeat)]
        out['wall_ms_per_sweep_' + draws] = 1e3 * float(np.median([r[0] for r in res])) / sweeps
        out['kernel_ms_per_sweep_' + draws] = 1e3 * float(np.median([r[1] for r in res])) / sweeps
    # what a user wrote before: per sweep nz_assign on fresh host uniforms + the host Dirichlet
    pos0 = samplers.stack_nz(d_pdfs)

    def loop(seed):
        rs = np.random.RandomState(seed)
        pos = pos0
        for _ in range(sweeps):
            counts = samplers.nz_assign(pos, d_pdfs, u=rs.rand(N))
            pos = rs.dirichlet(alpha + counts)
    loop(0)
    res = [timed(eng, lambda: loop(r)) for r in range(repeat)]
    out['wall_ms_per_sweep_loop_over_nz_assign'] = 1e3 * float(np.median([r[0] for r in res])) / sweeps
    # k_nz_assign alone, everything on the device: what the in-kernel generator is held against
    u, bins, counts = eng.device_array(np.random.RandomState(1).rand(N)), eng.device_empty(N, np.int64), np.zeros(G, dtype=np.int64)
    eng.nz_assign(d_pdfs, pos0, u, bins, counts, n=N)
    res = [timed(eng, lambda: eng.nz_assign(d_pdfs, pos0, u, bins, counts, n=N)) for _ in range(max(repeat, 5))]
    out['kernel_ms_k_nz_assign'] = 1e3 * float(np.median([r[1] for r in res]))
    out['sweep_kernel_over_k_nz_assign'] = out['kernel_ms_per_sweep_device'] / out['kernel_ms_k_nz_assign']
    out['speedup_wall_vs_loop'] = out['wall_ms_per_sweep_loop_over_nz_assign'] / out['wall_ms_per_sweep_device']
    return out


def loop_population(samplers, pdfs, niter, thin, mh_steps, rs):
    """the population chain over the parent's loglike_nz(..., overlap=, pair=, pair_step=) on a NumPy stack"""
    pos = pdfs.sum(axis=0) / pdfs.sum()
    lnpost, overlap = samplers.loglike_nz(pos, pdfs, return_overlap=True)
    for _ in range(niter):
        pairs = [rs.choice(len(pos), size=2, replace=False) for _ in range(thin)]
        for pair in pairs:
            t = np.zeros_like(pos)
            t[pair] = (1, -1)
            scale = 1e-4 * np.min(np.append(pos[pair], 1. - pos[pair]))
            grad = (samplers.loglike_nz(pos, pdfs, overlap=overlap, pair=pair, pair_step=scale / 2.) -
                    samplers.loglike_nz(pos, pdfs, overlap=overlap, pair=pair, pair_step=-scale / 2.)) / scale
            gscale = min(abs(1. / grad), abs(scale * 1e4)) if grad != 0. else abs(scale)
            for _k in range(mh_steps):
                z = rs.randn() * gscale
                new = pos + t * z
                lnew, onew = samplers.loglike_nz(new, pdfs, overlap=overlap, return_overlap=True, pair=pair, pair_step=z)
                if -rs.exponential() < lnew - lnpost:
                    pos, lnpost, overlap = new, lnew, onew
    return pos


def bench_population(eng, samplers, d_pdfs, N, G, repeat, thin=20, niter=2, nloop=100000):
    out = {'metric': 'nz_population_sample', 'objects': N, 'grid': G, 'thin': thin, 'mh_steps': 3}
    s = samplers.population_sampler(d_pdfs)
    s.run_mcmc(1, thin=2, rstate=np.random.RandomState(0), verbose=False)
    res = [timed(eng, lambda: s.run_mcmc(niter, thin=thin, rstate=np.random.RandomState(r), verbose=False)) for r in range(repeat)]
    out['wall_ms_per_sample'] = 1e3 * float(np.median([r[0] for r in res])) / niter
    out['kernel_ms_per_sample'] = 1e3 * float(np.median([r[1] for r in res])) / niter
    out['kernel_us_per_pair'] = 1e3 * out['kernel_ms_per_sample'] / thin
    # the loop a user wrote before, on a NumPy stack of `nloop` objects, and the sampler at that size
    nloop = min(nloop, N)
    small = host_stack(np.random.RandomState(3), nloop, G)
    with np.errstate(invalid='ignore', divide='ignore'):
        loop_population(samplers, small, 1, 2, 3, np.random.RandomState(0))
        t = []
        for r in range(repeat):
            t0 = time.perf_counter()
            loop_population(samplers, small, niter, thin, 3, np.random.RandomState(r))
            t.append((time.perf_counter() - t0) / niter)
    out['loop_objects'] = nloop
    out['wall_ms_per_sample_loop_over_loglike_nz'] = 1e3 * float(np.median(t))
    s2 = samplers.population_sampler(small)
    s2.run_mcmc(1, thin=2, rstate=np.random.RandomState(0), verbose=False)
    res = [timed(eng, lambda: s2.run_mcmc(niter, thin=thin, rstate=np.random.RandomState(r), verbose=False)) for r in range(repeat)]
    out['wall_ms_per_sample_at_loop_objects'] = 1e3 * float(np.median([r[0] for r in res])) / niter
    out['speedup_wall_vs_loop_at_loop_objects'] = out['wall_ms_per_sample_loop_over_loglike_nz'] / out['wall_ms_per_sample_at_loop_objects']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=1000000)
    ap.add_argument('--grid', type=int, default=701)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--only', choices=['population', 'hierarchical'], default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from frankenz_amd import samplers
    from frankenz_amd.engine import get_engine
    eng = get_engine(None)
    N, G = args.objects, args.grid
    d_pdfs = eng.device_empty((N, G))
    rs = np.random.RandomState(1622)
    for r0 in range(0, N, 100000):
        n = min(100000, N - r0)
        d_pdfs.set_rows(r0, host_stack(rs, n, G))
    if args.only != 'population':
        print(json.dumps(bench_hierarchical(eng, samplers, d_pdfs, N, G, args.repeat)))
    if args.only != 'hierarchical':
        print(json.dumps(bench_population(eng, samplers, d_pdfs, N, G, args.repeat)))


if __name__ == '__main__':
    main()
