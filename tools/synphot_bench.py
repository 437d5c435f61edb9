"""Synthetic photometry (fz_synphot) at the sizes of a mock catalogue: (template, redshift) pairs through synthetic curves of the
sizes of two of the reference's surveys -- LSST-like (6 filters x 2 100 points) and COSMOS-like (32 filters x 630 points) -- and 8
templates of 2 300 and 6 900 points, with the Madau attenuation on, redshifts uniform in [0, 6].  GPU: 1e5 and 1e6 pairs (wall time
of the engine call with host arrays in and out, which ends in a device synchronise, and the kernel's own time from device events);
host: the package's vectorised NumPy path at 1e4 pairs.  The reference's own loop is not run here (its data files are not shipped;
docs/simulate.md quotes its per-pair times from a CPU).  A slice of the GPU result is compared with the host path.  Every shape is
warmed up once and timed `--repeat` times (median).  Prints one JSON line.

    timeout -k 10 900 python tools/synphot_bench.py [--pairs 100000 1000000] [--host-pairs 10000] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SURVEYS = {'lsst_like': (6, 2100), 'cosmos_like': (32, 630)}
TEMPLATE_POINTS = (2300, 6900, 2300, 6900, 2300, 6900, 2300, 6900)


def make_survey(nf, npts, seed=0):
    from frankenz_amd import simulate
    rs = np.random.RandomState(seed)
    ms = simulate.MockSurvey()
    names, waves, trans = [], [], []
    for i in range(nf):
        lo = 3000. * (25000. / 3000.)**(i / float(nf))              # bands from 3000 A to 2.5 um, 12 % wide
        w = np.linspace(lo, 1.12 * lo, npts)
        names.append('f%d' % i); waves.append(w); trans.append(np.exp(-0.5 * ((w - w.mean()) / (0.03 * lo))**2) + 0.01)
    ms.set_filters(names, waves, trans, np.full(nf, 25.))
    ms.set_refmag(0, mode='counter')
    tn, tt, tw, tf = [], [], [], []
    for i, n in enumerate(TEMPLATE_POINTS):
        w = np.exp(np.linspace(np.log(91.), np.log(1.6e6), n))
        fl = (w / 5000.)**(-2.0 + 0.4 * i) * (1. + 0.8 * (w > 4000.)) * (0.02 + (w > 912.)) * (1. + 0.05 * rs.rand(n))
        tn.append('t%d' % i); tt.append('T%d' % (i % 3)); tw.append(w); tf.append(fl)
    ms.set_templates(tn, tt, tw, tf)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--host-pairs', type=int, default=10000)
    ap.add_argument('--repeat', type=int, default=3)
    a = ap.parse_args()
    from frankenz_amd import simulate
    from frankenz_amd.engine import get_engine
    eng = get_engine()
    out = {'metric': 'synphot', 'igm': 'madau+99', 'templates': list(TEMPLATE_POINTS)}
    for sname, (nf, npts) in SURVEYS.items():
        ms = make_survey(nf, npts)
        tb = simulate._Tables(ms.filters, ms.templates)
        rs = np.random.RandomState(1)
        res = {'filters': nf, 'filter_points': nf * npts}
        for n in a.pairs:
            tmpl, z = rs.randint(0, len(TEMPLATE_POINTS), n).astype(np.int64), rs.uniform(0., 6., n)
            ln1pz, phot = np.log(1 + z), np.empty((n, nf))
            eng.synphot_upload(tb)
            eng.synphot(tmpl, z, ln1pz, 1, phot)                     # warm-up of this shape
            wall, kern = [], []
            for _ in range(a.repeat):
                eng.timing_reset()
                t0 = time.perf_counter()
                eng.synphot(tmpl, z, ln1pz, 1, phot)
                wall.append(time.perf_counter() - t0)
                kern.append(eng.timing()['ms_other'])
            res['gpu_%d_pairs' % n] = {'wall_ms': 1e3 * float(np.median(wall)), 'kernel_ms': float(np.median(kern)),
                                       'wall_ms_all': [1e3 * w for w in wall],
                                       'point_evaluations_per_s': n * nf * npts / (1e-3 * float(np.median(kern)))}
        n = a.host_pairs
        t0 = time.perf_counter()
        want = simulate._synphot_host(tb, tmpl[:n], z[:n], ln1pz[:n], 1)
        res['host_%d_pairs_s' % n] = time.perf_counter() - t0
        res['host_us_per_pair'] = 1e6 * res['host_%d_pairs_s' % n] / n
        ok = want != 0
        res['slice_max_rel_diff'] = float(np.abs(phot[:n][ok] / want[ok] - 1).max())
        out[sname] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
