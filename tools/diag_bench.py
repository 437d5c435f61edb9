"""The validation sums of frankenz_amd.plotting at the headline size (1e6 objects x 701 x 701), on PDFs the package's own
fit_predict makes from the bench generator: the 2-D truth-vs-PDF stack with the sorted tile ranges and again with every tile given
the full object range, and the PIT pass (cdf_vs_epdf) at Nmc = 100.  Baselines: k_gemm_f64's 23.7 ms for the same dense flop count
(docs/summary_nz.md) and the restated host loop (tests/_diag_ref.py) timed on 2 000 objects and scaled linearly in N (objects are
independent).  Prints one JSON line.

    timeout -k 10 900 python tools/diag_bench.py [--objects 1000000] [--models 100000] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(eng, fn, repeat):
    wall, kern = [], []
    for _ in range(repeat):
        eng.timing_reset()
        t0 = time.perf_counter()
        fn()
        wall.append(time.perf_counter() - t0)
        kern.append(eng.timing()['ms_other'])
    return 1e3 * float(np.median(wall)), float(np.median(kern))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=1000000)
    ap.add_argument('--models', type=int, default=100000)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--host-objects', type=int, default=2000)
    a = ap.parse_args()
    import bench
    import _diag_ref as ref
    from frankenz_amd import BruteForce, PDFDict, plotting
    from frankenz_amd.engine import get_engine
    N, M = a.objects, a.models
    Y, Ye, Ym, X, Xe, Xm, z, ze = bench.make_problem(N, M, 0)
    rs = np.random.RandomState(0)                          # the generator's stream again, for the model behind every object
    rs.lognormal(mean=1.0, sigma=1.0, size=Y.shape)
    truth = z[rs.randint(0, M, size=N)]
    terr = np.full(N, 0.05)
    grid = np.arange(0, 7 + 1e-5, .01)
    d = PDFDict(grid, np.linspace(.005, 2, 500))
    pdfs = BruteForce(Y, Ye, Ym).fit_predict(X, Xe, Xm, z, ze, label_dict=d, save_fits=False, verbose=False)
    pdfs = np.ascontiguousarray(pdfs[0] if isinstance(pdfs, tuple) else pdfs)
    eng = get_engine()
    dev = eng.device_array(pdfs)
    G = len(grid)
    sel = plotting.stack_selection(truth, terr, d)
    out = {'metric': 'diag_stack2d', 'objects': N, 'grid_x': d.Ngrid, 'grid_y': G, 'selected': int(len(sel[0])),
           'dense_flops': 2.0 * N * d.Ngrid * G, 'k_gemm_f64_ms_same_flops': 23.7}
    stacks = {}
    for name, full in (('sorted', False), ('full_range', True)):
        fn = lambda: stacks.__setitem__(name, plotting._stack(eng, d, dev, G, sel, 1e-3, 2e-4, full_range=full))      # noqa: E731
        fn()
        out['wall_ms_' + name], out['kernel_ms_' + name] = timed(eng, fn, a.repeat)
    out['full_range_equals_sorted'] = bool(np.allclose(stacks['sorted'], stacks['full_range'], rtol=1e-11, atol=0))
    t0 = time.perf_counter()
    plotting.input_vs_pdf(truth, terr, d, dev, grid, plot=False)
    out['wall_ms_input_vs_pdf_resident'] = 1e3 * (time.perf_counter() - t0)
    fn = lambda: plotting.cdf_vs_epdf(truth, terr, dev, grid, Nmc=100, rstate=np.random.RandomState(1), plot=False)   # noqa: E731
    fn()
    out['wall_ms_cdf_vs_epdf_nmc100'], out['kernel_ms_cdf_vs_epdf_nmc100'] = timed(eng, fn, a.repeat)
    # the host loops on a slice, scaled linearly
    n = min(N, a.host_objects)
    t0 = time.perf_counter()
    want = ref.input_vs_pdf(truth[:n], terr[:n], d, pdfs[:n], grid)
    out['host_loop_s_stack_scaled'] = (time.perf_counter() - t0) * N / n
    got = plotting.input_vs_pdf(truth[:n], terr[:n], d, pdfs[:n], grid, plot=False)
    nz = want != 0
    out['slice_max_rel_diff'] = float(np.abs(got[nz] / want[nz] - 1).max())
    t0 = time.perf_counter()
    ref.cdf_vs_epdf(truth[:n], terr[:n], pdfs[:n], grid, Nmc=100, rstate=np.random.RandomState(1))
    out['host_loop_s_pit_scaled'] = (time.perf_counter() - t0) * N / n
    print(json.dumps(out))


if __name__ == '__main__':
    main()
