"""PDFs per second of the fused fit_predict with the BPZ prior P(z, t | m) (priors.logprob_bpz: two rows of a (1000, M) table
per object, blended in the kernel) against the only way to run the same problem without it: a dense (N, M) ln-prior formed on
the device (torch: gather two rows, blend, log -- from the same (1000, M) table, so the baseline is not charged for building
it) and handed to pdf.logprob_prior, the time to form it counted.  Mode B (free scale, model errors ignored: the demo's
likelihood), 5 bands, the demo's dictionary KDE; inputs and results device-resident.  Prints one JSON line per problem size.

    timeout -k 10 600 python tools/bpz_prior_bench.py [--objects 100000] [--models 8000 100000] [--repeat 3] [--dense-max-gb 40]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SDSS_SIGMA = np.array([0.873, 0.348, 0.418, 0.873, 3.476])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--objects', type=int, default=100000)
    ap.add_argument('--models', type=int, nargs='+', default=[8000, 100000], help='multiples of 8 (z grid x 8 templates)')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--dense-max-gb', type=float, default=40., help='skip the dense baseline above this table size')
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import torch
    from frankenz_amd import PDFDict, priors
    from frankenz_amd.engine import get_engine, kde_opts, like_opts
    from frankenz_amd.pdf import logprob_prior
    eng = get_engine(None)
    dev = torch.device('cuda', 0)
    pd = PDFDict(np.arange(0, 7 + 1e-5, .01), np.linspace(.005, 2, 500))
    opts, ko = like_opts({'free_scale': True, 'ignore_model_err': True}), kde_opts({'wt_thresh': 1e-3})
    N, B = args.objects, 5
    for M in args.models:
        rs = np.random.RandomState(181)
        nz = M // 8
        Y = rs.lognormal(1., 1., size=(M, B)) * 4; Ye = np.zeros_like(Y); Ym = np.ones_like(Y)
        model_z, model_type = np.repeat(np.linspace(0., 6., nz), 8), np.tile([0, 0, 1, 1, 1, 2, 2, 2], nz)
        X = Y[rs.choice(M, N)] * rs.uniform(0.5, 2., size=(N, 1)) + SDSS_SIGMA * rs.randn(N, B)
        Xe = np.tile(SDSS_SIGMA, (N, 1)); Xm = np.ones((N, B))
        mag = rs.uniform(19., 27., N)
        eng.upload_models(Y, Ye, Ym)
        eng.set_labels(model_z, np.full(M, 0.03), label_dict=pd)
        dX, dXe, dXm = (torch.from_numpy(a).to(dev) for a in (X, Xe, Xm))
        d_pdf = torch.empty((N, pd.Ngrid), dtype=torch.float64, device=dev)
        d_lm, d_le = (torch.empty(N, dtype=torch.float64, device=dev) for _ in range(2))
        eng.set_producer_stream(torch.cuda.current_stream().cuda_stream, 1)

        def timed(f):
            ts = []
            for _ in range(args.repeat):
                torch.cuda.synchronize(); eng.sync()
                t0 = time.perf_counter()
                r = f()
                torch.cuda.synchronize(); eng.sync()
                ts.append(time.perf_counter() - t0)
            return float(np.median(ts)), r

        priors.logprob_bpz(model_z[:8], model_type[:8], mag[:4])                # base table on the device, outside the timings
        t_build, hook = timed(lambda: priors.logprob_bpz(model_z, model_type, mag))
        lerp = hook.chunk(0, N, N)
        run = lambda pr: eng.fit_predict_prior(dX, dXe, dXm, opts, ko, pr, d_pdf, d_lm, d_le, n=N)
        run(lerp)                                                               # warm-up
        t_lerp, _ = timed(lambda: run(lerp))
        res = {'metric': 'bpz_prior_fit_predict', 'objects': N, 'models': M, 'bands': B, 'mode': 'B', 'table_build_s': t_build,
               'table_gb': 8e-9 * 1000 * M, 'lerp_s': t_lerp, 'lerp_pdfs_per_s': N / t_lerp, 'form': eng.last_form()}
        ref = d_pdf[:4096].clone()
        dense_gb = 8e-9 * N * M
        if dense_gb <= args.dense_max_gb:
            T = torch.empty((1000, M), dtype=torch.float64, device=dev)
            eng.lib.fz_dev_copy(eng.h, T.data_ptr(), hook.table.data_ptr(), T.numel() * 8); eng.sync()
            d_r, d_f = torch.from_numpy(hook.rows).to(dev), torch.from_numpy(hook.frac).to(dev)[:, None]

            def form():
                out = torch.empty((N, M), dtype=torch.float64, device=dev)
                step = max(1, (1 << 28) // M)
                for lo in range(0, N, step):
                    r, f = d_r[lo:lo + step], d_f[lo:lo + step]
                    out[lo:lo + step] = torch.log((1. - f) * T[r] + f * T[r + 1])
                return out
            form()
            t_form, dense = timed(form)
            dpr = logprob_prior(dense).chunk(0, N, N)
            run(dpr)
            t_dense, _ = timed(lambda: run(dpr))
            err = float((d_pdf[:4096] - ref).abs().max())
            res.update({'dense_gb': dense_gb, 'dense_form_s': t_form, 'dense_run_s': t_dense, 'dense_pdfs_per_s': N / (t_form + t_dense),
                        'speedup': (t_form + t_dense) / t_lerp, 'speedup_with_table_build': (t_form + t_dense) / (t_lerp + t_build),
                        'max_abs_pdf_difference': err})
            del dense, T
        else:
            res.update({'dense_gb': dense_gb, 'dense': 'skipped: above --dense-max-gb'})
        print(json.dumps(res), flush=True)
        del hook, lerp
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
