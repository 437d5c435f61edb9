"""G19: the reference's validation sums (plotting.py: input_vs_pdf, input_vs_dpdf, cdf_vs_epdf, cdf_vs_ecdf), recorded for
tests/test_diag_host.py and tests/test_hip_diag.py.  Run from the repository root with the reference importable (as make_golden.py
is); matplotlib draws into the Agg backend and every figure is thrown away:

    python tests/golden/make_golden_diag.py

Inputs, all stored as arrays (a regenerated exp could differ in its last bit and move an entry across a cut): a dictionary of 28
kernel widths on a 150-point grid, 256 PDFs on a 120-point grid (one or two Gaussians on a floor below the default cut), truths from
below the grid's first point to above its last (windows clipped at both ends), errors over the whole range of dictionary widths,
distinct random weights of which a few fall below the default weight cut.

The generator checks that the reference alone stays clear of every boundary a comparison could trip on: no CDF draw other than an
exact 0 or 1 lies within 1e-9 of a bin edge, and the kept set of no PDF changes when its cut value moves by one part in 1e12."""
import os
import sys
import warnings

os.environ.setdefault('MPLBACKEND', 'Agg')
import numpy as np  # noqa: E402

warnings.filterwarnings('ignore')
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ.get('FRANKENZ_REFERENCE', '/root/reference'))

from matplotlib import pyplot as plt  # noqa: E402
from frankenz import pdf as rpdf, plotting as rplot  # noqa: E402

NOBJ, NMC, NBINS, SEED = 256, 7, 20, 1234
HARSH = dict(pdf_wt_thresh=0.05, wt_thresh=0.2)
OBJ_CDF = dict(wt_thresh=None, cdf_thresh=0.05)
PDF_CDF = dict(pdf_wt_thresh=None, pdf_cdf_thresh=0.02)


def disp_scaled(pgrid, cent):
    return (pgrid - cent) / (1. + cent)


def cut_is_stable(rows, thresh):
    for p in rows:
        cut = max(p) * thresh
        a, b = p > cut * (1. - 1e-12), p > cut * (1. + 1e-12)
        if (a != b).any():
            return False
    return True


def main():
    rs = np.random.RandomState(19)
    xgrid = np.linspace(0., 3., 150)
    sgrid = np.linspace(0.01, 0.28, 28)
    vdict = rpdf.PDFDict(xgrid, sgrid)
    assert all(len(k) == 2 * w + 1 for k, w in zip(vdict.sigma_dict, vdict.sigma_width))
    pgrid = np.linspace(0., 3., 120)
    dgrid = np.linspace(-1., 1., 61)

    # PDFs: one or two Gaussians on a small floor, unit sum
    mu = rs.uniform(0.1, 2.9, NOBJ)
    sd = rs.uniform(0.03, 0.4, NOBJ)
    pdfs = np.exp(-0.5 * np.square((pgrid[None, :] - mu[:, None]) / sd[:, None]))
    two = rs.rand(NOBJ) < 0.4
    mu2, sd2, amp2 = rs.uniform(0.1, 2.9, NOBJ), rs.uniform(0.05, 0.3, NOBJ), rs.uniform(0.05, 0.8, NOBJ)
    pdfs += (two * amp2)[:, None] * np.exp(-0.5 * np.square((pgrid[None, :] - mu2[:, None]) / sd2[:, None]))
    pdfs += 1e-5 * rs.rand(NOBJ, len(pgrid))
    pdfs /= pdfs.sum(axis=1)[:, None]
    pdf_cent = (pdfs * pgrid).sum(axis=1)

    # truths beyond both ends of the grid, errors over all dictionary widths; an object off the grid gets an error wide enough
    # for its window to reach the grid (the reference fails otherwise)
    vals = rs.uniform(-0.25, 3.25, NOBJ)
    errs = rs.uniform(0.005, 0.3, NOBJ)
    off = np.maximum(np.maximum(-vals, vals - 3.), 0.)
    errs = np.maximum(errs, off / 5. + 0.03)
    cidx, eidx = vdict.fit(vals, errs)
    w = vdict.sigma_width[eidx]
    assert ((cidx + w >= 0) & (cidx - w <= vdict.Ngrid - 1)).all()
    assert (cidx - w < 0).sum() >= 10 and (cidx + w > vdict.Ngrid - 1).sum() >= 10 and (cidx < 0).any() and (cidx >= vdict.Ngrid).any()

    weights = rs.uniform(0.05, 1., NOBJ)
    weights[rs.choice(NOBJ, 12, replace=False)] = 1e-4 * rs.uniform(0.1, 1., 12)
    assert len(np.unique(weights)) == NOBJ and (weights < 1e-3 * weights.max()).sum() == 12

    def stack(fn, *a, **kw):
        s = fn(*a, **kw)
        plt.close('all')
        assert np.isfinite(s).all()
        return s

    base = (vals, errs, vdict, pdfs, pgrid)
    out = dict(xgrid=xgrid, sigma_grid=sgrid, delta=np.array(vdict.delta), dsigma=np.array(vdict.dsigma),
               sigma_width=np.asarray(vdict.sigma_width, dtype=np.int64), kern=np.concatenate(vdict.sigma_dict),
               kern_cdf=np.concatenate(vdict.sigma_dict_cdf), pgrid=pgrid, dgrid=dgrid, pdfs=pdfs, pdf_cent=pdf_cent, vals=vals,
               errs=errs, weights=weights, nmc=np.array(NMC), nbins=np.array(NBINS), seed=np.array(SEED),
               harsh=np.array([HARSH['pdf_wt_thresh'], HARSH['wt_thresh']]), obj_cdf_thresh=np.array(OBJ_CDF['cdf_thresh']),
               pdf_cdf_thresh=np.array(PDF_CDF['pdf_cdf_thresh']))
    out['stack_default'] = stack(rplot.input_vs_pdf, *base, weights=weights)
    out['stack_harsh'] = stack(rplot.input_vs_pdf, *base, weights=weights, **HARSH)
    out['stack_obj_cdf'] = stack(rplot.input_vs_pdf, *base, weights=weights, **OBJ_CDF)
    out['stack_pdf_cdf'] = stack(rplot.input_vs_pdf, *base, weights=weights, **PDF_CDF)
    out['dstack_default'] = stack(rplot.input_vs_dpdf, *base, pdf_cent, dgrid, weights=weights)
    out['dstack_scaled'] = stack(rplot.input_vs_dpdf, *base, pdf_cent, dgrid, weights=weights, disp_func=disp_scaled)

    # the PIT outputs, each from a fresh stream of the same seed, and the draws themselves by the reference's per-object calls
    out['epdf_n'] = rplot.cdf_vs_epdf(vals, errs, pdfs, pgrid, Nmc=NMC, weights=weights, Nbins=NBINS,
                                      rstate=np.random.RandomState(SEED))
    x, y = rplot.cdf_vs_ecdf(vals, errs, pdfs, pgrid, Nmc=NMC, rstate=np.random.RandomState(SEED))
    plt.close('all')
    out['ecdf_x'], out['ecdf_y'] = x, y
    st = np.random.RandomState(SEED)
    draws = np.zeros((NOBJ, NMC))
    for i in range(NOBJ):
        cdf = pdfs[i].cumsum()
        cdf /= cdf[-1]
        draws[i] = np.interp(st.normal(vals[i], errs[i], size=NMC), pgrid, cdf)
    out['draws'] = draws
    edges = np.linspace(0., 1., NBINS + 1)
    n, _ = np.histogram(draws.ravel(), bins=edges, weights=np.repeat(weights, NMC), density=True)
    assert np.array_equal(n, out['epdf_n'])                      # the recorded draws are the ones the reference binned
    first = (pdfs[:, 0] / pdfs.cumsum(axis=1)[:, -1])[:, None]
    assert (draws == first).any() and (draws == 1.).any()         # truths off both ends of the PDF grid clamp

    # the reference stays clear of the boundaries
    inner = draws[(draws != 0.) & (draws != 1.)]
    assert np.abs(inner[:, None] - edges[None, :]).min() > 1e-9
    for th in (1e-3, HARSH['pdf_wt_thresh']):
        assert cut_is_stable(pdfs, th)
    for disp in (lambda g, c: g - c, disp_scaled):
        rows = np.array([np.interp(dgrid, disp(pgrid, c), p) for p, c in zip(pdfs, pdf_cent)])
        assert cut_is_stable(rows, 1e-3)

    path = os.path.join(HERE, 'g19_diagnostics.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, size
    print('wrote %s (%d bytes)' % (path, size))


if __name__ == '__main__':
    main()
