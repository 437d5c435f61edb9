/*
 * frankenz_hip.h -- C ABI of libfrankenz_hip.so: the MI355X (gfx950) engine for
 * frankenz's brute-force photometric likelihood -> weighted Gaussian-KDE PDF path.
 *
 * This is the drop-in boundary.  The reference (joshspeagle/frankenz v0.3.5) is
 * pure Python/NumPy and has no FFI, so each entry point names the reference
 * function (file:line) whose arithmetic it replaces; INTEGRATION.md shows the
 * ctypes stub a frankenz maintainer would add.
 *
 * Conventions
 *  - every function returns 0 on success, <0 on error; the message is available
 *    from fz_last_error() (thread-local).
 *  - all floating-point data is float64, indices are int64, matrices are
 *    C-contiguous row-major exactly as the reference's NumPy arrays are.
 *  - every array pointer may be a HOST pointer or a DEVICE (hipMalloc'd) pointer;
 *    the library detects which (hipPointerGetAttributes) and stages host arrays
 *    through its own buffers.  Output pointers may be NULL = "not wanted".
 *  - masks are float64 0/1 (the reference's demos use np.ones_like(phot)).
 *  - STREAM ORDERING.  The library runs on a stream of its own.  By default an entry point
 *    that is handed device pointers first waits for ALL work queued on the device so far
 *    (hipDeviceSynchronize), so inputs produced by kernels on any caller stream are
 *    complete before they are read; and every entry point returns only when its own
 *    work has finished, so outputs may be consumed from any stream at once.  No
 *    caller-side synchronisation is needed on either side of a call.  A caller that
 *    overlaps the library with other device work (an RCCL all-gather of the previous
 *    block's rows in flight) names the stream its inputs are produced on instead --
 *    fz_set_producer_stream -- and the library waits for that stream alone.
 *  - one fz_ctx per device; a ctx is not thread-safe.
 */
#ifndef FRANKENZ_HIP_H
#define FRANKENZ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fz_ctx fz_ctx;

/* lprob_kwargs of frankenz.pdf.logprob / loglike (pdf.py:238-240, 326-328). */
typedef struct fz_like_opts {
    int32_t free_scale;       /* pdf.py:313  free_scale        (default 0) */
    int32_t ignore_model_err; /* pdf.py:76   ignore_model_err  (default 0) */
    int32_t dim_prior;        /* pdf.py:90   dim_prior         (default 1) */
    int32_t max_iter;         /* guard for the unbounded loop at pdf.py:199;
                                 <=0 means 10000.  Hitting it is an error.   */
    double  ltol;             /* pdf.py:199  ltol              (default 1e-4) */
    int32_t exact_evidence;   /* extension (no reference counterpart, default 0).  The default kernel of the fused
                                 path (k_hist, every form) forms and sums EVERY weight in fp64 -- the reference's
                                 logsumexp, bruteforce.py:619 -- and this flag changes nothing there.  It matters
                                 only to the older k_fused weight-space body, which serves what k_hist does not
                                 take (ln-prior tables, the direct grid KDE, many dictionary widths, wild values):
                                 0 = that body sums the weights BELOW wt_thresh of the best in fp32 (~1e-9
                                 relative on levid; lmap, PDFs and every stacked weight are fp64 either way),
                                 1 = its all-fp64 ln-space body.                                          */
    int32_t reserved_;        /* keep 0 */
} fz_like_opts;

/* kde_kwargs of gauss_kde / gauss_kde_dict (pdf.py:444-445, 529-531). */
typedef struct fz_kde_opts {
    double  wt_thresh;     /* relative-amplitude threshold (strict >), 1e-3     */
    int32_t use_wt_thresh; /* 1: wt_thresh rule (pdf.py:507-510 / 589-591).
                              0: the reference's CDF rule (wt_thresh=None,
                                 pdf.py:513-516 / 593-597) with cdf_thresh.
                              "no thresholding" is wt_thresh=-inf, use=1.       */
    int32_t normalize;     /* 1: pdf /= pdf.sum() (bruteforce.py:370, 629)      */
    double  cdf_thresh;    /* CDF rule: keep the ascending prefix with
                              cdf <= 1 - cdf_thresh (default 2e-4)              */
    int32_t exact_evidence;/* extension, default 0: as fz_like_opts.exact_evidence, for the calls that take
                              no likelihood options (predict from stored ln-weights): 1 = the whole
                              logsumexp in fp64; 0 = the weights below wt_thresh of the best in fp32  */
    int32_t reserved_;     /* keep 0 */
} fz_kde_opts;

/* accumulated device time per kernel family since fz_timing_reset (HIP events on
 * the context's own stream). */
typedef struct fz_timing {
    double  ms_planes;  int64_t n_planes;   /* materialising fit kernel       */
    double  ms_fused;   int64_t n_fused;    /* single-pass fit_predict kernel */
    double  ms_stats;   int64_t n_stats;    /* pass 1: max + logsumexp        */
    double  ms_kde;     int64_t n_kde;      /* pass 2: threshold + KDE stack  */
    double  ms_modec;   int64_t n_modec;    /* mode-C fixed-point iterations  */
    double  ms_knn;     int64_t n_knn;      /* brute-force top-k search       */
    double  ms_other;   int64_t n_other;    /* prep/clean/transposes          */
} fz_timing;

const char* fz_last_error(void);

/* Test / tuning switches.  The library does not read the environment: every switch that selects an alternative kernel form, a
 * launch geometry or a diagnostic (the "FZ_..." names listed in INTEGRATION.md section 5; none of them changes a result beyond
 * rounding) is set through this ONE call.  spec = "NAME=value;NAME=value;..." REPLACES the whole set (NULL or "": none set).
 * Process-wide; not to be called while another entry point runs.  The Python layer forwards the process's FZ_* environment
 * variables through it before each call (frankenz_amd/_lib.py), which is how the tests and tools/ set them. */
int  fz_debug_opts(const char* spec);
int  fz_device_count(void);

int  fz_ctx_create(int device, fz_ctx** out);
void fz_ctx_destroy(fz_ctx* ctx);
int  fz_sync(fz_ctx* ctx);
int  fz_timing_reset(fz_ctx* ctx);
int  fz_timing_get(fz_ctx* ctx, fz_timing* out);
/* which kernel form the last fused fit_predict / predict launch took ("k_hist<screen>", "k_hist<screen> (per-object band
 * counts)", "k_hist<exact>", "k_fused", "k_plane_rows", "k_plane_fused", "k_stats + k_kde", ...): the choice depends on the data (likelihood mode, masks, label errors, how broad the
 * likelihoods are), and a measurement should say what it measured.  No reference counterpart. */
const char* fz_last_form(fz_ctx* ctx);
/* byte budget for internal work space (candidate lists of the single-pass kernel, (N x M)
 * planes of mode C, host staging); default 45 % of the device memory, allocated on demand. */
int  fz_set_workspace_limit(fz_ctx* ctx, int64_t bytes);
/* the budget in force, in bytes, and the compute units of the context's device: the fused kernels choose their launch geometry and
 * between one pass and two from these (callers that change the budget put the value they found back); -1: NULL ctx */
int64_t fz_get_workspace_limit(fz_ctx* ctx);
int  fz_cu_count(fz_ctx* ctx);
/* Where device-resident INPUTS of the following calls come from (no reference counterpart: the reference has no device).
 * mode 0 (default): unknown -- every entry point handed device pointers drains the whole device first (hipDeviceSynchronize).
 * mode 1: they are produced by work queued on `stream` (a hipStream_t; NULL = the legacy default stream): the library records an
 *         event there and makes ITS stream wait for it -- no host wait, and work on other streams (a collective in flight) is
 *         not waited for.
 * mode 2: they are complete (the caller has synchronised): no wait at all.
 * Outputs are complete when a call returns in every mode. */
int  fz_set_producer_stream(fz_ctx* ctx, void* stream, int32_t mode);
/* page-locked host memory (hipHostMalloc) for results: device-to-host copies into it run at the link rate and overlap the next
 * chunk's kernel, which copies into pageable memory (np.zeros) do not.  The drop-in classes return their PDF arrays in it. */
int  fz_host_alloc(int64_t bytes, void** out);
int  fz_host_free(void* p);

/* BruteForce.__init__ (bruteforce.py:36-64): the model set (M,B) x3. */
int  fz_models_upload(fz_ctx* ctx, const double* models, const double* models_err,
                      const double* models_mask, int64_t M, int32_t B);

/* PDFDict tables (pdf.py:800-819): Ngrid, Ndict, sigma_width[D], ragged kernels
 * and their running sums flattened with offsets[D+1] (lengths are as built by
 * the reference, malformed entries included; they are rejected only if a label
 * maps onto one). */
int  fz_kdedict_upload(fz_ctx* ctx, int64_t G, int64_t D, const int64_t* widths,
                       const int64_t* offsets, const double* kern, const double* kcdf);

/* labels already mapped by PDFDict.fit (pdf.py:843-852) -> gauss_kde_dict path
 * (pdf.py:599-620).  Returns -3 (IndexError semantics) if a label's window lies
 * wholly off the grid, -4 (ValueError) if it maps onto a malformed entry. */
int  fz_labels_upload_dict(fz_ctx* ctx, const int64_t* y_idx, const int64_t* y_std_idx,
                           int64_t M);
/* raw labels for the direct gauss_kde path (pdf.py:489-502, 519-524). */
int  fz_labels_upload_grid(fz_ctx* ctx, const double* y, const double* y_std, int64_t M,
                           const double* grid, int64_t G, double dx, double sig_thresh);

/* pdf.loglike's in-place clean (pdf.py:309-311) over N objects: x, xe, xm (N,B)
 * are MODIFIED (host or device).  fz_fit / fz_fit_predict call it themselves. */
int  fz_clean(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N, int32_t B);

/* BruteForce._fit (bruteforce.py:127-205) with lprob_func = pdf.logprob
 * (pdf.py:326-411 -> _loglike pdf.py:27-100 / _loglike_s pdf.py:103-235).
 * Output planes are (N,M); any may be NULL.  x/xe/xm are cleaned in place. */
int  fz_fit(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
            const fz_like_opts* opts, double* lnlike, double* chi2, int64_t* ndim,
            double* scale, double* scale_err);

/* BruteForce._fit_predict with save_fits=False (bruteforce.py:505-631): never
 * materialises (N,M).  pdfs is (N,G); lmap/levid (N) may be NULL. */
int  fz_fit_predict(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                    const fz_like_opts* opts, const fz_kde_opts* kde,
                    double* pdfs, double* lmap, double* levid);

/* mode C (pdf.py:196-223) bookkeeping since the last fz_timing_reset, out4 = {objects whose stop decision fell within rounding
 * of ltol under the reciprocal-based solve and were re-run with IEEE divisions, iterations of the slowest object, 1 = one block
 * per object, one iteration per record read / 2 = state planes in HBM / 3 = one block per object, several iterations per record
 * read (k_modec_rounds; objects it hands back to the IEEE kernel are counted in the first entry too), threads per block of 1 / 3}; and the number of passes of the loop at pdf.py:199
 * each of the first n objects of the LAST mode-C chunk took (int32, host) -- the reference does not return it, the tests compare
 * it with their restated loop. */
int  fz_modec_info(fz_ctx* ctx, int64_t* out4);
int  fz_modec_niter(fz_ctx* ctx, int64_t n, int32_t* out);

/* ---- additive ln-prior (extension) ----
 * The reference's plug-in point is lprob_func, called once per object and returning
 * (lnprior, lnlike, lnprob = lnlike + lnprior, ...) (bruteforce.py:193-199; the BPZ
 * posterior of demos/2 cell 69 is the one use).  A Python callable cannot run on the
 * device, so the prior is passed as data: a (P,M) table of ln-prior rows over the M
 * models plus the row each object reads (e.g. P magnitude bins of P(z,t|m), or P = N
 * for a dense per-object prior, or P = 1 for one prior shared by all objects).
 * lnprob[i][j] = lnlike[i][j] + table[rows[i]][j].  -inf entries (prior 0) and nan
 * propagate as they do through the reference's lnlike + lnprior. */
typedef struct fz_prior {
    const double*  table;  /* (P,M) float64 row-major, host or device          */
    int64_t        P;      /* 1 <= P < 2^31                                     */
    const int64_t* rows;   /* (N) int64 in [0,P), host or device; NULL means
                              row 0 for everybody if P == 1, row i if P == N    */
} fz_prior;
/* fz_fit with the three probability planes of bruteforce.py:197-199 (prior may be
 * NULL: lnprior = 0, lnprob = lnlike, pdf.py:404-405). */
int  fz_fit_prior(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                  const fz_like_opts* opts, const fz_prior* prior, double* lnprior,
                  double* lnlike, double* lnprob, double* chi2, int64_t* ndim,
                  double* scale, double* scale_err);
/* fz_fit_predict weighting by lnprob = lnlike + lnprior (bruteforce.py:618-620). */
int  fz_fit_predict_prior(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                          const fz_like_opts* opts, const fz_kde_opts* kde,
                          const fz_prior* prior, double* pdfs, double* lmap, double* levid);

/* ---- interpolated prior (extension; docs/bpz_prior.md) ----
 * A prior that is linear along one per-object coordinate (the BPZ prior P(z, t | m) of the reference's priors.py along the
 * magnitude m): table holds prior VALUES, not logarithms, on P nodes of that coordinate, and object i reads the two rows
 * rows[i] and rows[i] + 1 with the weights 1 - frac[i] and frac[i]:
 *     lnprior[i][j] = ln((1 - frac[i]) * table[rows[i]][j] + frac[i] * table[rows[i] + 1][j]).
 * A zero value gives -inf, a negative or nan value nan.  rows outside [0, P - 2] or frac outside [0, 1] are refused (-7) before
 * any kernel reads the table.  frac == NULL makes every entry point below the fz_prior call of the same name (a table of ln rows). */
typedef struct fz_prior_lerp {
    const double*  table;  /* (P,M) float64 row-major, host or device          */
    int64_t        P;      /* 2 <= P < 2^31                                     */
    const int64_t* rows;   /* (N) int64 in [0,P-2], host or device              */
    const double*  frac;   /* (N) float64 in [0,1], host or device              */
} fz_prior_lerp;
int  fz_fit_prior_lerp(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                       const fz_like_opts* opts, const fz_prior_lerp* prior, double* lnprior,
                       double* lnlike, double* lnprob, double* chi2, int64_t* ndim,
                       double* scale, double* scale_err);
int  fz_fit_predict_prior_lerp(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                               const fz_like_opts* opts, const fz_kde_opts* kde,
                               const fz_prior_lerp* prior, double* pdfs, double* lmap, double* levid);
/* The table of such a prior for M models from a base table on a regular (coordinate, z, type) grid: base (P, NZ, NT) float64,
 * model j sits in z cell iz[j] in [0, NZ - 2] with the weight g[j] in [0, 1] of node iz[j] + 1 and has type t[j] in [0, NT):
 *     table[r][j] = (1 - g[j]) * base[r][iz[j]][t[j]] + g[j] * base[r][iz[j] + 1][t[j]].
 * base, iz, g, t: host or device; table (P, M): device memory.  Cells, types or weights out of range are refused (-7). */
int  fz_prior_rows_from_grid(fz_ctx* ctx, const double* base, int64_t P, int64_t NZ, int64_t NT, const int32_t* iz,
                             const double* g, const int32_t* t, int64_t M, double* table);

/* BruteForce._predict (bruteforce.py:303-372): rows of logwt (N,M) -> PDFs.
 * is_log=0 treats the rows as linear weights y_wt and skips the softmax
 * (gauss_kde / gauss_kde_dict called directly, pdf.py:444, 529). */
int  fz_predict_logwt(fz_ctx* ctx, const double* logwt, int64_t N, int32_t is_log,
                      const fz_kde_opts* kde, double* pdfs, double* lmap, double* levid);

/* ---- Monte-Carlo k-nearest-neighbour variant (knn.py) ---- */
/* K float32 feature sets (K,M,F) as fed to KDTree (knn.py:177-186). */
int  fz_knn_upload_trees(fz_ctx* ctx, const float* feats, int32_t K, int64_t M, int32_t F);
/* exact k-NN of N float64 queries (N,F) in each of the K sets under the Minkowski
 * norm lp_norm (1, 2 or inf): the flattened (N,K*k) table of knn.py:834-837;
 * entries at or beyond distance_upper_bound are M (KDTree's "missing" index). */
int  fz_knn_query(fz_ctx* ctx, const double* q, int64_t N, int32_t k, double lp_norm,
                  double distance_upper_bound, int64_t* idx);
/* knn.py:840-872: first-appearance de-dup of each row, likelihood on the subset,
 * weights, KDE.  Outputs padded like knn.py:812-821: neighbors (N,W) with -99,
 * nnbr (N), planes (N,W) with -inf/+inf/0/1 padding; any may be NULL. */
int  fz_knn_fit_predict(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                        const int64_t* idx, int64_t W, const fz_like_opts* opts,
                        const fz_kde_opts* kde, int64_t* neighbors, int64_t* nnbr,
                        double* lnlike, double* chi2, int64_t* ndim, double* scale,
                        double* scale_err, double* pdfs, double* lmap, double* levid);

/* the same with an additive ln-prior (see fz_prior): lnprior[i][s] = table[rows[i]][
 * neighbors[i][s]], lnprob = lnlike + lnprior, padded with -inf like knn.py:815-817;
 * PDFs are weighted by lnprob (knn.py:859-863).  prior may be NULL (lnprior = 0). */
int  fz_knn_fit_predict_prior(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                              const int64_t* idx, int64_t W, const fz_like_opts* opts,
                              const fz_kde_opts* kde, const fz_prior* prior, int64_t* neighbors,
                              int64_t* nnbr, double* lnprior, double* lnlike, double* lnprob,
                              double* chi2, int64_t* ndim, double* scale, double* scale_err,
                              double* pdfs, double* lmap, double* levid);

/* NearestNeighbors._fit_predict (knn.py:826-874) in one call: fz_knn_query + fz_knn_fit_predict_prior over chunks of <= 2^17
 * objects with the (N, K*k) neighbour table kept on the device (it only leaves through `neighbors`, if wanted).  q (N,F): the
 * objects' query features (knn.py:830-832), drawn by the caller so that the random stream is the reference's. */
int  fz_knn_search_fit_predict_prior(fz_ctx* ctx, const double* q, double* x, double* xe, double* xm, int64_t N,
                                     int32_t k, double lp_norm, double distance_upper_bound,
                                     const fz_like_opts* opts, const fz_kde_opts* kde, const fz_prior* prior,
                                     int64_t* neighbors, int64_t* nnbr, double* lnprior, double* lnlike,
                                     double* lnprob, double* chi2, int64_t* ndim, double* scale,
                                     double* scale_err, double* pdfs, double* lmap, double* levid);
/* the two calls above with an interpolated prior (fz_prior_lerp) */
int  fz_knn_fit_predict_prior_lerp(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N,
                                   const int64_t* idx, int64_t W, const fz_like_opts* opts,
                                   const fz_kde_opts* kde, const fz_prior_lerp* prior, int64_t* neighbors,
                                   int64_t* nnbr, double* lnprior, double* lnlike, double* lnprob,
                                   double* chi2, int64_t* ndim, double* scale, double* scale_err,
                                   double* pdfs, double* lmap, double* levid);
int  fz_knn_search_fit_predict_prior_lerp(fz_ctx* ctx, const double* q, double* x, double* xe, double* xm, int64_t N,
                                          int32_t k, double lp_norm, double distance_upper_bound,
                                          const fz_like_opts* opts, const fz_kde_opts* kde, const fz_prior_lerp* prior,
                                          int64_t* neighbors, int64_t* nnbr, double* lnprior, double* lnlike,
                                          double* lnprob, double* chi2, int64_t* ndim, double* scale,
                                          double* scale_err, double* pdfs, double* lmap, double* levid);

/* NearestNeighbors._predict (knn.py:488-558): PDFs from stored (N,W) ln-weights,
 * the stored neighbour table (N,W) and counts (N). */
int  fz_knn_predict_logwt(fz_ctx* ctx, const double* logwt, const int64_t* neighbors,
                          const int64_t* nnbr, int64_t N, int64_t W, const fz_kde_opts* kde,
                          double* pdfs, double* lmap, double* levid);

/* ---- consumers of the PDF stack ---- */
/* pdf.pdfs_summarize (pdf.py:899-1074).  pdfs (N,G) is renormalised IN PLACE when
 * renormalize != 0 (pdf.py:984-985).  urand (N): the rstate.rand() of each object
 * (pdf.py:1000), drawn by the caller so that the stream is the reference's.  loss
 * (G,G): 1 - kernel over (truth, guess) (pdf.py:1003-1024).  widths (N,4) or NULL:
 * the wconf_func windows around mean/median/mode/best; NULL means the default
 * (1 + point) * wconf_scale (pdf.py:1041-1043, 0.03).  stats (21,N) rows:
 * mean{value,std,conf,risk}, median{..}, mode{..}, best{..}, low95, low68, high68,
 * high95, Monte-Carlo draw -- the reference's return tuple flattened. */
int  fz_pdfs_summarize(fz_ctx* ctx, double* pdfs, int64_t N, int64_t G, const double* pgrid,
                       int32_t renormalize, const double* urand, const double* loss,
                       const double* widths, double wconf_scale, double* stats);
/* pdf.pdfs_resample (pdf.py:855-896): numpy.interp of every row of pdfs (N,G) from
 * old_grid onto new_grid (Gn points), `left` / `right` beyond the old grid's ends,
 * optional renormalisation to unit sum; out is (N,Gn). */
int  fz_pdfs_resample(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, const double* old_grid,
                      int64_t Gn, const double* new_grid, double left, double right,
                      int32_t renormalize, double* out);
/* samplers.loglike_nz (samplers.py:23-86) for finite non-negative nz: overlap (N) =
 * pdfs @ nz + pair_step * (pdfs[:,i] - pdfs[:,j]) (pair_i < 0: no pair), lnlike =
 * sum(log(overlap)). */
int  fz_overlap_nz(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, const double* nz,
                   int64_t pair_i, int64_t pair_j, double pair_step, double* overlap,
                   double* lnlike);

/* samplers.py:498-499, 519-520 -- the redshift-assignment step of the hierarchical / population
 * Gibbs samplers: one categorical draw per object from  pdfs[i] * nz / dot(pdfs[i], nz).  The
 * reference draws rstate.multinomial(1, ...) per object in a Python list comprehension and sums the
 * one-hot rows; here the draw is the inverse CDF of the caller's uniform u[i] in [0, 1)
 * (bin = number of grid points with running sum <= u[i] * total), so the caller keeps the random
 * stream.  bins (N, int64; -1 for a row without mass; may be NULL) and counts (G, int64: objects per
 * bin, i.e. the summed one-hot rows). */
int  fz_nz_assign(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, const double* nz, const double* u,
                  int64_t* bins, int64_t* counts);

/* ---- inference through a trained network (networks.py:244-356, 782-936, 1200-1473) ----
 * The network is DATA here (node positions in data space and, after populate_network, the per-node model lists); a SOM is
 * trained by fz_som_train (below).  Node ln-probabilities come from fz_fit with the (matched) nodes uploaded as noiseless, unmasked models
 * (networks.py:305-307, 874-876).  Every array may live in host or device memory.
 *
 * fz_net_select -- which nodes an object's (N, Nn) ln-probabilities select, in the reference's order (networks.py:885-896, 316-327):
 *   use_wt != 0: lnprob > ln(wt_thresh) + max(lnprob), strict, node index ascending.  wt_thresh == 0 is numpy's ln 0 = -inf: every
 *                node above -inf.  wt_thresh < 0 (the -inf a caller passes for "no threshold at all"): every node, -inf entries too.
 *   use_wt == 0: ascending ln-prob (ties by index), the prefix whose running probability exp(l - logsumexp) stays <= 1 - cdf_thresh.
 *   Special rows follow numpy: a row holding a nan selects nothing under either rule; under the CDF rule a row of nothing but -inf
 *   selects nothing and a row holding +inf selects its entries below +inf; under the weight rule a row holding +inf selects nothing
 *   (wt_thresh >= 0).  No node selected: nsel 0, rawlen 0, lmap = levid = -inf.
 *   match (Nn, or NULL = identity): the node behind column c (networks.py:873 match_sel); csr_off (Nnodes + 1, or NULL): offsets of
 *   the per-node lists.  Out: nsel (N) int32, sel (N, Nn) int32 column indices (first nsel[i] valid), rawlen (N) int64 summed
 *   list length of the selected nodes (NULL if not wanted), lmap / levid (N): max and logsumexp over the selected entries
 *   (networks.py:330-333; NULL if not wanted).  1 <= Nn <= 4096, refused beyond with the limit in the message (a wave per object,
 *   its row in LDS: four objects per block up to 2 560 nodes, two up to 4 096). */
int  fz_net_select(fz_ctx* ctx, const double* lnprob, int64_t N, int32_t Nn, int32_t use_wt, double wt_thresh,
                   double cdf_thresh, const int32_t* match, const int64_t* csr_off, int64_t Nnodes, int32_t* nsel,
                   int32_t* sel, int64_t* rawlen, double* lmap, double* levid);
/* networks.py:912-918: idx (N, W) = the lists (csr_items, int64 model indices) of every object's selected nodes concatenated in
 * order, padded to W with the row's first entry -- the table fz_knn_fit_predict takes: it removes repeats in first-appearance
 * order, which is pandas.unique (networks.py:919), and fits the remaining models (networks.py:925-928).  A row longer than W is cut
 * at W; a row of no entry at all (nsel 0, or only empty lists) is W times index 0: the caller must not fit it. */
int  fz_net_table(fz_ctx* ctx, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn, const int32_t* match,
                  const int64_t* csr_off, const int64_t* csr_items, int64_t Nnodes, int64_t W, int64_t* idx);
/* The union of the selected nodes' lists with repeats removed (extension: Network.fit_sparse; docs/network.md, "Sparse rows").
 * U_i = the set of model indices in the lists of object i's selected nodes: the node is nd = match ? match[sel[i][s]] : sel[i][s] for
 * s < nsel[i], its list csr_items[csr_off[nd] .. csr_off[nd + 1]).  nuniq[i] = |U_i|, the full count in either form of the call.
 * idx != NULL: row i of idx (N, W) holds the elements of U_i in ascending order, cut at W, padded to W with its own first (smallest)
 * element -- the table fz_knn_fit_predict takes: its first-appearance de-duplication then leaves the ascending order.  An empty union
 * gives nuniq 0 and W times index 0, as fz_net_table does: the caller must not fit such a row.  idx == NULL is the counting call
 * (W is not looked at).  An index outside [0, M) in a list that a selected node reaches returns -3; it is found before any row of
 * idx is written (a bad index in a list no object selects is not an error).  M > FZ_NET_UNION_MMAX = 2^20 is refused with -5: a wave
 * per object keeps a bitmap of M bits in LDS, four objects per block up to 327 680 models, two up to 655 360, one beyond.  Every
 * array may live in host or device memory. */
#define FZ_NET_UNION_MMAX (1 << 20)
int  fz_net_union(fz_ctx* ctx, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn, const int32_t* match,
                  const int64_t* csr_off, const int64_t* csr_items, int64_t Nnodes, int64_t M, int64_t W, int64_t* nuniq,
                  int64_t* idx);
/* networks.py:907-909 (nodes_only): out (N, W) 8-byte elements = plane (N, Nn) at the selected columns, `pad_bits` beyond nsel. */
int  fz_net_gather(fz_ctx* ctx, const void* plane, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn, int32_t W,
                   uint64_t pad_bits, void* out);
/* networks.py:1459-1466, 1473 (nodes_only): pdfs (N, G) = softmax over the selected ln-probabilities @ node_pdfs (Nnodes, G) rows of
 * the selected nodes, each row divided by its sum; lmap / levid (N) over the selected entries. */
int  fz_net_stack(fz_ctx* ctx, const double* lnprob, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn,
                  const int32_t* match, const double* node_pdfs, int64_t Nnodes, int64_t G, double* pdfs, double* lmap,
                  double* levid);

/* ---- training of a self-organizing map (networks.py:1517-1867, SelfOrganizingMap.train_network) ----
 * fz_som_train -- steps [s0, s1) of the sequential training loop, run by ONE persistent workgroup (docs/som.md).  Step i draws
 * row draws[i] of the CLEANED models (M, B) / models_err / models_mask (pdf.py:309-311 applied by the caller), takes its
 * ln-probability against every node as a noiseless, unmasked model with the likelihood options *opts (free_scale, ignore_model_err,
 * dim_prior), rescales every node by its best-fit scale if track_scale (needs free_scale; networks.py:1838-1840), takes the
 * best-matching unit (np.argmax order: first maximum, first nan) into bmus[i], weighs every node by its squared grid distance d to
 * it (nodes_pos (NNODE, NPROJ) int32; neighbor_kind 0: exp(-0.5 d / sigma[i]^2), 1: sigma[i]^2 / (d + sigma[i]^2)), selects the
 * nodes (use_wt != 0: w > wt_thresh * max(w); use_wt == 0: the ascending-weight prefix whose running probability stays
 * <= 1 - cdf_thresh, ties split in node-index order) and moves them: nodes[n] += learn_rate[i] * w[n] * (models[row] - nodes[n])
 * over all B bands.  nodes (NNODE, B) is read and written; draws / learn_rate / sigma / bmus have T entries.  Calling with
 * consecutive ranges gives bit-identical nodes to one call over their union.  B <= 32, NPROJ <= 8, NNODE <= 4194304. */
int  fz_som_train(fz_ctx* ctx, const double* models, const double* models_err, const double* models_mask, int64_t M, int32_t B,
                  double* nodes, const int32_t* nodes_pos, int32_t NNODE, int32_t NPROJ, const int64_t* draws,
                  const double* learn_rate, const double* sigma, int64_t T, int32_t neighbor_kind, int32_t use_wt,
                  double wt_thresh, double cdf_thresh, const fz_like_opts* opts, int32_t track_scale, int64_t s0, int64_t s1,
                  int32_t* bmus);

/* ---- training of a growing neural gas (networks.py:1870-2260, GrowingNeuralGas.train_network) ----
 * fz_gng_train -- steps [s0, s1) of the sequential training loop, batch ends included, run by ONE persistent workgroup
 * (docs/gng.md).  Step i draws row draws[i] of the CLEANED models (as fz_som_train), takes its ln-probability against every live node,
 * writes the label of the best node to bmus[i] (heapq.nlargest order: ties to the earlier node, nan ln-probs lowest), moves it by
 * learn_best and its graph neighbours by learn_neighbor towards the row, adds the step's chi2 to its error, resets or creates the edge
 * to the second-best node, ages the best node's edges and lists those whose age equals max_age.  Every step i with i % nbatch == 0
 * ends a batch: batch[2 k + 1] (k = i / nbatch) = the number of listed edges; listed edges and nodes left without edges are removed;
 * if fewer than max_nodes nodes live, a node labelled nnode_init + k is inserted between the node of the largest error and that
 * node's neighbour of the largest error (both errors *= new_err_keep); batch[2 k] = live nodes.  Then every error *= all_err_keep.
 * The network is the caller's state, read and written, in slot order = the reference's node order:
 *   fstate  doubles: pos[cap * B] | fit[cap * B] (the rescaled copy of track_scale) | err[cap] | alias_rows[2 * B]
 *   istate  int32:   counters[16] = {live nodes, prune entries, edge ids handed out, status, step of the status, slot of the node that
 *                    is model row alias0 (-1: removed), the same for alias1, current adjacency buffer (0 / 1), 0...} |
 *                    degree[cap] | aux[cap] (zero) | adjacency[2][cap * max_degree] pairs (neighbour slot, edge id), neighbour order |
 *                    prune list[prune_cap] triples | age[edge_cap] by edge id
 *   ids     int64[cap]: node labels.
 * alias0 / alias1 (-1: none): model rows that ARE the positions of two nodes (the reference's initial nodes are views of the caller's
 * rows): a draw of such a row reads the node's current position; alias_rows holds what the two rows hold after the call.
 * Calling with consecutive ranges gives bit-identical state to one call over their union.  A node that would get more than
 * max_degree neighbours stops the run: the call fails and names the limit.  B <= 32, cap <= FZ_GNG_MAX_NODES, 2 <= max_degree <= 64,
 * T < 2^30; edge_cap >= initial edges + T + 2 * batch ends. */
#define FZ_GNG_MAX_NODES 65536
int  fz_gng_train(fz_ctx* ctx, const double* models, const double* models_err, const double* models_mask, int64_t M, int32_t B,
                  const int64_t* draws, int64_t T, double* fstate, int32_t* istate, int64_t* ids, int32_t cap, int32_t max_degree,
                  int32_t prune_cap, int32_t edge_cap, int32_t nbatch, int32_t max_age, int32_t max_nodes, int64_t nnode_init,
                  double learn_best, double learn_neighbor, double new_err_keep, double all_err_keep, const fz_like_opts* opts,
                  int32_t track_scale, int64_t alias0, int64_t alias1, int64_t s0, int64_t s1, int64_t* bmus, int32_t* batch);

/* ---- device memory that outlives a call (the samplers' resident PDF stack and per-object state) ----
 * fz_dev_alloc / fz_dev_free: plain device allocations on the context's GPU.  fz_dev_copy: `bytes` from src to dst, either side in
 * host or device memory, complete on return. */
int  fz_dev_alloc(fz_ctx* ctx, int64_t bytes, void** out);
int  fz_dev_free(fz_ctx* ctx, void* p);
int  fz_dev_copy(fz_ctx* ctx, void* dst, const void* src, int64_t bytes);

/* ---- the n(z) samplers (samplers.py:83-535: population_sampler, hierarchical_sampler; docs/samplers.md) ----
 * fz_pdfs_colsum -- colsum (G) = pdfs.sum(axis=0) in a fixed order (blocks of 512 rows added in row order, then the blocks in
 * order): the stacked n(z), and with it the samplers' default start  colsum / sum(colsum). */
int  fz_pdfs_colsum(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, double* colsum);
/* fz_nz_pairs -- saved samples [s0, s1) of population_sampler.sample (samplers.py:262-308) with a flat prior, `thin` pairs per
 * sample and mh_steps proposals per pair, without a host synchronisation in between.  pdfs (N, G), overlap (N) = pdfs @ pos and the
 * scratch column dcol (N) must be DEVICE arrays; pos (G) and lnpost (1) are read and written; pairs (nsamp * thin, 2) int64,
 * normals and expo (nsamp * thin, mh_steps) are the reference's random stream drawn ahead (rstate.choice(G, 2, replace=False) per
 * pair at the start of each sample, then per proposal randn() and exponential()).  Per pair (i, j), d = pdfs[:, i] - pdfs[:, j]:
 * scale = 1e-4 min(pos[i], pos[j], 1 - pos[i], 1 - pos[j]); grad = (sum log(overlap + scale/2 d) - sum log(overlap - scale/2 d)) /
 * scale; gscale = min(|1 / grad|, |scale 1e4|) (|scale| if grad == 0); per proposal z = normal * gscale, rejected without an
 * evaluation if pos[i] + z or pos[j] - z is negative or not finite, accepted if -expo < sum log(overlap + z d) - lnpost, and then
 * overlap += z d, pos[i] += z, pos[j] -= z.  Every sum is formed in one fixed order (blocks of 1024 objects, then the block sums in
 * index order): a chain is reproducible bit for bit, also when cut into segments.  Out: samples (nsamp, G), samples_lnp (nsamp) rows
 * [s0, s1); accept (nsamp * thin, mh_steps) int32 and gscale (nsamp * thin) of the segment's pairs. */
int  fz_nz_pairs(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, double* pos, double* overlap, double* dcol, double* lnpost,
                 const int64_t* pairs, const double* normals, const double* expo, int64_t nsamp, int32_t thin, int32_t mh_steps,
                 int64_t s0, int64_t s1, double* samples, double* samples_lnp, int32_t* accept, double* gscale);
/* fz_nz_pair_eval -- one evaluation of the same chain with the decision left to the host (a user's ln-prior is a Python callable).
 * An accepted step is handed back as (has_pend, pend_step) and applied to overlap (with the column in dcol) before anything else.
 * what 0: gather dcol for the new pair (pair_i, pair_j), sums[0], sums[1] = sum log(overlap +- step * dcol); what 1: sums[0] =
 * sum log(overlap + step * dcol); what 2: the pending step only.  sums is a host array of two doubles. */
int  fz_nz_pair_eval(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, double* overlap, double* dcol, int32_t what,
                     int64_t pair_i, int64_t pair_j, int32_t has_pend, double pend_step, double step, double* sums);
/* fz_nz_sweep -- the assignment step of one Gibbs sweep of hierarchical_sampler (samplers.py:498-499, 519-520): fz_nz_assign's draw
 * and counts (G, int64) without the per-object bins; a row without mass under nz is left out of the counts.  use_philox == 0: the
 * uniforms u (N) of the caller.  use_philox != 0: object i draws the uniform of Philox4x32-10 under the key (key0, key1) at the
 * counter (i lo, i hi, sweep lo, sweep hi), made of the first two output words a, b as ((a >> 5) 2^26 + (b >> 6)) / 2^53
 * (samplers._philox_uniform is the NumPy twin). */
int  fz_nz_sweep(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, const double* nz, const double* u, int32_t use_philox,
                 uint32_t key0, uint32_t key1, uint64_t sweep, int64_t* counts);

/* ---- validation of a PDF stack against known values (the arithmetic of plotting.py; docs/diagnostics.md) ----
 * fz_stack2d -- plotting.input_vs_pdf / input_vs_dpdf (plotting.py:127-159, 309-344): stack (Gx, Gy) = sum over the nsel selected
 * objects of  kern_e[x - (c - w)] q[y] w_eff / sum(kern on the grid) / sum(q[keep]),  Gx and the kernels being those of the
 * dictionary last uploaded (fz_kdedict_upload).  pdfs (Nrows, Gy) lives in host or device memory (host rows are staged in chunks).
 * The per-object arrays are HOST arrays of nsel entries in ascending order of cent: rows (the object's row of pdfs), cent (grid
 * index of its centre), eidx (its dictionary entry), weff (its weight).  prepared == 0: keep = p > max(p) * pdf_thresh (strict),
 * q = p / sum(p[keep]) (pdf_thresh = -inf keeps everything); prepared != 0: the rows are already cut and divided, every entry
 * counts as it stands.  A row without mass adds nothing.  full_range != 0: every x tile visits every object (measurements only).
 * accumulate != 0: the result is added to what stack holds.  No floating-point atomics: two calls give the same bits.
 * Refused with the row in the message (-4): a malformed dictionary entry (taps != 2 w + 1), a window [c - w, c + w] that does
 * not meet [0, Gx), a value of a selected row that is not finite. */
int  fz_stack2d(fz_ctx* ctx, const double* pdfs, int64_t Nrows, int64_t Gy, int64_t nsel, const int64_t* rows,
                const int64_t* cent, const int64_t* eidx, const double* weff, double pdf_thresh, int32_t prepared,
                int32_t full_range, int32_t accumulate, double* stack);
/* plotting.py:319-320: out (N, Gd) row i = np.interp(dgrid, xp, pdfs[i]) with xp = pgrid - cent[i] (disp 0) or
 * (pgrid - cent[i]) / (1 + cent[i]) (disp 1); beyond the ends of xp the end values. */
int  fz_recentre_rows(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, const double* pgrid, const double* cent,
                      int32_t disp, int64_t Gd, const double* dgrid, double* out);
/* plotting.py:427-436, 501-505: per object cdf = cumsum(pdfs[i]) / cumsum(pdfs[i])[-1]; draws (N, Nmc) =
 * np.interp(mc[i], grid, cdf) for the caller's Monte-Carlo truths mc (N, Nmc); hist (Nbins) = the draws' histogram over
 * edges (Nbins + 1, ascending), draw (i, m) weighing weights[i]: bin j holds edges[j] <= u < edges[j + 1], the last bin closed
 * (np.histogram), summed in a fixed order.  draws or hist may be NULL (then weights / edges are not read).  2 <= G <= 19200. */
int  fz_cdf_draws(fz_ctx* ctx, const double* pdfs, int64_t N, int64_t G, const double* grid, const double* mc, int64_t Nmc,
                  const double* weights, const double* edges, int64_t Nbins, double* draws, double* hist);

/* ---- synthetic photometry (simulate.py:811-840, 986-1014 with the Madau IGM of reddening.py:23-95; docs/simulate.md) ----
 * fz_synphot_upload -- the filter curves and templates of a survey, once.  HOST arrays.  Filters: foff (Nf + 1) offsets into the
 * concatenated per-point arrays fwave (the wavelength as the reference forms it, exp(log(wavelength))), flw (ln wavelength), fwt (the
 * trapezoid weight of the point over frequency, transmission / nu included, divided by the filter's norm) and ftab (points, 18):
 * columns 0..11 the running sums P[j] of the first j Lyman-line terms coeff_i (wave / l_i)^3.46 in the reference's order (P[0] = 0),
 * columns 12..17 (wave / 912)^{3, 0.46, 1.5, 0.18, -1.32, 1.68}.  Templates: toff (Nt + 1) offsets into tlw (ln wavelength) and
 * tasinh (arcsinh of f_nu).  Refused (-4): a filter or template of fewer than 2 points, a wavelength that is not positive and
 * finite, template wavelengths that decrease (repeated filter wavelengths are allowed).
 * fz_synphot -- out (Npair, Nf)[p][f] = sum_k fwt_k sinh(np.interp(flw_k - ln1pz_p, tlw, tasinh)) exp(-tau(fwave_k, z_p)) over the
 * points k of filter f and the template tmpl[p]; igm 0: tau = 0, 1: Madau (tau1 + max(tau2, 0), strict wave < l (1 + z)).  tmpl, z
 * and ln1pz = log(1 + z) are HOST arrays of Npair entries; out lives in host or device memory.  One wave per (pair, filter) and a
 * fixed-order reduction, no floating-point atomics: two calls give the same bits, and a pair's result does not depend on the other
 * pairs of the call.  Refused before anything is written: a template index out of range (-3), 1 + z negative or not finite (-4). */
int  fz_synphot_upload(fz_ctx* ctx, int64_t Nf, const int64_t* foff, const double* fwave, const double* flw, const double* fwt,
                       const double* ftab, int64_t Nt, const int64_t* toff, const double* tlw, const double* tasinh);
int  fz_synphot(fz_ctx* ctx, int64_t Npair, const int64_t* tmpl, const double* z, const double* ln1pz, int32_t igm, double* out);

/* ---- posterior draws over the model set (extension, no reference counterpart; docs/draws.md) ----
 * For a row r[0..L) of ln-weights: w_j = exp(r_j - max r), cdf_j = w_0 + ... + w_j, tot = cdf_{L-1}; a draw with uniform u in [0, 1] is
 * j = #{k : cdf_k <= u tot}, clipped to the last entry with w_j > 0 (the rule of fz_nz_assign).  A row that holds a nan, or whose max
 * is not finite, gives -1 for every draw.  lmap / levid: the row's max and logsumexp (fp64).  The sums are formed in a fixed,
 * segmented order (docs/draws.md): a draw is a function of (row, u) alone -- the same bits whatever the chunking (workspace limit),
 * the object order, the number of objects in a call and the memory the arguments live in.
 * Uniforms: u (N, S) from the caller, each checked to lie in [0, 1] before anything is drawn (-4); or u == NULL: Philox4x32-10 under
 * (key0, key1) at the counter (first + i, s) for draw s of object i, the double formed as fz_nz_sweep forms it (`first`: the index of
 * object 0 in the caller's whole array, so that a caller who splits a call gets the same draws).
 * Limits (-5, before any launch): 1 <= S <= 65536 (FZ_DRAW_SMAX), rows of at most 2^20 entries (FZ_DRAW_LMAX); S < 1 is -4.
 *
 * fz_draw_logwt -- logwt (N, W) rows; neighbors (N, W) / nnbr (N) both NULL, or both given: only the first nnbr[i] entries of row i
 *   count and the value returned for entry j is neighbors[i][j] (nnbr[i] outside [0, W]: -3).  idx (N, S) int64; lmap, levid (N) or NULL.
 * fz_fit_draw -- objects -> draws with the built-in likelihood (every mode) and an optional ln-prior (prior->frac == NULL: a plain
 *   ln table, else the interpolated form): per chunk the ln-likelihood plane of fz_fit (mode C: its final plane), + the prior, drawn
 *   from in place; chunks sized from the workspace limit.  x, xe, xm are cleaned in place like fz_fit.
 * fz_knn_search_fit_draw -- fz_knn_search_fit_predict_prior_lerp without the KDE half: the K searches, the subset likelihood (+ prior),
 *   then draws from each object's padded ln-prob row; the values drawn are MODEL indices.  neighbors (N, K k) / nnbr (N): optional
 *   outputs, as there. */
int  fz_draw_logwt(fz_ctx* ctx, const double* logwt, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr,
                   const double* u, uint32_t key0, uint32_t key1, int64_t first, int64_t S, int64_t* idx, double* lmap,
                   double* levid);
int  fz_fit_draw(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N, const fz_like_opts* opts, const fz_prior_lerp* prior,
                 const double* u, uint32_t key0, uint32_t key1, int64_t first, int64_t S, int64_t* idx, double* lmap,
                 double* levid);
int  fz_knn_search_fit_draw(fz_ctx* ctx, const double* q, double* x, double* xe, double* xm, int64_t N, int32_t k, double lp_norm,
                            double distance_upper_bound, const fz_like_opts* opts, const fz_prior_lerp* prior, const double* u,
                            uint32_t key0, uint32_t key1, int64_t first, int64_t S, int64_t* neighbors, int64_t* nnbr, int64_t* idx,
                            double* lmap, double* levid);

/* ---- hierarchical re-weighting of the training set: Gibbs over model weights (extension; docs/model_weights.md) ----
 * The law of the reference's hierarchical_sampler (samplers.py:311-535) with the M training objects in the place of the label grid.
 * One sweep: per object the row t_ij = rows_ij + lnw[nbr_ij] (one fp64 add; dense rows: nbr_ij = j, W == M) and ONE posterior draw
 * from it, exactly the draw of fz_draw_logwt on that row; counts_j = objects assigned to j; a row without a posterior (a nan, a max
 * that is not finite -- all its neighbours at weight 0 included --, nnbr[i] == 0) is left out of the counts and gets assign = -1.
 * Then g_j ~ Gamma(alpha_j + counts_j, 1), pos = g / sum(g), lnw = log(g) - log(sum(g)) (g_j = 0: lnw_j = -inf).
 * Random numbers: Philox4x32-10.  The sweep's uniform of object i is the one of fz_nz_sweep under (key0, key1) at the counter
 * (first + i, sweep).  The gamma draws use the key (key0, key1 ^ 0x6D775F67) and the counter (j, slot, sweep lo, sweep hi): slot 2a
 * the normal of attempt a (Box-Muller of the two doubles of the four words), slot 2a + 1 its acceptance uniform, slot 128 the
 * uniform of the shape + 1 boost (Marsaglia-Tsang; at most 64 attempts, else -7).  The sum of g is formed in one fixed order.
 * Refusals: W > 2^20 (FZ_DRAW_LMAX) or M >= 2^31 (FZ_MW_MMAX): -5 before any launch; a neighbour index outside [0, M) within
 * nnbr[i], or nnbr[i] outside [0, W]: -3 (the index is not used to read anything; counts are then not to be used); alpha_j <= 0 or
 * not finite: -4; a caller's uniform outside [0, 1]: -4.
 *
 * fz_mw_sweep -- one sweep's assignments.  rows (N, W), neighbors (N, W) / nnbr (N) (both NULL: dense), u (N) or NULL (Philox),
 *   assign (N) or NULL: host or device, staged in chunks from the workspace limit; lnw (M), counts (M, int64; zeroed by the call).
 * fz_mw_dirichlet -- the weights' step: alpha (M), counts (M) -> pos (M), lnw (M); host or device.
 * fz_mw_chain -- nsweeps sweeps (numbers sweep0, sweep0 + 1, ...) back to back without a host synchronisation inside; rows, neighbors
 *   and nnbr must be device arrays.  lnw (M) in and out; counts (M) and pos (M) of the last sweep; counts_all (nsweeps, M) or NULL:
 *   the counts of every sweep.  Bit for bit nsweeps calls of fz_mw_sweep (u == NULL) + fz_mw_dirichlet. */
int  fz_mw_sweep(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                 const double* lnw, const double* u, uint32_t key0, uint32_t key1, int64_t first, uint64_t sweep, int64_t* counts,
                 int64_t* assign);
int  fz_mw_dirichlet(fz_ctx* ctx, const double* alpha, const int64_t* counts, int64_t M, uint32_t key0, uint32_t key1, uint64_t sweep,
                     double* pos, double* lnw);
int  fz_mw_chain(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                 const double* alpha, double* lnw, uint32_t key0, uint32_t key1, int64_t first, uint64_t sweep0, int32_t nsweeps,
                 int64_t* counts, double* pos, int64_t* counts_all);

/* ---- EM over the model weights: point estimate and marginal ln-likelihood (extension; docs/model_weights.md, "EM") ----
 * The expectation form of the sweep above, i.e. of the reference's hierarchical_sampler (samplers.py:311-535) over the model set:
 * where fz_mw_sweep draws j_i ~ exp(rows_ij) w_j and counts, an iteration adds every entry's responsibility.  From lnw:
 *   ell_i = logsumexp_k (rows_ik + lnw[nbr_ik]) over the counted entries, bit for bit the levid of fz_draw_logwt on the pre-added row;
 *           a row without a posterior (the sweep's rule) is skipped: ell_i = nan, it adds to nothing and is counted in nskip.
 *   lnpost = sum_i ell_i (block partials in index order) + sum_{j: alpha_j != 1} (alpha_j - 1) lnw_j
 *   c_j    = sum over the counted entries with nbr_ik = j of exp((rows_ik + lnw_j) - ell_i), column j of the inverted index in
 *           segments of 1024 entries (FZ_MW_EM_CSEG; dense rows: strips of 1024 objects), segment sums added in order
 *   a_j    = c_j + (alpha_j - 1);  pos = a / sum(a);  lnw = log(a) - log(sum(a))      (sum(a) in the order of fz_mw_dirichlet's sum)
 * No float atomics: every result is a function of its inputs alone.  Refusals: those of fz_mw_sweep; N >= 2^31 (FZ_MW_EM_NMAX): -5;
 * alpha_j < 1 or not finite: -4 (no maximum); sum(a) == 0 (every object skipped at alpha == 1): -7.
 *
 * fz_mw_em_index_bytes -- nnbr (N), host or device (NULL: dense rows, no index): entries = sum(nnbr), bytes = what col_off (M + 1)
 *   int64, col_obj (entries) int32 and col_val (entries) float64 need together.  The caller allocates.
 * fz_mw_em_index -- device-resident rows, neighbors, nnbr -> the inverted index: column j's slice [col_off[j], col_off[j + 1]) lists the
 *   counted entries with neighbour j in ascending (i, k) order, the object index and a copy of the row value (a stable LSD counting
 *   sort by model index).  A bad table is refused (-3) before anything is gathered.
 * fz_mw_loglike -- rows, neighbors, nnbr host or device (staged in chunks from the workspace limit as fz_mw_sweep), lnw (M) ->
 *   ell (N) or NULL, lnlike (one double: sum of ell), nskip (one int64).  Needs no index; the same bits whatever the chunking.
 * fz_mw_em -- niter iterations back to back without a host synchronisation inside, on device-resident rows and index (dense rows:
 *   col_* NULL, entries 0).  lnw (M) in and out; pos (M) and counts (M, float64: c) of the last iteration; trace (niter): lnpost of
 *   the weights going INTO each iteration; nskip (niter).  Bit for bit niter calls with niter = 1. */
int  fz_mw_em_index_bytes(fz_ctx* ctx, int64_t N, int64_t W, const int64_t* nnbr, int64_t M, int64_t* entries, int64_t* bytes);
int  fz_mw_em_index(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                    int64_t entries, int64_t* col_off, int32_t* col_obj, double* col_val);
int  fz_mw_loglike(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                   const double* lnw, double* ell, double* lnlike, int64_t* nskip);
int  fz_mw_em(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
              const int64_t* col_off, const int32_t* col_obj, const double* col_val, int64_t entries, const double* alpha, double* lnw,
              int32_t niter, double* pos, double* counts, double* trace, int64_t* nskip);

/* ---- sparse rows out of an exhaustive fit (extension, no reference counterpart; docs/sparse_fits.md) ----
 * For a row r[0..L) of ln-weights, a cap W >= 1 and a cut lncut < 0 (-inf allowed): a nan among the entries, or a max that is not
 * finite, keeps nothing (Nneighbors = 0).  Else m = max r, entry j is eligible iff r_j - m > lncut (one IEEE subtraction, strict), and
 * kept are the first min(W, E) eligible entries in the order (value descending, index ascending; compared as doubles), stored in that
 * order: column 0 is the MAP model, and the result for W' < W is the first W' columns of the result for W.  Layout of the k-NN
 * fitter: neighbors (N, W) int64 padded with -99, nnbr (N) int64, rows (N, W) padded like NearestNeighbors' (lnprior, lnlike, lnprob
 * -inf; chi2 +inf; Ndim 0; scale 1; scale_err 0).  lmap / levid: of the FULL row, bit for bit those of fz_draw_logwt; lnkept: the
 * logsumexp of the kept entries (-inf when nothing is kept).  The result is a function of (row, W, lncut) alone.
 * Refusals, before any launch: W > 4096 (FZ_SPARSE_WMAX) or rows longer than 2^20 (FZ_DRAW_LMAX): -5; W < 1, lncut >= 0 or nan: -4.
 *
 * fz_sparsify_logwt -- extension, no reference counterpart.  logwt (N, M) rows, host or device, staged in chunks from the workspace
 *   limit; neighbors (N, W), nnbr (N) required; vals (N, W), lmap, levid, lnkept (N) or NULL.
 * fz_fit_sparse -- extension, no reference counterpart.  Objects -> sparse rows with the built-in likelihood (every mode) and an
 *   optional ln-prior (as fz_fit_draw): per chunk the planes of fz_fit that are asked for, the selection on the ln-prob plane and a
 *   gather per other plane; chunks sized from the workspace limit by the number of planes formed.  Every per-pair output may be NULL;
 *   a kept entry of one is the plane's value at (i, neighbors[i][t]), bit for bit.  x, xe, xm are cleaned in place like fz_fit. */
int  fz_sparsify_logwt(fz_ctx* ctx, const double* logwt, int64_t N, int64_t M, int64_t W, double lncut, int64_t* neighbors, int64_t* nnbr,
                       double* vals, double* lmap, double* levid, double* lnkept);
int  fz_fit_sparse(fz_ctx* ctx, double* x, double* xe, double* xm, int64_t N, const fz_like_opts* opts, const fz_prior_lerp* prior, int64_t W,
                   double lncut, int64_t* neighbors, int64_t* nnbr, double* lnprior, double* lnlike, double* lnprob, double* chi2,
                   int64_t* ndim, double* scale, double* scale_err, double* lmap, double* levid, double* lnkept);

/* ---- posterior moments of per-model values, and the zero-point sums (extension, no reference counterpart; docs/predictive.md) ----
 * The law.  A row r[0..n) of ln-weights with model indices j_t (dense rows: j_t = t, n = M), optional scales s_t (absent: 1), a value
 * table V (M, L), an optional error table Ve (M, L) and an optional mask table Vm (M, L; non-zero: usable).  A nan among the counted
 * entries, or a max m that is not finite (n = 0 included), means the row has no posterior (the rule of fz_draw_logwt and fz_mw_sweep):
 * every output of the row is nan, its share 0, and it is counted in nskip.  Otherwise w_t = exp(r_t - m); an entry with w_t == 0
 * contributes nothing at all (not 0 * inf); Z = sum w_t; column l includes the entries with w_t > 0 and Vm[j_t][l] != 0;
 * c_tl = s_t V[j_t][l] (one rounding), and over the included entries
 *     Z_l     = sum w_t                      share_l = Z_l / Z                     mean_l = sum w_t c_tl / Z_l
 *     var_l   = sum w_t (c_tl - mean_l)^2 / Z_l  [+ sum w_t (s_t Ve[j_t][l])^2 / Z_l   with Ve]
 * -- the CENTRAL form of the law of total variance.  Z_l == 0: mean_l = var_l = nan, share_l = 0.  Entries past nnbr[i] are never
 * read.  Every sum is formed in one fixed order that depends on the row alone (thread q of the object's 64 or 256 adds the entries
 * q, q + 64 [256], ... in order; one xor butterfly over the lanes; the wave sums in wave order): the same bits whatever the chunking
 * under the workspace limit, the object order, the number of objects in the call, and host or device arguments.
 * Refusals, before anything is gathered: an index outside [0, M) within the count, or a count outside [0, W]: -3; L < 1: -4; L > 32
 * (FZ_MOM_LMAX, the band limit), W > 2^20 (FZ_DRAW_LMAX) or M >= 2^31: -5; dense rows with W != M: -4.
 *
 * fz_row_moments -- rows (N, W), neighbors (N, W) int64 and nnbr (N) int64 (both NULL: dense rows), scale (N, W) or NULL, mean (N, L),
 *   var (N, L) or NULL, share (N, L) or NULL: host or device, staged in chunks from the workspace limit.  values, value_errs (or NULL),
 *   value_mask (or NULL): (M, L), host or device.  nskip: one int64.
 * fz_phot_sums -- x, xe, xm, mean, var (N, B), host or device, staged in chunks of whole strips.  Per band b over the objects with
 *   xm != 0 and finite x, xe, p = mean, v = var:  omega = 1 / (xe^2 + v), d = x - p;  A = sum omega x p, B = sum omega p^2,
 *   C = sum omega d^2, n = their number.  clip > 0: an object-band with omega d^2 > clip^2 is left out of all four and counted in
 *   nclip (clip == 0: off; negative or nan: -4).  sums (3, B) float64 = A, B, C; counts (2, B) int64 = n, nclip.  Partial sums run
 *   over strips of 1024 objects counted from object 0 (thread t adds objects t, t + 256, ... of its strip, then a halving tree) and
 *   the strip sums are added in index order: chunking does not change a bit.  B < 1: -4; B > 32: -5. */
int  fz_row_moments(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr,
                    const double* scale, int64_t M, int32_t L, const double* values, const double* value_errs, const double* value_mask,
                    double* mean, double* var, double* share, int64_t* nskip);
int  fz_phot_sums(fz_ctx* ctx, const double* x, const double* xe, const double* xm, const double* mean, const double* var, int64_t N,
                  int32_t B, double clip, double* sums, int64_t* counts);

/* ---- posterior bin masses and mixture CDFs of a Gaussian label kernel (extension, no reference counterpart; docs/bins.md) ----
 * The law.  A row r[0..n) of ln-weights with model indices j_t (dense rows: j_t = t, n = M), labels y (M) and label errors s (M),
 * edges e[0..E) finite and strictly increasing (E - 1 >= 1 bins), a cut lncut = ln(wt_thresh) < 0 (-inf: none).  A nan among the
 * counted entries, or a max m that is not finite (n = 0 included), means the row has no posterior (the rule of fz_row_moments): every
 * output of the row is nan and it is counted in nskip.  Otherwise entry t is included iff r_t - m > lncut (one IEEE subtraction,
 * strict) and w_t = exp(r_t - m) > 0; Z = sum w_t over the included entries; q_j = 1 / (s_j sqrt 2), each operation rounded once, and
 *     F_t(x) = 0.5 erfc(-((x - y_j) q_j))               s_j > 0
 *     F_t(x) = 1 if x >= y_j else 0                     s_j == 0 (q_j = +inf); a bin EDGE at y_j belongs to the bin above it: the
 *                                                       whole mass goes to the bin with e_k <= y_j < e_k+1, y_j == e[E-1] is above
 *     p_k   = sum w_t (F_t(e_k+1) - F_t(e_k)) / Z       below = sum w_t F_t(e_0) / Z
 *     above = sum w_t 0.5 erfc(+((e_E-1 - y_j) q_j)) / Z                  (s_j == 0: 1 if y_j >= e_E-1 else 0)
 *     normalize: p_k /= sum_k p_k  (nan by IEEE division when no mass lies inside the range)
 *     C_p   = sum w_t F_t(x_p) / Z                      the CDF at points x (P), shared or per object, in any order
 * Entries past nnbr[i] are never read.  Every sum is formed in one fixed order that depends on the row length and the bin count alone
 * (thread q of the object's 64 or 256 adds the entries q, q + 64 [256], ... in order; one xor butterfly over the lanes; the wave sums
 * in wave order; the sum over bins by lane l over bins l, l + 64, ... and one butterfly): the same bits whatever the chunking under
 * the workspace limit, the object order, the number of objects in the call, and host or device arguments.
 * Refusals, before any row is walked: E < 2 (P < 1), an edge or point that is not finite, edges that do not increase strictly, a label
 * that is not finite or an error that is negative or nan (the smallest such model is named), lncut >= 0 or nan: -4; more than 256
 * bins or points (FZ_BINS_MAX), W > 2^20 (FZ_DRAW_LMAX) or M >= 2^31: -5.  An index outside [0, M) within the count, or a count outside
 * [0, W]: -3, before anything is gathered for that row.
 *
 * fz_row_bins -- rows (N, W), neighbors (N, W) int64 and nnbr (N) int64 (both NULL: dense rows), p (N, E - 1), below and above (N) or
 *   NULL: host or device, staged in chunks from the workspace limit.  labels, label_errs (M), edges (E): host or device.  nskip: one
 *   int64.
 * fz_row_cdf -- points (P) with per_object == 0, else (N, P) staged with the rows; cdf (N, P). */
int  fz_row_bins(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                 const double* labels, const double* label_errs, const double* edges, int64_t E, double lncut, int32_t normalize,
                 double* p, double* below, double* above, int64_t* nskip);
int  fz_row_cdf(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                const double* labels, const double* label_errs, const double* points, int64_t P, int32_t per_object, double lncut,
                double* cdf, int64_t* nskip);

/* ---- posterior quantiles of the same label kernel (extension, no reference counterpart; docs/quantiles.md) ----
 * The law.  Selection, w_t, Z, the strict ln-space cut and the rows without a posterior (every output nan, counted in nskip) are
 * those of fz_row_cdf; entries past nnbr[i] are never read.  C(x) = sum w_t F_t(x) / Z with F_t the right-continuous kernel CDF
 * above, C-(x) its left limit (x > y_j for s_j == 0), and the quantile function is Q(p) = inf{x : C(x) >= p}.  probs[0..Q): each
 * finite and strictly inside (0, 1), shared by all objects, in any order, duplicates allowed, 1 <= Q <= 256 (FZ_BINS_MAX).  Label
 * errors must be finite here (s = inf has no quantile) and |y_j| + 40 s_j must be finite.  Per row, over the included entries:
 *     hull   [a0, b0] = [min(y_j - 40 s_j), max(y_j + 40 s_j)]   (erfc(40 / sqrt 2) is 0 in fp64: C(a0-) = 0, C(b0) = 1 as evaluated)
 *     R = max(|a0|, |b0|),  delta = 4 u R,  tau = 4 (W / 64 + 16) u,  u = 2^-53
 * An output x for (row, p) lies in the hull and satisfies, in exact arithmetic,
 *     C-(x - 2 delta) - 2 tau  <=  p  <=  C(x + 2 delta) + 2 tau
 * -- |C(x) - p| <= 2 tau up to 2 delta on a continuous mixture, within 2 delta of the label at which C crosses p at a point mass, any
 * point of the gap on a flat stretch.  The solve keeps a bracket C_dev(a) < p <= C_dev(b) from the hull inward and stops at
 * |C_dev(x) - p| <= tau with a positive density sum at x (x is returned) or b - a <= delta (b is returned); C_dev is the fixed-order
 * sum of fz_row_cdf, within tau of C.  Where the density sum is 0 (point masses, a gap) the solve goes on to the lower end of the flat
 * stretch: p = 1/2 of two equal point masses gives the lower label.
 * Each evaluation also forms the density sum w_t q_j exp(-z^2) / sqrt(pi), z = (x - y_j) q_j (0 for s_j == 0).  The step is Newton's from
 * the bracket end with the smaller residual, and a bisection when that end's density is 0, when the Newton point leaves the bracket,
 * or when neither the bracket nor that residual halved in the last step; the first bisections go to the ends of Cantelli's bracket
 * mu -+ sigma sqrt((1 - p) / p), sqrt(p / (1 - p)) (mixture mean and deviation, rounded outward, inside the hull), later ones to the
 * midpoint.  The start is mu + 0.6267 sigma ln(p / (1 - p)) inside that bracket.  At most FZ_QUANT_MAXIT = 128 evaluations per
 * (row, p): a solve that ends on the cap returns its bracket midpoint and is counted in nfail; niter is the total number of
 * evaluations.  An output is a function of the row's counted entries in order, the label records, p and W alone: not of the other
 * probabilities, their number or order, the chunking under the workspace limit, the object order or count, or host versus device
 * arguments.
 * Refusals, before any row is walked: Q < 1, a probability outside (0, 1) or not finite, a label that is not finite, an error that is
 * negative, nan or inf, an overflowing |y| + 40 s (the smallest such model is named), lncut >= 0 or nan: -4; Q > 256 (FZ_BINS_MAX),
 * W > 2^20 (FZ_DRAW_LMAX) or M >= 2^31: -5.  An index outside [0, M) within the count, or a count outside [0, W]: -3, before anything
 * is gathered for that row.
 *
 * fz_row_quantiles -- rows, neighbors, nnbr as fz_row_bins; labels, label_errs (M), probs (Q): host or device; out (N, Q): host or
 *   device, staged in chunks; nskip, nfail, niter: one int64 each, host or device. */
int  fz_row_quantiles(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                      const double* labels, const double* label_errs, const double* probs, int64_t Q, double lncut, double* out,
                      int64_t* nskip, int64_t* nfail, int64_t* niter);

/* ---- posterior scoring rules of the same label kernel (extension, no reference counterpart; docs/scores.md) ----
 * The law.  Selection, m, w_t = exp(r_t - m), Z, the strict ln-space cut and the rows without a posterior (every output nan, ninc 0,
 * counted in nskip) are those of fz_row_bins; entries past nnbr[i] are never read; repeated model indices are separate entries.
 * Labels y must be finite, label errors s finite and >= 0 (s = inf, a flat kernel, has no finite score); an error whose square is 0
 * in fp64 (s < 2^-537 = 2.2e-162) is read as s = 0, a point mass, everywhere below.  Points x (P) shared or
 * (N, P) per object, finite, in any order, 1 <= P <= 256 (FZ_BINS_MAX).  With W_t = w_t / Z over the included entries,
 *     A(d, v) = d erf(d / sqrt(2 v)) + sqrt(2 v / pi) exp(-d^2 / 2 v)      v > 0;   |d| for v == 0        (always >= 0)
 *     G(d, v) = exp(-d^2 / 2 v) / sqrt(2 pi v)                             v > 0;   +inf if d == 0 else 0 for v == 0
 *     lnpdf_ip = ln sum_t W_t N(x_ip | y_t, s_t)     formed in ln space: a_t = (r_t - m) - z_t^2 - ln s_t, z_t = (x - y_t) q_t,
 *                q_t = 1 / (s_t sqrt 2); the max a_max of the a_t first, then a_max + ln sum exp(a_t - a_max) - ln Z - ln sqrt(2 pi).
 *                An included entry with s_t == 0 contributes +inf if x == y_t, nothing otherwise.
 *     crps_ip  = sum_t W_t A(x_ip - y_t, s_t^2)  -  spread_i
 *     spread_i = 1/2 sum_t sum_u W_t W_u A(y_t - y_u, s_t^2 + s_u^2)  =  sum_{t<u} ... + 1/2 sum_t W_t^2 A(0, 2 s_t^2)
 *     sqnorm_i = sum_t sum_u W_t W_u G(y_t - y_u, s_t^2 + s_u^2)       the integral of the squared density; +inf as soon as one
 *                included s_t == 0
 *     ninc_i   = the number of included entries
 * (the CDE loss of a truth x is sqnorm - 2 exp(lnpdf)).  Each unordered pair is evaluated once and A and G share their exp; the pair
 * sums are formed over w_t w_u and divided by Z twice.  Every sum has one fixed order that depends on the row alone.  Point sums: thread
 * q of the object's 64 or 256 adds the entries q, q + 64 [256], ... in order, one xor butterfly over the lanes, the wave sums in wave
 * order.  Pair sums: the included entries are compacted in entry order; tile I holds entries 64 I .. 64 I + 63 one per lane; a lane adds
 * its terms over the tiles J >= I and the entries u of J in order (on the diagonal tile u > lane, and half of its own term), one
 * butterfly; rows longer than FZ_DRAW_WAVE_LMAX deal the tiles I to four waves round-robin and add the wave sums in wave order.  The
 * same bits whatever the chunking under the workspace limit, the object order, the number of objects in the call, the outputs asked
 * for, and host or device arguments.
 * The pair sums of a row are quadratic in its included count: with crps, spread or sqnorm asked for, a row of more than
 * FZ_SCORES_NMAX = 16384 included entries is refused, -5, naming the object and the limit, after the counts of its chunk are known and
 * before any pair sum of that chunk is started.  Without them there is no cap.
 * Refusals, before any row is walked: P < 1, a point that is not finite, a label that is not finite or an error that is negative, nan
 * or inf (the smallest such model is named), lncut >= 0 or nan: -4; P > 256 (FZ_BINS_MAX), W > 2^20 (FZ_DRAW_LMAX) or M >= 2^31: -5.
 * An index outside [0, M) within the count, or a count outside [0, W]: -3, before anything is gathered for that row.
 *
 * fz_row_scores -- rows, neighbors, nnbr as fz_row_bins; labels, label_errs (M): host or device; points (P) with per_object == 0,
 *   else (N, P) staged with the rows.  lnpdf, crps (N, P), spread, sqnorm (N), ninc (N) int64: host or device, staged in chunks, each
 *   may be NULL; the pair sums run only if crps, spread or sqnorm is given.  Per object 24 W + 16 bytes of device scratch count towards
 *   the chunk size under the workspace limit.  nskip: one int64. */
int  fz_row_scores(fz_ctx* ctx, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                   const double* labels, const double* label_errs, const double* points, int64_t P, int32_t per_object, double lncut,
                   double* lnpdf, double* crps, double* spread, double* sqnorm, int64_t* ninc, int64_t* nskip);

/* ---- Monte-Carlo draws of the k-NN fitter on the device (extension; docs/knn.md, knn.py:158-188 / 830-832) ----
 * The reference draws its K feature sets (knn.py:158-188) and every object's query features (knn.py:830-832) with NumPy's normal and
 * maps them to magnitudes / luptitudes.  Here the variates are Philox4x32-10: one call gives two standard normals by Box-Muller
 * (u1 = 1 - U(words 0, 1), u2 = U(words 2, 3), r = sqrt(-2 ln u1), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2)) under the key
 * (key0, key1 ^ 0x6B6E6D63) at the counter (row lo, row hi, band >> 1, set): an even band takes z0, an odd one z1; set 0 is a query
 * draw of object `first + i`, set 1 + t feature set t of model j.  A draw is a function of (key, row, band, set) alone.  The law is the
 * reference's, the realisation for a seed is not.
 * fz_knn_map -- kind 0 identity, 1 magnitude (-2.5 log10(d / zeropoints)), 2 luptitude (-2.5 / ln 10 (asinh(d / (2 skynoise)) +
 *   ln(skynoise / zeropoints))), with one fp64 constant per band.
 * fz_knn_draw_features -- x, xe, q (N, F) float64, host or device, rows AS GIVEN (before any clean): q = map(fma(xe, z, x)) in fp64.
 *   xe == 0 gives x; non-finite x follows IEEE arithmetic; a negative or nan xe: -4, naming the smallest such object.  N == 0: no launch.
 * fz_knn_draw_trees -- models, models_err (M, F) float64, host or device (the shape of the uploaded models): set t, model j is
 *   float32(map(double(float32(fma(ye, z, y))))) -- the reference's two float32 roundings, the map in fp64 between them -- and the K
 *   sets become the resident sets exactly as fz_knn_upload_trees of the same floats makes them; feats_out (K, M, F) float32, host or
 *   device, or NULL: a copy of them.  A negative or nan error: -4, nothing installed. */
typedef struct fz_knn_map {
    int32_t kind;               /* 0 identity, 1 magnitude, 2 luptitude */
    int32_t reserved_;
    double  skynoise[32];       /* per band (luptitude) */
    double  zeropoints[32];     /* per band (magnitude, luptitude) */
} fz_knn_map;
int  fz_knn_draw_features(fz_ctx* ctx, const double* x, const double* xe, int64_t N, int32_t F, const fz_knn_map* map, uint32_t key0,
                          uint32_t key1, int64_t first, double* q);
int  fz_knn_draw_trees(fz_ctx* ctx, const double* models, const double* models_err, int32_t K, int64_t M, int32_t F,
                       const fz_knn_map* map, uint32_t key0, uint32_t key1, float* feats_out /* may be NULL */);

/* diagnostic: evaluate one of the library's device math helpers elementwise
 * (which: 0 v_rcp_f64 seed, 1 / 2 rcp with one / two Newton steps, 3 log_pos,
 * 4 exp_neg).  Used by tests to pin their accuracy against NumPy. */
int  fz_selftest_math(fz_ctx* ctx, int32_t which, const double* x, int64_t n, double* out);

#ifdef __cplusplus
}
#endif
#endif /* FRANKENZ_HIP_H */
