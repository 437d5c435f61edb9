// ---- knn.py ABI ------------------------------------------------------------------
// (K,M,F) float32 Monte-Carlo feature sets -> device SoA [K][FT][Mp], zero padded
__global__ void k_knn_pack(const float* in, int K, int64_t M, int F, int FT, int64_t Mp, float* out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y;
    if (j >= Mp) return;
    for (int f = 0; f < FT; ++f)
        out[((size_t)t * FT + f) * Mp + j] = (j < M && f < F) ? in[((size_t)t * M + j) * F + f] : 0.0f;
}

// the shape checks of a set of feature sets against the uploaded models
static int knn_trees_shape(const fz_ctx* c, const char* who, int32_t K, int64_t M, int32_t F) {
    if (K <= 0 || M <= 0 || F <= 0) return fail(-1, "%s: bad shape", who);
    if (!c->M || M != c->M || F != c->B) return fail(-1, "%s: feature sets (%lld,%d) must match the uploaded models (%lld,%d)", who,
                                                   (long long)M, F, (long long)c->M, c->B);
    return 0;
}
// The shared tail of fz_knn_upload_trees and fz_knn_draw_trees: the raw (K,M,F) float32 block sits in d_pl[0] (copied in, or drawn by
// k_knn_mc_sets) and becomes the resident sets -- the SoA copy, the k-d ordering, the operands of the matrix-pipe search.
static int knn_install_trees(fz_ctx* c, int32_t K, int64_t M, int32_t F) {
    const size_t raw = (size_t)K * M * F * 4;
    FZCHK(c->d_trees.ensure((size_t)K * c->BT * c->Mp * 4));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(k_knn_pack, dim3((unsigned)((c->Mp + 255) / 256), (unsigned)K), dim3(256), 0, c->stream,
                           c->d_pl[0].as<float>(), (int)K, M, (int)F, c->BT, c->Mp, c->d_trees.as<float>());
    }
    HIPCHK(hipGetLastError());
    c->knn_mfma = false; c->knn_sorted = false;
    // (F <= 5 carries the model's original index as a float in the B operand's free slot: exact below 2^24 models only --
    //  larger sets keep the vector-ALU search)
    if (F <= 6 && !(F <= 5 && M >= (1 << 24))) {        // operands of the matrix-pipe Euclidean search (fz_knn_mfma.h): centres, B tiles, max centred norm
        FZCHK(c->d_kcen.ensure((size_t)K * 8 * 4));
        FZCHK(c->d_kpmax.ensure((size_t)K * 4));
        FZCHK(c->d_kbmat.ensure((size_t)K * (c->Mp >> 6) * FZ_KM_TSTR * 4));
        HIPCHK(hipMemsetAsync(c->d_kpmax.p, 0, (size_t)K * 4, c->stream));
        // k-d order of every set's models (the reference's index is a k-d tree too: knn.py:186): recursive splits along the widest feature
        // of the node, at a multiple of 64 models (each node's tiles split floor / ceil), so that every 64-model tile of the device layout
        // IS one leaf -- disjoint, tight boxes.  On the benchmark's sets a query ball reaches 25 such tiles (57 in round 3's Morton order,
        // whose tiles straddle the curve's jumps) and a wave's 16 queries 107 (215).  Leaves in depth-first order; the tree is implicit
        // (a node over tiles [a, b) splits at a + (b - a) / 2): tab[set][tile][2] = {split feature, split value (float bits)} of the
        // internal node whose right half starts at that tile -- what a query needs to find its leaf (knn_kd_leaf).
        // Needs the free slot 7 of the B operand for the original index (F <= 5) and indices that a float holds exactly.
        const bool sorted = F <= 5 && M < (1 << 24) && !fz_dbg_set("FZ_KNN_NOSORT");
        if (sorted) {
            std::vector<float> h((size_t)K * M * F);
            HIPCHK(hipStreamSynchronize(c->stream));
            HIPCHK(hipMemcpy(h.data(), c->d_pl[0].p, raw, hipMemcpyDeviceToHost));
            const int64_t ntl = (M + 63) / 64;
            std::vector<int32_t> perm((size_t)K * M), tab((size_t)K * ntl * 2, 0);
            std::vector<std::pair<int64_t, int64_t>> stack;
            for (int t = 0; t < K; ++t) {
                const float* ft = h.data() + (size_t)t * M * F;
                int32_t* ix = perm.data() + (size_t)t * M;
                for (int64_t j = 0; j < M; ++j) ix[j] = (int32_t)j;
                auto fv = [&](int32_t j, int d) { const float v = ft[(int64_t)j * F + d]; return v == v ? v : INFINITY; };     // (nan: one end, consistently)
                stack.clear();
                stack.emplace_back(0, M);
                while (!stack.empty()) {
                    const int64_t lo = stack.back().first, hi = stack.back().second;
                    stack.pop_back();
                    const int64_t n = hi - lo;
                    if (n <= 64) continue;
                    int dbest = 0; float ebest = -1.f;
                    for (int d = 0; d < F; ++d) {
                        float mn = INFINITY, mx = -INFINITY;
                        for (int64_t j = lo; j < hi; ++j) { const float v = fv(ix[j], d); if (v < mn) mn = v; if (v > mx && v < INFINITY) mx = v; }
                        const float e = mx - mn;
                        if (e > ebest) { ebest = e; dbest = d; }
                    }
                    const int64_t half = (((n + 63) / 64) / 2) * 64;
                    std::nth_element(ix + lo, ix + lo + half, ix + hi, [&](int32_t a, int32_t b) { const float va = fv(a, dbest), vb = fv(b, dbest); return va < vb || (va == vb && a < b); });
                    {
                        const float sv = fv(ix[lo + half], dbest);           // left: feature <= sv, right: >= sv
                        int32_t bits; memcpy(&bits, &sv, 4);
                        int32_t* nd = tab.data() + ((size_t)t * ntl + (size_t)((lo + half) / 64)) * 2;
                        nd[0] = dbest; nd[1] = bits;
                    }
                    stack.emplace_back(lo, lo + half);
                    stack.emplace_back(lo + half, hi);
                }
            }
            FZCHK(c->d_kperm.ensure(perm.size() * 4)); FZCHK(c->d_ktab.ensure(tab.size() * 4));
            FZCHK(copy_in(c, c->d_kperm.p, perm.data(), perm.size() * 4));
            FZCHK(copy_in(c, c->d_ktab.p, tab.data(), tab.size() * 4));
        }
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_knn_center, dim3((unsigned)K), dim3(256), 0, c->stream, c->d_pl[0].as<float>(), M, (int)F, c->d_kcen.as<float>());
        hipLaunchKernelGGL(fz::k_knn_pack_mfma, dim3((unsigned)((c->Mp + 255) / 256), (unsigned)K), dim3(256), 0, c->stream,
                           c->d_pl[0].as<float>(), M, (int)F, c->Mp, c->d_kcen.as<float>(), c->d_kbmat.as<float>(), c->d_kpmax.as<unsigned>(),
                           sorted ? c->d_kperm.as<int>() : (const int*)nullptr);
        // bounding boxes of the 64-model tiles and of <= 128 groups of 2^gsl tiles, for the scan's reachability mask (spatial orders only)
        FZCHK(c->d_ktbox.ensure((size_t)K * (c->Mp >> 6) * 16 * 4));
        hipLaunchKernelGGL(fz::k_knn_boxes, dim3((unsigned)(c->Mp >> 6), (unsigned)K), dim3(64), 0, c->stream, c->d_pl[0].as<float>(), M, (int)F,
                           c->Mp, sorted ? c->d_kperm.as<int>() : (const int*)nullptr, c->d_ktbox.as<float>());
        c->knn_gsl = 0;
        while ((((int64_t)(M + 63) >> 6) + ((int64_t)1 << c->knn_gsl) - 1) >> c->knn_gsl > 128) ++c->knn_gsl;
        FZCHK(c->d_kgbox.ensure((size_t)K * 128 * 16 * 4));
        hipLaunchKernelGGL(fz::k_knn_maskboxes, dim3(128, (unsigned)K), dim3(64), 0, c->stream, c->Mp, (int)M, c->knn_gsl, c->d_ktbox.as<float>(), c->d_kgbox.as<float>());
        HIPCHK(hipGetLastError());
        c->knn_mfma = true; c->knn_sorted = sorted;
    }
    c->knn_K = K; c->knn_F = F; c->knn_M = M;
    return 0;
}

extern "C" int fz_knn_upload_trees(fz_ctx* c, const float* feats, int32_t K, int64_t M, int32_t F) {
    if (!c || !feats) return fail(-1, "fz_knn_upload_trees: NULL argument");
    FZCHK(knn_trees_shape(c, "fz_knn_upload_trees", K, M, F));
    HIPCHK(hipSetDevice(c->device));
    const size_t raw = (size_t)K * M * F * 4;
    FZCHK(c->d_pl[0].ensure(raw));
    FZCHK(copy_in(c, c->d_pl[0].p, feats, raw));
    return knn_install_trees(c, K, M, F);
}

#ifdef FZ_KM_STATS
// development counters of k_knn_mfma (fz_knn_mfma.h, tools/devbuild.sh with FZ_DEV_MAINFLAGS=-DFZ_KM_STATS): printed per launch
static void kmstats_dump(fz_ctx* c, const char* what) {
    unsigned long long h[128], z[128] = {0};
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(fz::fz_kmstats), sizeof h);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(fz::fz_kmstats), z, sizeof z);
    const double w = h[0] ? (double)h[0] : 1.0;
    fprintf(stderr, "KMSTATS %s: waves %llu | per wave: tiles %.1f slow-iter %.1f passing %.1f admitted %.1f drains %.1f drain-rounds %.1f insertions %.1f\n",
            what, h[0], h[1] / w, h[2] / w, h[3] / w, h[4] / w, h[5] / w, h[6] / w, h[7] / w);
    fprintf(stderr, "KMSTATS   cycles per wave: setup %.0f | mask %.0f | next_tile+stage %.0f | tile (MFMA, signs, barrier) %.0f | slow %.0f | drain %.0f | output %.0f | wait for the next tile %.0f\n",
            h[8] / w, h[9] / w, h[10] / w, h[11] / w, h[12] / w, h[13] / w, h[14] / w, h[15] / w);
}
#define KMSTATS_DUMP(c, w) kmstats_dump(c, w)
#else
#define KMSTATS_DUMP(c, w) do { } while (0)
#endif
static bool knn_on_matrix_pipe(const fz_ctx* c, int pnorm) {
    return pnorm == 2 && c->knn_mfma && !fz_dbg_set("FZ_KNN_FP64") && !fz_dbg_set("FZ_KNN_NOMFMA");
}
// k beyond one wave's width (64) is served by the matrix-pipe search only (lists in LDS, 64-entry segments)
static int check_knn_k(const fz_ctx* c, int k, int pnorm, const char* who) {
    if (k <= 0 || k > FZ_KNN_KMAX) return fail(-5, "%s: k=%d unsupported (1..%d)", who, k, FZ_KNN_KMAX);
    if (k > 64 && !knn_on_matrix_pipe(c, pnorm))
        return fail(-5, "%s: k=%d > 64 needs the Euclidean norm and at most 6 features (the other searches keep one list entry per lane)", who, k);
    return 0;
}
// the norm and bound of a search as the kernels take them: pnorm 2 / 1 / 0 (inf), b2 the bound (squared under the Euclidean norm)
static int parse_lp_norm(const char* who, double lp_norm, double dub, int* pnorm, double* b2) {
    if (lp_norm == 2.0) *pnorm = 2; else if (lp_norm == 1.0) *pnorm = 1; else if (lp_norm == INFINITY) *pnorm = 0;
    else return fail(-5, "%s: Minkowski p=%g is not implemented (1, 2 and inf are)", who, lp_norm);
    *b2 = (dub == INFINITY || *pnorm != 2) ? dub : dub * dub;      // KDTree keeps d < bound (strict)
    return 0;
}
static int run_knnquery(fz_ctx* c, const double* q, int64_t n, int k, double b2, int64_t* idx, int pnorm) {
    if (knn_on_matrix_pipe(c, pnorm)) {
        // register lists (row-parallel admissions) for k <= 32, the reference's default is 20; FZ_KNN_SERIAL=1: the wave-serial LDS lists
        const int kpl = fz_dbg_set("FZ_KNN_SERIAL") ? 0 : (k <= 20 ? 5 : (k <= 32 ? 8 : 0));
        const int kpad = std::max((k + 3) & ~3, 4 * kpl);
        // one wave per block with its own 64-model tiles: no barrier skew between waves whose admission paths differ in
        // length, and every wave scans from its own queries' place (shared 128-model tiles for four waves measured 79.9 ms
        // against 75.3 per 1e5 x 25 x 1e5 search before the visiting order went in)
        const int nwb = 1;
        // dynamic LDS: the wave's sorted lists / its admission queues, then one bit per 64-model tile (the scan's reachability mask)
        const size_t lds = fz::knn_mfma_list_bytes(kpad, kpl) + (size_t)((((c->knn_M + 63) >> 6) + 63) >> 6) * 8;
        auto kern = (c->knn_F == 5) ? (kpl == 5 ? fz::k_knn_mfma<64, 5, 1, 5> : (kpl == 8 ? fz::k_knn_mfma<64, 5, 1, 8> : fz::k_knn_mfma<64, 5, 1, 0>))
                                    : (kpl == 5 ? fz::k_knn_mfma<64, 0, 1, 5> : (kpl == 8 ? fz::k_knn_mfma<64, 0, 1, 8> : fz::k_knn_mfma<64, 0, 1, 0>));
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        const unsigned gx = (unsigned)((n + 16 * nwb - 1) / (16 * nwb));
        // the queries grouped by their leaf in set 0's tree (counting sort): the 16 queries of a wave are neighbours, and each wave
        // starts its scan at its own queries' leaf in the set it searches
        const int* qperm = nullptr; const int* ktab = nullptr;
        if (c->knn_sorted && nwb == 1) {
            FZCHK(c->d_kqperm.ensure((size_t)n * 4)); FZCHK(c->d_kqcnt.ensure(4096 * 4));
            HIPCHK(hipMemsetAsync(c->d_kqcnt.p, 0, 4096 * 4, c->stream));
            const unsigned gq = (unsigned)((n + 255) / 256);
            const int kdn = (int)((c->knn_M + 63) / 64);
            hipLaunchKernelGGL(fz::k_knn_qhist, dim3(gq), dim3(256), 0, c->stream, q, n, c->knn_F, c->d_kqcnt.as<int>(), c->d_ktab.as<int>(), kdn);
            hipLaunchKernelGGL(fz::k_knn_qscan, dim3(1), dim3(1024), 0, c->stream, c->d_kqcnt.as<int>());
            hipLaunchKernelGGL(fz::k_knn_qscatter, dim3(gq), dim3(256), 0, c->stream, q, n, c->knn_F, c->d_kqcnt.as<int>(),
                               c->d_kqperm.as<int>(), c->d_ktab.as<int>(), kdn);
            qperm = c->d_kqperm.as<int>(); ktab = c->d_ktab.as<int>();
        }
        const bool skip = c->knn_sorted && !fz_dbg_set("FZ_KNN_NOBOX");      // (storage order: boxes exclude nothing)
        const float* gbx = skip ? c->d_kgbox.as<float>() : nullptr;
        const float* tbx = skip ? c->d_ktbox.as<float>() : nullptr;
        Timer t(c, &c->tm.ms_knn, &c->tm.n_knn);
        // every feature set is searched cold, one launch (fz_knn_mfma.h: why set 0's neighbours no longer seed the others)
        hipLaunchKernelGGL(kern, dim3(gx, (unsigned)c->knn_K), dim3(nwb * 64), lds, c->stream,
                           c->d_kbmat.as<float>(), c->d_kcen.as<float>(), c->d_kpmax.as<float>(), c->Mp,
                           (int)c->knn_M, q, n, c->knn_F, k, kpad, b2, idx, c->knn_K, qperm, ktab, tbx, gbx, c->knn_gsl);
        KMSTATS_DUMP(c, "search");
        HIPCHK(hipGetLastError());
        return 0;
    }
    const fz_bt_table* t = bt_lookup(c);
    return t ? t->knnquery(c, q, n, k, b2, idx, pnorm) : -5;
}
static int run_knnsubset(fz_ctx* c, int mode, int var, int dp, int64_t n, const int64_t* idx, int W, const fz_kde_opts* ko,
                         const KnnOut* out, int* ef) {
    const fz_bt_table* t = bt_lookup(c);
    return t ? t->knnsubset(c, mode, var, dp, n, idx, W, ko, out, ef) : -5;
}

// launch k_knn_predict on device-resident chunk buffers
static int knn_predict_chunk(fz_ctx* c, int64_t n, int64_t M, const double* dl, const int64_t* dn, const int64_t* dc, int W,
                             const fz_kde_opts* ko, double* dp, double* dm, double* de) {
    if (!ko->use_wt_thresh) return run_cdf(c, n, W, M, dl, dn, dc, 1, ko, dp, dm, de);
    const int64_t savedM = c->M; c->M = M;
    KdeView kv; const int rc = fz_kde_view(c, kv);
    c->M = savedM;
    if (rc) return rc;
    FZCHK(fz_upload_kv(c, kv));
    int wpb = 4;
    while (wpb > 1 && (size_t)kv.acc_stride * 8 * wpb > 64 * 1024) wpb >>= 1;
    const size_t lds = (size_t)kv.acc_stride * 8 * wpb;
    HIPCHK(hipFuncSetAttribute((const void*)k_knn_predict, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int ef = 0;
    FZCHK(fz_flag_roundtrip(c, ef, [&](int* d_flags) {
        Timer t(c, &c->tm.ms_knn, &c->tm.n_knn);
        hipLaunchKernelGGL(k_knn_predict, dim3((unsigned)((n + wpb - 1) / wpb)), dim3(wpb * 64), lds, c->stream,
                           c->d_kv.as<KdeView>(), kv.acc_stride, n, (int)M, dl, dn, dc, W, ko->wt_thresh, ko->normalize,
                           dp, dm, de, d_flags);
        return 0;
    }));
    if (ef) return fail(-3, "neighbour table entry outside [0, Nmodel) or Nneighbors outside [0, K*k]");
    return 0;
}

extern "C" int fz_knn_query(fz_ctx* c, const double* q, int64_t N, int32_t k, double lp_norm, double dub, int64_t* idx) {
    if (!c || !q || !idx) return fail(-1, "fz_knn_query: NULL argument");
    if (!c->knn_K) return fail(-1, "fz_knn_query: feature sets have not been uploaded");
    if (k > c->knn_M) return fail(-1, "fz_knn_query: k exceeds the number of models");
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {q, idx}));
    const int F = c->knn_F, K = c->knn_K;
    int pnorm; double b2;
    FZCHK(parse_lp_norm("fz_knn_query", lp_norm, dub, &pnorm, &b2));
    FZCHK(check_knn_k(c, k, pnorm, "fz_knn_query"));
    const StageRows qv(c, q, (size_t)F * 8, c->d_q, STAGE_IN), iv(c, idx, (size_t)K * k * 8, c->d_idx, STAGE_OUT);
    const int64_t nc = std::min<int64_t>(N, 1 << 18);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dq; int64_t* di;
        FZCHK(qv.at(i0, n, &dq)); FZCHK(iv.at(i0, n, &di));
        FZCHK(run_knnquery(c, dq, n, k, b2, di, pnorm));
        FZCHK(iv.back(i0, n));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_knn_fit_predict_prior(fz_ctx* c, double* x, double* xe, double* xm, int64_t N, const int64_t* idx, int64_t W,
                                        const fz_like_opts* o, const fz_kde_opts* ko, const fz_prior* pr, int64_t* neighbors,
                                        int64_t* nnbr, double* lnprior, double* lnlike, double* lnprob, double* chi2,
                                        int64_t* ndim, double* scale, double* scale_err, double* pdfs, double* lmap,
                                        double* levid) {
    fz_prior_lerp pl{};
    if (pr) pl = prior_plain(pr);
    return fz_knn_fit_predict_prior_lerp(c, x, xe, xm, N, idx, W, o, ko, pr ? &pl : nullptr, neighbors, nnbr, lnprior, lnlike, lnprob, chi2, ndim,
                                         scale, scale_err, pdfs, lmap, levid);
}
extern "C" int fz_knn_fit_predict_prior_lerp(fz_ctx* c, double* x, double* xe, double* xm, int64_t N, const int64_t* idx, int64_t W,
                                             const fz_like_opts* o, const fz_kde_opts* ko, const fz_prior_lerp* pr, int64_t* neighbors,
                                             int64_t* nnbr, double* lnprior, double* lnlike, double* lnprob, double* chi2,
                                             int64_t* ndim, double* scale, double* scale_err, double* pdfs, double* lmap,
                                             double* levid) {
    if (!c || !x || !xe || !xm || !idx || !o) return fail(-1, "fz_knn_fit_predict: NULL argument");
    if (!c->M) return fail(-1, "fz_knn_fit_predict: models have not been uploaded");
    if (W <= 0 || W > FZ_KNN_WMAX) return fail(-5, "fz_knn_fit_predict: K*k = %lld unsupported (max %d)", (long long)W, FZ_KNN_WMAX);
    fz_kde_opts kdef{};
    if (pdfs) { FZCHK(check_kde_opts(ko)); if (c->label_mode == 0) return fail(-1, "fz_knn_fit_predict: labels have not been uploaded"); }
    else { kdef.wt_thresh = 1e-3; kdef.use_wt_thresh = 1; kdef.normalize = 1; ko = &kdef; }
    const int mode = eff_mode(c, like_mode(o));
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {x, xe, xm, idx, neighbors, nnbr, lnprior, lnlike, lnprob, chi2, ndim, scale, scale_err, pdfs, lmap, levid}));
    const int64_t G = c->G;
    PriorBind pb; PriorGuard guard{c};
    FZCHK(prior_begin(c, pr, N, c->M, pb));
    const bool want_prior = pb.kind || lnprior || lnprob;
    // outputs: {ptr, bytes per object, the buffer that stages it}
    constexpr int NO = 12;
    const size_t row = (size_t)W * 8;
    const StageRows outs[NO] = {{c, neighbors, row, c->d_nbr, STAGE_OUT}, {c, nnbr, 8, c->d_nn, STAGE_OUT}, {c, lnlike, row, c->d_pl[0], STAGE_OUT},
                                {c, chi2, row, c->d_pl[1], STAGE_OUT}, {c, ndim, row, c->d_pl[2], STAGE_OUT}, {c, scale, row, c->d_pl[3], STAGE_OUT},
                                {c, scale_err, row, c->d_pl[4], STAGE_OUT}, {c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_OUT},
                                {c, lmap, 8, c->d_lmap, STAGE_OUT}, {c, levid, 8, c->d_levid, STAGE_OUT},
                                {c, lnprior, row, c->d_pl[5], STAGE_OUT}, {c, lnprob, row, c->d_pl[6], STAGE_OUT}};
    const StageRows iv(c, idx, row, c->d_idx, STAGE_IN);
    size_t per_obj = row * 3 + (size_t)pb.chunk_bytes_per_obj;
    for (auto& u : outs) if (u.staged()) per_obj += u.row;
    int64_t nc = std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / (int64_t)per_obj, 1 << 18));
    nc = std::min(nc, N);
    const bool cdf = pdfs && !ko->use_wt_thresh;
    // iterative likelihood, CDF rule and priors work from materialised (n,W) rows; the plain
    // case is one fused kernel
    const bool rows_route = (mode == 3) || cdf || want_prior;
    FZCHK(for_chunks(c, x, xe, xm, N, nc, o, pb, [&](int64_t i0, int64_t n, int var, int) -> int {
        const int64_t* di;
        FZCHK(iv.at(i0, n, &di));
        void* dev[NO];
        for (int u = 0; u < NO; ++u) FZCHK(outs[u].at(i0, n, &dev[u]));
        KnnOut ko_; ko_.neighbors = (int64_t*)dev[0]; ko_.nnbr = (int64_t*)dev[1]; ko_.lnlike = (double*)dev[2];
        ko_.chi2 = (double*)dev[3]; ko_.ndim = (int64_t*)dev[4]; ko_.scale = (double*)dev[5];
        ko_.serr = (double*)dev[6]; ko_.pdfs = (double*)dev[7]; ko_.lmap = (double*)dev[8]; ko_.levid = (double*)dev[9];
        int ef = 0;
        if (!rows_route) {
            FZCHK(fz_flag_roundtrip(c, ef, [&](int* d_flags) { return run_knnsubset(c, mode, var, o->dim_prior, n, di, (int)W, ko, &ko_, d_flags); }));
        } else {
            int64_t* nb = ko_.neighbors; int64_t* nn = ko_.nnbr;
            if (!nb) { FZCHK(c->d_nbr.ensure((size_t)n * W * 8)); nb = c->d_nbr.as<int64_t>(); }
            if (!nn) { FZCHK(c->d_nn.ensure((size_t)n * 8)); nn = c->d_nn.as<int64_t>(); }
            double* lpl = ko_.lnlike;
            if (mode == 3) {
                // pdf.py:196-223 on the subset: de-dup, then the mode-C state machine with the
                // neighbour table as indirection
                int dw = 4;                                                         // waves per block: list[wcap] + keys[2 wcap] + positions[2 wcap] ints each
                while (dw > 1 && (size_t)dw * 5 * fz_knn_wcap((int)W) * 4 > 64 * 1024) dw >>= 1;
                const size_t dl = (size_t)dw * 5 * fz_knn_wcap((int)W) * 4;
                HIPCHK(hipFuncSetAttribute((const void*)k_knn_dedup, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dl));
                FZCHK(fz_flag_roundtrip(c, ef, [&](int* d_flags) {
                    Timer t(c, &c->tm.ms_knn, &c->tm.n_knn);
                    hipLaunchKernelGGL(k_knn_dedup, dim3((unsigned)((n + dw - 1) / dw)), dim3(dw * 64), dl, c->stream, n, (int)c->M, di, (int)W, nb, nn,
                                       d_flags);
                    return 0;
                }));
                if (!ef) {
                    FZCHK(run_modec(c, var, n, o, nullptr, nb, nn, (int)W));
                    if (!lpl) lpl = c->d_mc[1].as<double>();                     // in place on the state plane
                    FZCHK(modec_final(c, n, var != VAR_FAST, o, lpl, ko_.chi2, ko_.ndim, ko_.scale, ko_.serr, nb, nn, (int)W));
                }
            } else {
                KnnOut k2 = ko_;
                k2.neighbors = nb; k2.nnbr = nn; k2.pdfs = nullptr;
                if (!lpl) { FZCHK(c->d_mc[1].ensure((size_t)n * W * 8)); lpl = c->d_mc[1].as<double>(); }
                k2.lnlike = lpl;
                FZCHK(fz_flag_roundtrip(c, ef, [&](int* d_flags) { return run_knnsubset(c, mode, var, o->dim_prior, n, di, (int)W, ko, &k2, d_flags); }));
            }
            if (!ef) {
                const double* lw = lpl;
                if (want_prior) {
                    double* lpr = (double*)dev[11];
                    if (!lpr) { FZCHK(c->d_pl[6].ensure((size_t)n * W * 8)); lpr = c->d_pl[6].as<double>(); }
                    FZCHK(prior_add(c, lpl, n, W, nb, nn, (double*)dev[10], lpr));
                    lw = lpr;
                }
                if (ko_.pdfs) {
                    double* dm = ko_.lmap; double* de = ko_.levid;
                    if (!dm) { FZCHK(c->d_lmap.ensure(n * 8)); dm = c->d_lmap.as<double>(); }
                    if (!de) { FZCHK(c->d_levid.ensure(n * 8)); de = c->d_levid.as<double>(); }
                    if (cdf) FZCHK(run_cdf(c, n, (int)W, c->M, lw, nb, nn, 1, ko, ko_.pdfs, dm, de));
                    else FZCHK(knn_predict_chunk(c, n, c->M, lw, nb, nn, (int)W, ko, ko_.pdfs, dm, de));
                }
            }
        }
        if (ef) return fail(-3, "a neighbour index is outside [0, Nmodel): KDTree returns Nmodel for neighbours beyond "
                                "distance_upper_bound and the reference then fails on models[idxs] (knn.py:847)");
        for (auto& u : outs) FZCHK(u.back(i0, n));
        return 0;
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
extern "C" int fz_knn_fit_predict(fz_ctx* c, double* x, double* xe, double* xm, int64_t N, const int64_t* idx, int64_t W,
                                  const fz_like_opts* o, const fz_kde_opts* ko, int64_t* neighbors, int64_t* nnbr,
                                  double* lnlike, double* chi2, int64_t* ndim, double* scale, double* scale_err,
                                  double* pdfs, double* lmap, double* levid) {
    return fz_knn_fit_predict_prior_lerp(c, x, xe, xm, N, idx, W, o, ko, nullptr, neighbors, nnbr, nullptr, lnlike, nullptr, chi2, ndim,
                                         scale, scale_err, pdfs, lmap, levid);
}

// objects per chunk of the two search drivers (fz_knn_search_fit_predict*, fz_knn_search_fit_draw) at the most
static int64_t knn_search_chunk_cap() { return std::max<int64_t>(1, std::min<int64_t>(1 << 17, fz_dbg_int("FZ_CHUNK", 1 << 17))); }
// *out: the prior of objects [i0, i0 + n) of N, for a driver that hands its chunks to another entry point
static int prior_slice(const fz_prior_lerp* pr, int64_t i0, int64_t n, int64_t N, int64_t M, fz_prior_lerp* out) {
    *out = *pr;
    if (pr->frac) out->frac = pr->frac + i0;
    if (pr->rows) out->rows = pr->rows + i0;
    else if (pr->P != 1) {
        if (pr->P != N) return fail(-4, "ln-prior table has %lld rows for %lld objects and no row index", (long long)pr->P, (long long)N);
        out->table = pr->table + i0 * M; out->P = n;
    }
    return 0;
}
// knn.py:826-874 in one call: the K searches AND the subset likelihood / PDFs, with the (N, K*k) neighbour table never leaving the
// device (it is 4 GB at 1e6 objects x 500 and the two-call form above bounced it through the host: 4 GB out of fz_knn_query,
// 4 GB into fz_knn_fit_predict).  q (N,F): the query features (knn.py:830-832; the caller draws them, so the stream is the
// reference's).  Searched and fitted in chunks of <= 2^17 objects (FZ_CHUNK: fewer).
extern "C" int fz_knn_search_fit_predict_prior(fz_ctx* c, const double* q, double* x, double* xe, double* xm, int64_t N, int32_t k,
                                               double lp_norm, double dub, const fz_like_opts* o, const fz_kde_opts* ko,
                                               const fz_prior* pr, int64_t* neighbors, int64_t* nnbr, double* lnprior, double* lnlike,
                                               double* lnprob, double* chi2, int64_t* ndim, double* scale, double* scale_err,
                                               double* pdfs, double* lmap, double* levid) {
    fz_prior_lerp pl{};
    if (pr) pl = prior_plain(pr);
    return fz_knn_search_fit_predict_prior_lerp(c, q, x, xe, xm, N, k, lp_norm, dub, o, ko, pr ? &pl : nullptr, neighbors, nnbr, lnprior, lnlike,
                                                lnprob, chi2, ndim, scale, scale_err, pdfs, lmap, levid);
}
extern "C" int fz_knn_search_fit_predict_prior_lerp(fz_ctx* c, const double* q, double* x, double* xe, double* xm, int64_t N, int32_t k,
                                                    double lp_norm, double dub, const fz_like_opts* o, const fz_kde_opts* ko,
                                                    const fz_prior_lerp* pr, int64_t* neighbors, int64_t* nnbr, double* lnprior,
                                                    double* lnlike, double* lnprob, double* chi2, int64_t* ndim, double* scale,
                                                    double* scale_err, double* pdfs, double* lmap, double* levid) {
    if (!c || !q || !x || !xe || !xm || !o) return fail(-1, "fz_knn_search_fit_predict: NULL argument");
    if (!c->knn_K) return fail(-1, "fz_knn_search_fit_predict: feature sets have not been uploaded");
    if (k <= 0) return fail(-5, "fz_knn_search_fit_predict: k=%d unsupported", k);
    if (k > c->knn_M) return fail(-1, "fz_knn_search_fit_predict: k exceeds the number of models");
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {q, x, xe, xm}));
    const int F = c->knn_F, K = c->knn_K, B = c->B;
    const int64_t W = (int64_t)K * k, G = c->G, M = c->M;
    int pnorm; double b2;
    FZCHK(parse_lp_norm("fz_knn_search_fit_predict", lp_norm, dub, &pnorm, &b2));
    FZCHK(check_knn_k(c, k, pnorm, "fz_knn_search_fit_predict"));
    const StageRows qv(c, q, (size_t)F * 8, c->d_q, STAGE_IN);
    const int64_t nc = std::min<int64_t>(N, knn_search_chunk_cap());
    FZCHK(c->d_idxs.ensure((size_t)nc * W * 8));
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dq;
        FZCHK(qv.at(i0, n, &dq));
        FZCHK(run_knnquery(c, dq, n, k, b2, c->d_idxs.as<int64_t>(), pnorm));
        fz_prior_lerp pc; const bool has_prior = pr && pr->table;
        if (has_prior) FZCHK(prior_slice(pr, i0, n, N, M, &pc));
        auto at = [&](auto* p, int64_t per) { return p ? p + i0 * per : p; };
        FZCHK(fz_knn_fit_predict_prior_lerp(c, x + i0 * B, xe + i0 * B, xm + i0 * B, n, c->d_idxs.as<int64_t>(), W, o, ko, has_prior ? &pc : nullptr, at(neighbors, W),
                                            at(nnbr, 1), at(lnprior, W), at(lnlike, W), at(lnprob, W), at(chi2, W), at(ndim, W), at(scale, W),
                                            at(scale_err, W), at(pdfs, G), at(lmap, 1), at(levid, 1)));
    }
    return 0;
}

extern "C" int fz_knn_predict_logwt(fz_ctx* c, const double* logwt, const int64_t* neighbors, const int64_t* nnbr, int64_t N,
                                    int64_t W, const fz_kde_opts* ko, double* pdfs, double* lmap, double* levid) {
    if (!c || !logwt || !neighbors || !nnbr || !pdfs) return fail(-1, "fz_knn_predict_logwt: NULL argument");
    FZCHK(check_kde_opts(ko));
    if (c->label_mode == 0) return fail(-1, "fz_knn_predict_logwt: labels have not been uploaded");
    if (W <= 0 || N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {logwt, neighbors, nnbr, pdfs, lmap, levid}));
    const int64_t G = c->G, M = c->label_M;
    const int64_t nc = std::min<int64_t>(N, std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / (W * 16 + G * 8), 1 << 18)));
    const StageRows lv(c, logwt, (size_t)W * 8, c->d_pl[0], STAGE_IN), nv(c, neighbors, (size_t)W * 8, c->d_nbr, STAGE_IN), cv(c, nnbr, 8, c->d_nn, STAGE_IN);
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_OUT), mv(c, lmap, 8, c->d_lmap, STAGE_OUT, true), ev(c, levid, 8, c->d_levid, STAGE_OUT, true);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dl; const int64_t* dn; const int64_t* dc; double *dp, *dm, *de;
        FZCHK(lv.at(i0, n, &dl)); FZCHK(nv.at(i0, n, &dn)); FZCHK(cv.at(i0, n, &dc));
        FZCHK(pv.at(i0, n, &dp)); FZCHK(mv.at(i0, n, &dm)); FZCHK(ev.at(i0, n, &de));
        FZCHK(knn_predict_chunk(c, n, M, dl, dn, dc, (int)W, ko, dp, dm, de));
        FZCHK(pv.back(i0, n)); FZCHK(mv.back(i0, n)); FZCHK(ev.back(i0, n));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- diagnostic: device math helpers, elementwise ----
__global__ void k_selftest_math(int which, const double* x, int64_t n, double* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double r;
    switch (which) {
        case 0: r = rcp_nr<0>(v); break;
        case 1: r = rcp_nr<1>(v); break;
        case 2: r = rcp_nr<2>(v); break;
        case 3: r = log_pos(v); break;
        default: r = exp_neg(v); break;
    }
    out[i] = r;
}
extern "C" int fz_selftest_math(fz_ctx* c, int32_t which, const double* x, int64_t n, double* out) {
    if (!c || !x || !out || n <= 0) return fail(-1, "fz_selftest_math: bad argument");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(c->d_pl[0].ensure(n * 8)); FZCHK(c->d_pl[1].ensure(n * 8));
    FZCHK(copy_in(c, c->d_pl[0].p, x, n * 8));
    hipLaunchKernelGGL(k_selftest_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (int)which,
                       c->d_pl[0].as<double>(), n, c->d_pl[1].as<double>());
    HIPCHK(hipGetLastError());
    FZCHK(copy_out(c, out, c->d_pl[1].p, n * 8));
    return 0;
}
