// Host side of the sparse fits (fz_sparse.h; docs/sparse_fits.md): fz_sparsify_logwt, fz_fit_sparse.
// Included by frankenz_hip.hip after fz_draw_host.inc (for_chunks, chunk_planes, prior_* are above).

static int sparse_limits(const char* who, int64_t L, int64_t W, double lncut) {
    if (W < 1) return fail(-4, "%s: Nkeep = %lld, need at least 1", who, (long long)W);
    if (!(lncut < 0.0)) return fail(-4, "%s: the cut %g is not below 0 (wt_thresh must lie in [0, 1))", who, lncut);
    if (W > FZ_SPARSE_WMAX) return fail(-5, "%s: Nkeep = %lld exceeds FZ_SPARSE_WMAX = %d", who, (long long)W, FZ_SPARSE_WMAX);
    if (L < 1) return fail(-4, "%s: rows of %lld entries", who, (long long)L);
    if (L > FZ_DRAW_LMAX) return fail(-5, "%s: rows of %lld entries exceed FZ_DRAW_LMAX = %d", who, (long long)L, FZ_DRAW_LMAX);
    return 0;
}

// n rows of L ln-weights in device memory -> the kept entries (device; vals, lmap, levid, lnkept may be nullptr).  The geometry is a
// function of L alone (FZ_SPARSE_WPO = 1 / 4 forces one: tests).
static int run_sparse_select(fz_ctx* c, int64_t n, int64_t L, const double* rows, int64_t W, double lncut, int64_t* nbr, int64_t* nn, double* vals,
                             double* lmap, double* levid, double* lnkept) {
    int nw = L <= FZ_DRAW_WAVE_LMAX ? 1 : 4;
    const long long forced = fz_dbg_int("FZ_SPARSE_WPO", 0);
    if (forced == 1 || forced == 4) nw = (int)forced;
    const int64_t step = (int64_t)nw * FZ_DRAW_SEG;
    // the candidate buffer: the kept entries and one step's worth of new ones, plus slack -- half of either, whichever is more -- so
    // that a cut makes room for several steps (with none, every step past the first cut would cut again), and at least the power
    // of two the final sort of the kept entries pads to.  12 B per entry: the LDS decides how many blocks share a CU
    const int64_t wc = std::min<int64_t>(W, (L + step - 1) / step * step);
    int64_t p2 = 1;
    while (p2 < wc) p2 <<= 1;
    const int cap = (int)std::max<int64_t>(wc + step + std::max<int64_t>(wc, step) / 2, p2);
    const size_t nsegL = (size_t)((L + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
    const size_t lds = std::max<size_t>(16 * nsegL, 12 * (size_t)cap);
    if (lds > FZ_LDS_BYTES - 2048) return fail(-5, "sparse fits: rows of %lld entries, %lld kept, need %zu bytes of LDS", (long long)L, (long long)W, lds);
    const void* kern = nw == 1 ? (const void*)fz::k_sparse_select<1> : (const void*)fz::k_sparse_select<4>;
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Timer t(c, &c->tm.ms_other, &c->tm.n_other);
    const dim3 grid((unsigned)n), blk(nw * 64);
    if (nw == 1) hipLaunchKernelGGL(fz::k_sparse_select<1>, grid, blk, lds, c->stream, rows, n, L, (int)W, lncut, cap, nbr, nn, vals, lmap, levid, lnkept);
    else hipLaunchKernelGGL(fz::k_sparse_select<4>, grid, blk, lds, c->stream, rows, n, L, (int)W, lncut, cap, nbr, nn, vals, lmap, levid, lnkept);
    HIPCHK(hipGetLastError());
    return 0;
}

static int run_sparse_gather(fz_ctx* c, const void* plane, int64_t n, int64_t M, const int64_t* nbr, const int64_t* nn, int64_t W, uint64_t fill,
                             uint64_t pad, void* out) {
    const int64_t tot = n * W;
    Timer t(c, &c->tm.ms_other, &c->tm.n_other);
    hipLaunchKernelGGL(fz::k_sparse_gather, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)plane, n, M, nbr, nn,
                       (int)W, (unsigned long long)fill, (unsigned long long)pad, (unsigned long long*)out);
    HIPCHK(hipGetLastError());
    return 0;
}

static uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }

// the selection's own outputs, staged chunk by chunk
struct SparseArgs {
    StageRows nv, cv, vv, lmv, lev, lkv;
    SparseArgs(fz_ctx* c, int64_t W, int64_t* neighbors, int64_t* nnbr, double* vals, double* lmap, double* levid, double* lnkept)
        : nv(c, neighbors, (size_t)W * 8, c->d_draw[0], STAGE_OUT), cv(c, nnbr, 8, c->d_draw[1], STAGE_OUT),
          vv(c, vals, (size_t)W * 8, c->d_sparse[1], STAGE_OUT), lmv(c, lmap, 8, c->d_lmap, STAGE_OUT), lev(c, levid, 8, c->d_levid, STAGE_OUT),
          lkv(c, lnkept, 8, c->d_sparse[0], STAGE_OUT) {}
    int64_t staged_bytes_per_obj() const { return (int64_t)((nv.staged() ? nv.row : 0) + (vv.staged() ? vv.row : 0) + 32); }
    // selects on `rows`; *dn / *dc: the chunk's neighbours and counts on the device, for the gathers
    int run(fz_ctx* c, int64_t i0, int64_t n, int64_t L, const double* rows, int64_t W, double lncut, int64_t** dn, int64_t** dc) const {
        double *dv, *dm, *de, *dk;
        FZCHK(nv.at(i0, n, dn)); FZCHK(cv.at(i0, n, dc)); FZCHK(vv.at(i0, n, &dv)); FZCHK(lmv.at(i0, n, &dm)); FZCHK(lev.at(i0, n, &de));
        FZCHK(lkv.at(i0, n, &dk));
        FZCHK(run_sparse_select(c, n, L, rows, W, lncut, *dn, *dc, dv, dm, de, dk));
        FZCHK(nv.back(i0, n)); FZCHK(cv.back(i0, n)); FZCHK(vv.back(i0, n)); FZCHK(lmv.back(i0, n)); FZCHK(lev.back(i0, n)); FZCHK(lkv.back(i0, n));
        return 0;
    }
};

extern "C" int fz_sparsify_logwt(fz_ctx* c, const double* logwt, int64_t N, int64_t M, int64_t W, double lncut, int64_t* neighbors, int64_t* nnbr,
                                 double* vals, double* lmap, double* levid, double* lnkept) {
    if (!c || !logwt || !neighbors || !nnbr) return fail(-1, "fz_sparsify_logwt: NULL argument");
    FZCHK(sparse_limits("fz_sparsify_logwt", M, W, lncut));
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {logwt, neighbors, nnbr, vals, lmap, levid, lnkept}));
    const StageRows rv(c, logwt, (size_t)M * 8, c->d_draw[2], STAGE_IN);
    const SparseArgs sa(c, W, neighbors, nnbr, vals, lmap, levid, lnkept);
    const int64_t per_obj = (rv.staged() ? M * 8 : 0) + sa.staged_bytes_per_obj();
    int64_t nc = std::max<int64_t>(1, c->ws_limit / per_obj);
    nc = std::min<int64_t>(std::min<int64_t>(nc, N), 1 << 18);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dr; int64_t *dn, *dc;
        FZCHK(rv.at(i0, n, &dr));
        FZCHK(sa.run(c, i0, n, M, dr, W, lncut, &dn, &dc));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// objects -> sparse rows with the built-in likelihood: fz_fit's planes (chunk_planes) as far as asked for, the selection on the
// ln-prob plane and one gather per other plane
extern "C" int fz_fit_sparse(fz_ctx* c, double* x, double* xe, double* xm, int64_t N, const fz_like_opts* o, const fz_prior_lerp* pr, int64_t W,
                             double lncut, int64_t* neighbors, int64_t* nnbr, double* lnprior, double* lnlike, double* lnprob, double* chi2,
                             int64_t* ndim, double* scale, double* scale_err, double* lmap, double* levid, double* lnkept) {
    if (!c || !x || !xe || !xm || !o || !neighbors || !nnbr) return fail(-1, "fz_fit_sparse: NULL argument");
    if (!c->M) return fail(-1, "fz_fit_sparse: models have not been uploaded");
    FZCHK(sparse_limits("fz_fit_sparse", c->M, W, lncut));
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {x, xe, xm, pr ? pr->table : nullptr, pr ? pr->rows : nullptr, pr ? pr->frac : nullptr, neighbors, nnbr, lnprior,
                                 lnlike, lnprob, chi2, ndim, scale, scale_err, lmap, levid, lnkept}));
    const int mode = eff_mode(c, like_mode(o));
    const int64_t M = c->M;
    PriorBind pb; PriorGuard guard{c};
    FZCHK(prior_begin(c, pr, N, M, pb));
    const bool has_prior = pb.kind != 0;
    const SparseArgs sa(c, W, neighbors, nnbr, lnprob, lmap, levid, lnkept);
    // planes formed per chunk: ln-like always; chi2, N_dim, scale, its error when asked for; with a prior the ln-prior when asked for
    // and a ln-prob plane of its own when the ln-like is asked for too (else the sum is formed in place)
    const bool own_lnprob = has_prior && lnlike;
    const int nplanes = 1 + (chi2 ? 1 : 0) + (ndim ? 1 : 0) + (scale ? 1 : 0) + (scale_err ? 1 : 0) + (has_prior && lnprior ? 1 : 0) + (own_lnprob ? 1 : 0);
    // the gathered rows of one plane at a time go through one buffer (each is copied back before the next is formed)
    void* gouts[6] = {lnprior, lnlike, chi2, ndim, scale, scale_err};
    bool gstaged = false;
    for (void* p : gouts) gstaged |= p && !is_device_ptr(p);
    const int64_t per_obj = M * 8 * (nplanes + (mode == 3 ? 4 : 0)) + pb.chunk_bytes_per_obj + sa.staged_bytes_per_obj() + (gstaged ? W * 8 : 0);
    int64_t nc = std::min<int64_t>(N, fz_dbg_int("FZ_CHUNK", 1 << 18));
    nc = std::min<int64_t>(nc, std::max<int64_t>(1, c->ws_limit / per_obj));
    const uint64_t ninf = bits_of(-INFINITY), pinf = bits_of(INFINITY), one = bits_of(1.0), zero = bits_of(0.0);
    FZCHK(for_chunks(c, x, xe, xm, N, nc, o, pb, [&](int64_t i0, int64_t n, int var, int) -> int {
        const bool want[7] = {true, chi2 != nullptr, ndim != nullptr, scale != nullptr, scale_err != nullptr, has_prior && lnprior, own_lnprob};
        void* pl[7];
        for (int k = 0; k < 7; ++k) {
            if (want[k]) FZCHK(c->d_pl[k].ensure((size_t)n * M * 8));
            pl[k] = want[k] ? c->d_pl[k].p : nullptr;
        }
        Planes p; p.lnl = (double*)pl[0]; p.chi2 = (double*)pl[1]; p.ndim = (int64_t*)pl[2]; p.scale = (double*)pl[3];
        p.serr = (double*)pl[4]; p.lnprior = (double*)pl[5];
        if (has_prior) p.lnprob = own_lnprob ? (double*)pl[6] : p.lnl;
        FZCHK(chunk_planes(c, mode, var, n, o, p));
        int64_t *dn, *dc;
        FZCHK(sa.run(c, i0, n, M, has_prior ? p.lnprob : p.lnl, W, lncut, &dn, &dc));
        // (without a prior the ln-prior of a kept entry is 0 and ln-prob is the ln-like: bruteforce.py:195-203 through pdf.py:404-405)
        const void* gplanes[6] = {p.lnprior, p.lnl, p.chi2, p.ndim, p.scale, p.serr};      // (p.lnl is intact whenever lnlike is asked for)
        const uint64_t gpads[6] = {ninf, ninf, pinf, 0, one, zero};
        for (int k = 0; k < 6; ++k) {
            if (!gouts[k]) continue;
            const StageRows gv(c, gouts[k], (size_t)W * 8, c->d_sparse[2], STAGE_OUT);
            void* dg;
            FZCHK(gv.at(i0, n, &dg));
            FZCHK(run_sparse_gather(c, gplanes[k], n, M, dn, dc, W, zero, gpads[k], dg));
            FZCHK(gv.back(i0, n));
        }
        return 0;
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
