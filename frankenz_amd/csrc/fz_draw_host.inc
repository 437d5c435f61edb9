// Host side of the posterior draws (fz_draw.h; docs/draws.md): fz_draw_logwt, fz_fit_draw, fz_knn_search_fit_draw.
// Included by frankenz_hip.hip after the entry points it builds on (for_chunks, chunk_lnprob_rows, prior_*, the k-NN calls).

static int draw_limits(const char* who, int64_t L, int64_t S) {
    if (S < 1) return fail(-4, "%s: Nsamples = %lld, need at least 1", who, (long long)S);
    if (S > FZ_DRAW_SMAX) return fail(-5, "%s: Nsamples = %lld exceeds FZ_DRAW_SMAX = %d", who, (long long)S, FZ_DRAW_SMAX);
    if (L < 1) return fail(-4, "%s: rows of %lld entries", who, (long long)L);
    if (L > FZ_DRAW_LMAX) return fail(-5, "%s: rows of %lld entries exceed FZ_DRAW_LMAX = %d", who, (long long)L, FZ_DRAW_LMAX);
    return 0;
}

// n rows of L ln-weights in device memory -> idx (n, S), lmap, levid (device; the last two may be nullptr).  u (n, S) on the device, or
// nullptr: Philox under (k0, k1), object `first` + row.  The geometry is row_geometry's.
static int run_draw(fz_ctx* c, int64_t n, int64_t L, const double* rows, const int64_t* nbr, const int64_t* nnb, const double* u, uint32_t k0,
                    uint32_t k1, int64_t first, int64_t S, int64_t* idx, double* lmap, double* levid) {
    if (u) {
        int bad = 0;
        const int64_t tot = n * S;
        FZCHK(fz_flag_roundtrip(c, bad, [&](int* d_flags) {
            hipLaunchKernelGGL(fz::k_draw_check_u, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, u, tot, d_flags);
            return 0;
        }));
        if (bad) return fail(-4, "posterior draws: a uniform outside [0, 1]");
    }
    const RowGeometry geo = row_geometry(L);
    size_t lds;
    FZCHK(geo.seg_lds("posterior draws", L, &lds));
    const void* kern = geo.wpo == 1 ? (const void*)fz::k_draw<1> : (const void*)fz::k_draw<4>;
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int ef = 0;
    FZCHK(fz_flag_roundtrip(c, ef, [&](int* d_flags) {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        const dim3 grid = geo.grid(n), blk(256);
        if (geo.wpo == 1) hipLaunchKernelGGL(fz::k_draw<1>, grid, blk, lds, c->stream, rows, n, L, nbr, nnb, u, k0, k1, first, (int)S, idx, lmap, levid, d_flags);
        else hipLaunchKernelGGL(fz::k_draw<4>, grid, blk, lds, c->stream, rows, n, L, nbr, nnb, u, k0, k1, first, (int)S, idx, lmap, levid, d_flags);
        return 0;
    }));
    if (ef) return fail(-3, "posterior draws: Nneighbors outside [0, %lld]", (long long)L);
    return 0;
}

// the draw's own arguments, staged chunk by chunk: u in, idx / lmap / levid out
struct DrawArgs {
    StageRows uv, iv, lmv, lev;
    DrawArgs(fz_ctx* c, const double* u, int64_t S, int64_t* idx, double* lmap, double* levid)
        : uv(c, u, (size_t)S * 8, c->d_draw[4], STAGE_IN), iv(c, idx, (size_t)S * 8, c->d_draw[5], STAGE_OUT),
          lmv(c, lmap, 8, c->d_lmap, STAGE_OUT), lev(c, levid, 8, c->d_levid, STAGE_OUT) {}
    int64_t staged_bytes_per_obj() const { return (int64_t)((uv.staged() ? uv.row : 0) + (iv.staged() ? iv.row : 0) + 16); }
    int run(fz_ctx* c, int64_t i0, int64_t n, int64_t L, const double* rows, const int64_t* nbr, const int64_t* nnb, uint32_t k0, uint32_t k1,
            int64_t first, int64_t S) const {
        const double* du; int64_t* di; double *dm, *de;
        FZCHK(uv.at(i0, n, &du)); FZCHK(iv.at(i0, n, &di)); FZCHK(lmv.at(i0, n, &dm)); FZCHK(lev.at(i0, n, &de));
        FZCHK(run_draw(c, n, L, rows, nbr, nnb, du, k0, k1, first + i0, S, di, dm, de));
        FZCHK(iv.back(i0, n)); FZCHK(lmv.back(i0, n)); FZCHK(lev.back(i0, n));
        return 0;
    }
};

extern "C" int fz_draw_logwt(fz_ctx* c, const double* logwt, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr,
                             const double* u, uint32_t key0, uint32_t key1, int64_t first, int64_t S, int64_t* idx, double* lmap,
                             double* levid) {
    if (!c || !logwt || !idx) return fail(-1, "fz_draw_logwt: NULL argument");
    FZCHK(rows_together("fz_draw_logwt", neighbors, nnbr));
    FZCHK(draw_limits("fz_draw_logwt", W, S));
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {logwt, neighbors, nnbr, u, idx, lmap, levid}));
    RowsIn in(c, logwt, neighbors, nnbr, W, c->d_draw[2], c->d_draw[0], c->d_draw[1]);
    DrawArgs da(c, u, S, idx, lmap, levid);
    FZCHK(for_row_chunks(c, N, in, {&da.uv, &da.iv, &da.lmv, &da.lev}, [&](int64_t i0, int64_t n) {
        return run_draw(c, n, W, in.rows(), in.nbr(), in.nnb(), da.uv.as<const double>(), key0, key1, first + i0, S, da.iv.as<int64_t>(),
                        da.lmv.as<double>(), da.lev.as<double>());
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// objects -> draws with the built-in likelihood: the ln-prob rows of fit_predict_impl's CDF rule (chunk_lnprob_rows), chunked from the
// workspace limit in the same way, with the draw kernel as the rows' consumer
extern "C" int fz_fit_draw(fz_ctx* c, double* x, double* xe, double* xm, int64_t N, const fz_like_opts* o, const fz_prior_lerp* pr,
                           const double* u, uint32_t key0, uint32_t key1, int64_t first, int64_t S, int64_t* idx, double* lmap,
                           double* levid) {
    if (!c || !x || !xe || !xm || !o || !idx) return fail(-1, "fz_fit_draw: NULL argument");
    if (!c->M) return fail(-1, "fz_fit_draw: models have not been uploaded");
    FZCHK(draw_limits("fz_fit_draw", c->M, S));
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {x, xe, xm, pr ? pr->table : nullptr, pr ? pr->rows : nullptr, pr ? pr->frac : nullptr, u, idx, lmap, levid}));
    const int mode = eff_mode(c, like_mode(o));
    const int64_t M = c->M;
    PriorBind pb; PriorGuard guard{c};
    FZCHK(prior_begin(c, pr, N, M, pb));
    const DrawArgs da(c, u, S, idx, lmap, levid);
    int64_t nc = std::min<int64_t>(N, fz_dbg_int("FZ_CHUNK", 1 << 20));
    const int64_t per_obj = M * 8 * (mode == 3 ? 4 : 1) + pb.chunk_bytes_per_obj + da.staged_bytes_per_obj();
    nc = std::min<int64_t>(nc, std::max<int64_t>(1, c->ws_limit / per_obj));
    FZCHK(for_chunks(c, x, xe, xm, N, nc, o, pb, [&](int64_t i0, int64_t n, int var, int) -> int {
        double* lpl; bool in_kernel;
        FZCHK(chunk_lnprob_rows(c, mode, var, n, o, &lpl, &in_kernel));
        return da.run(c, i0, n, M, lpl, nullptr, nullptr, key0, key1, first, S);
    }));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// query features + objects -> draws over each object's neighbour subset, without the KDE half: per chunk the searches and the subset
// likelihood of fz_knn_search_fit_predict_prior_lerp (its padded ln-prob rows, neighbours and counts stay on the device), then the
// draw kernel on those rows.  neighbors (N, K k) / nnbr (N): optional outputs, as there.
extern "C" int fz_knn_search_fit_draw(fz_ctx* c, const double* q, double* x, double* xe, double* xm, int64_t N, int32_t k, double lp_norm,
                                      double dub, const fz_like_opts* o, const fz_prior_lerp* pr, const double* u, uint32_t key0,
                                      uint32_t key1, int64_t first, int64_t S, int64_t* neighbors, int64_t* nnbr, int64_t* idx,
                                      double* lmap, double* levid) {
    if (!c || !q || !x || !xe || !xm || !o || !idx) return fail(-1, "fz_knn_search_fit_draw: NULL argument");
    if (!c->knn_K) return fail(-1, "fz_knn_search_fit_draw: feature sets have not been uploaded");
    if (k <= 0) return fail(-5, "fz_knn_search_fit_draw: k=%d unsupported", k);
    const int64_t W = (int64_t)c->knn_K * k, M = c->M;
    const int F = c->knn_F, B = c->B;
    FZCHK(draw_limits("fz_knn_search_fit_draw", W, S));
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    const bool has_prior = pr && pr->table;
    const DrawArgs da(c, u, S, idx, lmap, levid);
    const int64_t nc = std::min<int64_t>(N, std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / (W * 48 + da.staged_bytes_per_obj()), knn_search_chunk_cap())));
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        FZCHK(c->d_draw[0].ensure((size_t)n * W * 8)); FZCHK(c->d_draw[1].ensure((size_t)n * 8)); FZCHK(c->d_draw[2].ensure((size_t)n * W * 8));
        if (has_prior) FZCHK(c->d_draw[3].ensure((size_t)n * W * 8));
        int64_t* d_nb = c->d_draw[0].as<int64_t>(); int64_t* d_nn = c->d_draw[1].as<int64_t>();
        double* d_lnl = c->d_draw[2].as<double>(); double* d_lpr = has_prior ? c->d_draw[3].as<double>() : nullptr;
        fz_prior_lerp pc;
        if (has_prior) FZCHK(prior_slice(pr, i0, n, N, M, &pc));
        FZCHK(fz_knn_search_fit_predict_prior_lerp(c, q + i0 * F, x + i0 * B, xe + i0 * B, xm + i0 * B, n, k, lp_norm, dub, o, nullptr, has_prior ? &pc : nullptr, d_nb,
                                                   d_nn, nullptr, d_lnl, d_lpr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
        FZCHK(da.run(c, i0, n, W, has_prior ? d_lpr : d_lnl, d_nb, d_nn, key0, key1, first, S));
        if (neighbors) FZCHK(copy_out(c, neighbors + i0 * W, d_nb, (size_t)n * W * 8));
        if (nnbr) FZCHK(copy_out(c, nnbr + i0, d_nn, (size_t)n * 8));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
