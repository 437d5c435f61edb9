// Host side of fz_pdfs_summarize / fz_overlap_nz (kernels in fz_summary.h).

extern "C" int fz_pdfs_summarize(fz_ctx* c, double* pdfs, int64_t N, int64_t G, const double* pgrid, int32_t renormalize,
                                 const double* urand, const double* loss, const double* widths, double wconf_scale,
                                 double* stats) {
    if (!c || !pdfs || !pgrid || !urand || !loss || !stats) return fail(-1, "fz_pdfs_summarize: NULL argument");
    if (G < 2 || G > FZ_SUM_MAXG) return fail(-5, "fz_pdfs_summarize: grid of %lld points unsupported (2..%d)", (long long)G, FZ_SUM_MAXG);
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, pgrid, urand, loss, widths, stats}));
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, renormalize ? STAGE_INOUT : STAGE_IN);      // renormalised in place, pdf.py:985
    const StageRows uv(c, urand, 8, c->d_lmap, STAGE_IN), wv(c, widths, 32, c->d_levid, STAGE_IN);
    const bool s_dev = is_device_ptr(stats);
    // resident for the whole call: grid and loss matrix
    FZCHK(c->d_sgrid.ensure((size_t)G * 8)); FZCHK(copy_in(c, c->d_sgrid.p, pgrid, (size_t)G * 8));
    const double* d_loss = loss;
    if (!is_device_ptr(loss)) { FZCHK(c->d_sloss.ensure((size_t)G * G * 8)); FZCHK(copy_in(c, c->d_sloss.p, loss, (size_t)G * G * 8)); d_loss = c->d_sloss.as<double>(); }
    // chunk: staged pdf rows (if on the host) + risk rows + outputs
    const int64_t per_obj = G * 8 * (pv.dev ? 1 : 2) + 21 * 8 + 5 * 8;
    int64_t nc = std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / per_obj, (int64_t)1 << 20));
    nc = std::min(nc, N);
    const size_t lds_g = (size_t)2 * 2 * FZ_GEMM_BK * FZ_GEMM_LD * 8;
    const int swpb = G <= 4800 ? 4 : (G <= 9600 ? 2 : 1);               // waves (= objects) per block of k_summarize: one CDF row each in LDS
    const size_t lds_s = (size_t)swpb * G * 8;
    HIPCHK(hipFuncSetAttribute((const void*)k_gemm_f64, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_g));
    HIPCHK(hipFuncSetAttribute((const void*)k_summarize, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_s));
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        double* dp; const double* du; const double* dw;
        FZCHK(pv.at(i0, n, &dp)); FZCHK(uv.at(i0, n, &du)); FZCHK(wv.at(i0, n, &dw));
        FZCHK(c->d_pl[0].ensure((size_t)n * G * 8));                    // risk rows
        double* dr = c->d_pl[0].as<double>();
        double* ds; int64_t ostride;
        if (s_dev) { ds = stats + i0; ostride = N; }
        else { FZCHK(c->d_pl[1].ensure((size_t)n * 21 * 8)); ds = c->d_pl[1].as<double>(); ostride = n; }
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            if (renormalize) hipLaunchKernelGGL(k_rownorm, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, dp, n, (int)G);
            dim3 grid((unsigned)((n + FZ_GEMM_BM - 1) / FZ_GEMM_BM), (unsigned)((G + FZ_GEMM_BN - 1) / FZ_GEMM_BN));
            hipLaunchKernelGGL(k_gemm_f64, grid, dim3(256), lds_g, c->stream, dp, G, d_loss, G, dr, G, n, (int)G, (int)G);
            hipLaunchKernelGGL(k_summarize, dim3((unsigned)((n + swpb - 1) / swpb)), dim3(swpb * 64), lds_s, c->stream, dp, dr, n, (int)G,
                               c->d_sgrid.as<double>(), du, dw, wconf_scale, ostride, ds);
        }
        HIPCHK(hipGetLastError());
        FZCHK(pv.back(i0, n));
        if (!s_dev) for (int r = 0; r < 21; ++r) FZCHK(copy_out(c, stats + r * N + i0, ds + r * n, (size_t)n * 8));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_overlap_nz(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, const double* nz, int64_t pair_i, int64_t pair_j,
                             double pair_step, double* overlap, double* lnlike) {
    if (!c || !pdfs || !nz || !overlap || !lnlike) return fail(-1, "fz_overlap_nz: NULL argument");
    if (N <= 0 || G <= 0) return fail(-1, "fz_overlap_nz: bad shape");
    if ((pair_i >= 0) != (pair_j >= 0) || pair_i >= G || pair_j >= G) return fail(-3, "fz_overlap_nz: pair index out of range");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, nz, overlap, lnlike}));
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_IN), ov(c, overlap, 8, c->d_lmap, STAGE_OUT);
    FZCHK(c->d_sgrid.ensure((size_t)G * 8)); FZCHK(copy_in(c, c->d_sgrid.p, nz, (size_t)G * 8));
    int64_t nc = pv.dev ? N : std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / (G * 8 + 16), (int64_t)1 << 22));
    nc = std::min(nc, N);
    const int64_t nblk_max = (nc + 3) / 4;
    FZCHK(c->d_pl[1].ensure((size_t)nblk_max * 8 + 64));
    double total = 0.0;
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dp; double* dov;
        FZCHK(pv.at(i0, n, &dp)); FZCHK(ov.at(i0, n, &dov));
        const int64_t nblk = (n + 3) / 4;
        double* part = c->d_pl[1].as<double>();
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            hipLaunchKernelGGL(k_overlap, dim3((unsigned)nblk), dim3(256), 0, c->stream, dp, n, (int)G, c->d_sgrid.as<double>(),
                               (int)pair_i, (int)pair_j, pair_step, dov, part);
            hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, part, nblk, part + nblk_max);
        }
        HIPCHK(hipGetLastError());
        double chunk = 0.0;
        FZCHK(copy_out(c, &chunk, part + nblk_max, 8));
        total += chunk;
        FZCHK(ov.back(i0, n));
    }
    return host_write(lnlike, &total, 8);
}

extern "C" int fz_pdfs_resample(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, const double* old_grid, int64_t Gn,
                                const double* new_grid, double left, double right, int32_t renormalize, double* out) {
    if (!c || !pdfs || !old_grid || !new_grid || !out) return fail(-1, "fz_pdfs_resample: NULL argument");
    if (G < 1 || Gn < 1) return fail(-1, "fz_pdfs_resample: bad grid");
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, old_grid, new_grid, out}));
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_IN), ov(c, out, (size_t)Gn * 8, c->d_pl[0], STAGE_OUT);
    FZCHK(c->d_sgrid.ensure((size_t)(G + Gn) * 8));
    FZCHK(copy_in(c, c->d_sgrid.p, old_grid, (size_t)G * 8));
    FZCHK(copy_in(c, c->d_sgrid.as<double>() + G, new_grid, (size_t)Gn * 8));
    int64_t nc = std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / ((G + Gn) * 8), (int64_t)1 << 20));
    nc = std::min(nc, N);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dp; double* dout;
        FZCHK(pv.at(i0, n, &dp)); FZCHK(ov.at(i0, n, &dout));
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            hipLaunchKernelGGL(k_resample, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, dp, n, (int)G, c->d_sgrid.as<double>(),
                               (int)Gn, c->d_sgrid.as<double>() + G, left, right, renormalize, dout);
        }
        HIPCHK(hipGetLastError());
        FZCHK(ov.back(i0, n));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}


// samplers.py:498-499 / 519-520: one categorical draw per object from pdf_i * nz (inverse CDF on the caller's uniforms)
extern "C" int fz_nz_assign(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, const double* nz, const double* u,
                            int64_t* bins, int64_t* counts) {
    if (!c || !pdfs || !nz || !u || !counts) return fail(-1, "fz_nz_assign: NULL argument");
    if (N <= 0 || G <= 0 || G >= ((int64_t)1 << 24)) return fail(-1, "fz_nz_assign: bad shape");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, nz, u, bins, counts}));
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_IN), uv(c, u, 8, c->d_lmap, STAGE_IN), bv(c, bins, 8, c->d_levid, STAGE_OUT, true);
    const bool c_dev = is_device_ptr(counts);
    FZCHK(c->d_sgrid.ensure((size_t)G * 8)); FZCHK(copy_in(c, c->d_sgrid.p, nz, (size_t)G * 8));
    FZCHK(c->d_sloss.ensure((size_t)G * 8));
    HIPCHK(hipMemsetAsync(c->d_sloss.p, 0, (size_t)G * 8, c->stream));
    int64_t nc = pv.dev ? N : std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / (G * 8 + 32), (int64_t)1 << 22));
    nc = std::min(nc, N);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dp; const double* du; int64_t* db;
        FZCHK(pv.at(i0, n, &dp)); FZCHK(uv.at(i0, n, &du)); FZCHK(bv.at(i0, n, &db));
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            const size_t rows_lds = (size_t)4 * G * 8;          // four rows of p * nz (up to 48 KB: grids of 1 536 points; longer: no staging)
            const int staged = rows_lds <= 48 * 1024;
            hipLaunchKernelGGL(k_nz_assign, dim3((unsigned)((n + 3) / 4)), dim3(256), staged ? rows_lds : 0, c->stream, dp, n, (int)G,
                               c->d_sgrid.as<double>(), du, db, c->d_sloss.as<unsigned long long>(), staged);
        }
        HIPCHK(hipGetLastError());
        FZCHK(bv.back(i0, n));
    }
    if (c_dev) HIPCHK(hipMemcpyAsync(counts, c->d_sloss.p, (size_t)G * 8, hipMemcpyDeviceToDevice, c->stream));
    else FZCHK(copy_out(c, counts, c->d_sloss.p, (size_t)G * 8));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
