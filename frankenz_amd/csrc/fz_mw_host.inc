// Host side of the model-weight sampler (fz_mw.h; docs/model_weights.md): fz_mw_sweep, fz_mw_dirichlet, fz_mw_chain.
// Included by frankenz_hip.hip after fz_rows_host.inc (geometry, mw_limits, the error flags, the chunk loop), fz_draw_host.inc and
// fz_nzmc_host.inc.

namespace {
int mw_flags_check(fz_ctx* c, const char* who, int64_t W, int64_t M) {
    int ef;
    FZCHK(mw_flags_read(c, &ef));
    if (ef & FZ_MW_ERR_ALPHA) return fail(-4, "%s: alpha must be finite and positive", who);
    FZCHK(row_flags_check(who, ef, W, M));
    if (ef & FZ_MW_ERR_TRIES) return fail(-7, "%s: a gamma draw was not accepted within %d attempts", who, FZ_MW_TRIES);
    if (ef & FZ_MW_ERR_ZERO) return fail(-7, "%s: every gamma draw underflowed to 0 (alpha too small for these counts): no weights to normalise", who);
    return 0;
}
// One of the two gathered-row kernels (k_mw_sweep, k_mw_em_rows) over n device rows of L entries, enqueued.  kern: its forms <1, REG>,
// <1>, <4>.  The geometry is row_geometry's with the segment tables' LDS; short rows (every default k-NN row) stay in registers
// (FZ_MW_REG=0: the re-reading form; the results are the same).
template <class K, class... A>
int mw_launch_rows(fz_ctx* c, int64_t n, int64_t L, K* const (&kern)[3], A... args) {
    const RowGeometry geo = row_geometry(L);
    size_t lds;
    FZCHK(geo.seg_lds("model weights", L, &lds));
    const bool reg = geo.wpo == 1 && L <= FZ_MW_REG_LMAX && fz_dbg_int("FZ_MW_REG", 1) != 0;
    K* const k = kern[reg ? 0 : geo.wpo == 1 ? 1 : 2];
    HIPCHK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, geo.grid(n), dim3(256), lds, c->stream, args...);
    return 0;
}
// one sweep over n device rows, enqueued
int mw_launch_sweep(fz_ctx* c, int64_t n, int64_t L, const double* rows, const int64_t* nbr, const int64_t* nnb, int64_t M, const double* lnw,
                    const double* u, uint32_t k0, uint32_t k1, int64_t first, uint64_t sweep, unsigned long long* counts, int64_t* assign,
                    int* d_flags) {
    decltype(fz::k_mw_sweep<1, true>)* const kern[3] = {fz::k_mw_sweep<1, true>, fz::k_mw_sweep<1, false>, fz::k_mw_sweep<4, false>};
    return mw_launch_rows(c, n, L, kern, rows, n, L, nbr, nnb, M, lnw, u, k0, k1, first, sweep, counts, assign, d_flags);
}
// the Dirichlet step, enqueued: pos (M) and lnw (M) from alpha and counts; scratch d_mw[1] (block partials and their sum)
int mw_launch_dirichlet(fz_ctx* c, const double* alpha, const unsigned long long* counts, int64_t M, uint32_t k0, uint32_t k1, uint64_t sweep,
                        double* pos, double* lnw, int* d_flags) {
    const int64_t nblk = (M + NZ_NT - 1) / NZ_NT;
    FZCHK(c->d_mw[1].ensure((size_t)(nblk + 1) * 8));
    double* part = c->d_mw[1].as<double>();
    hipLaunchKernelGGL(fz::k_mw_gamma, dim3((unsigned)nblk), dim3(NZ_NT), 0, c->stream, alpha, counts, M, k0, k1, sweep, pos, part, d_flags);
    hipLaunchKernelGGL(fz::k_mw_gsum, dim3(1), dim3(NZ_NT), 0, c->stream, part, nblk, d_flags);
    hipLaunchKernelGGL(fz::k_mw_norm, dim3((unsigned)nblk), dim3(NZ_NT), 0, c->stream, (const double*)pos, M, (const double*)(part + nblk), pos, lnw);
    return 0;
}
}  // namespace

extern "C" int fz_mw_sweep(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                           const double* lnw, const double* u, uint32_t key0, uint32_t key1, int64_t first, uint64_t sweep, int64_t* counts,
                           int64_t* assign) {
    if (!c || !rows || !lnw || !counts) return fail(-1, "fz_mw_sweep: NULL argument");
    FZCHK(rows_entry("fz_mw_sweep", neighbors, nnbr, N, W, M));
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, lnw, u, counts, assign}));
    RowsIn in(c, rows, neighbors, nnbr, W, c->d_draw[2], c->d_draw[0], c->d_draw[1]);
    StageRows uv(c, u, 8, c->d_draw[4], STAGE_IN), av(c, assign, 8, c->d_draw[5], STAGE_OUT);
    StageWhole st{c};
    const void* d_lnw; void* d_counts;
    FZCHK(st.in(lnw, (size_t)M * 8, &d_lnw)); FZCHK(st.out(counts, (size_t)M * 8, &d_counts));
    HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)M * 8, c->stream));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    FZCHK(for_row_chunks(c, N, in, {&uv, &av}, [&](int64_t i0, int64_t n) {
        const double* du = uv.as<const double>();
        if (du) {
            int bad = 0;
            FZCHK(fz_flag_roundtrip(c, bad, [&](int* df) {
                hipLaunchKernelGGL(fz::k_draw_check_u, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, du, n, df);
                return 0;
            }));
            if (bad) return fail(-4, "fz_mw_sweep: a uniform outside [0, 1]");
        }
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        return mw_launch_sweep(c, n, W, in.rows(), in.nbr(), in.nnb(), M, (const double*)d_lnw, du, key0, key1, first + i0, sweep,
                               (unsigned long long*)d_counts, av.as<int64_t>(), d_flags);
    }));
    FZCHK(mw_flags_check(c, "fz_mw_sweep", W, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_mw_dirichlet(fz_ctx* c, const double* alpha, const int64_t* counts, int64_t M, uint32_t key0, uint32_t key1, uint64_t sweep,
                               double* pos, double* lnw) {
    if (!c || !alpha || !counts || !pos || !lnw) return fail(-1, "fz_mw_dirichlet: NULL argument");
    FZCHK(mw_limits("fz_mw_dirichlet", 1, M, false));
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {alpha, counts, pos, lnw}));
    StageWhole st{c};
    const void *d_al, *d_cn; void *d_pos, *d_lnw;
    FZCHK(st.in(alpha, (size_t)M * 8, &d_al)); FZCHK(st.in(counts, (size_t)M * 8, &d_cn));
    FZCHK(st.out(pos, (size_t)M * 8, &d_pos)); FZCHK(st.out(lnw, (size_t)M * 8, &d_lnw));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        FZCHK(mw_launch_dirichlet(c, (const double*)d_al, (const unsigned long long*)d_cn, M, key0, key1, sweep, (double*)d_pos, (double*)d_lnw, d_flags));
    }
    FZCHK(mw_flags_check(c, "fz_mw_dirichlet", 1, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_mw_chain(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                           const double* alpha, double* lnw, uint32_t key0, uint32_t key1, int64_t first, uint64_t sweep0, int32_t nsweeps,
                           int64_t* counts, double* pos, int64_t* counts_all) {
    if (!c || !rows || !alpha || !lnw || !counts || !pos) return fail(-1, "fz_mw_chain: NULL argument");
    FZCHK(rows_together("fz_mw_chain", neighbors, nnbr));
    FZCHK(mw_limits("fz_mw_chain", W, M, neighbors == nullptr));
    if (N <= 0 || nsweeps < 1) return fail(-4, "fz_mw_chain: %lld objects, %d sweeps", (long long)N, (int)nsweeps);
    if (!is_device_ptr(rows) || (neighbors && (!is_device_ptr(neighbors) || !is_device_ptr(nnbr))))
        return fail(-4, "fz_mw_chain: rows, neighbors and nnbr must be device arrays (they stay resident over the chain)");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, alpha, lnw, counts, pos, counts_all}));
    StageWhole st{c};
    const void* d_al; void *d_lnw, *d_cn, *d_pos, *d_all;
    FZCHK(st.in(alpha, (size_t)M * 8, &d_al)); FZCHK(st.inout(lnw, (size_t)M * 8, &d_lnw));
    FZCHK(st.out(counts, (size_t)M * 8, &d_cn)); FZCHK(st.out(pos, (size_t)M * 8, &d_pos));
    FZCHK(st.out(counts_all, (size_t)nsweeps * M * 8, &d_all));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    {
        // the whole chain is enqueued without a host synchronisation: the order of the stream is the chain's order
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        for (int32_t s = 0; s < nsweeps; ++s) {
            unsigned long long* cn = d_all ? (unsigned long long*)d_all + (size_t)s * M : (unsigned long long*)d_cn;
            HIPCHK(hipMemsetAsync(cn, 0, (size_t)M * 8, c->stream));
            FZCHK(mw_launch_sweep(c, N, W, rows, neighbors, nnbr, M, (const double*)d_lnw, nullptr, key0, key1, first, sweep0 + (uint64_t)s, cn, nullptr,
                                  d_flags));
            FZCHK(mw_launch_dirichlet(c, (const double*)d_al, cn, M, key0, key1, sweep0 + (uint64_t)s, (double*)d_pos, (double*)d_lnw, d_flags));
        }
        if (d_all) HIPCHK(hipMemcpyAsync(d_cn, (char*)d_all + (size_t)(nsweeps - 1) * M * 8, (size_t)M * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    FZCHK(mw_flags_check(c, "fz_mw_chain", W, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
