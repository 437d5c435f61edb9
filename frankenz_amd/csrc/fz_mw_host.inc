// Host side of the model-weight sampler (fz_mw.h; docs/model_weights.md): fz_mw_sweep, fz_mw_dirichlet, fz_mw_chain.
// Included by frankenz_hip.hip after fz_draw_host.inc (draw geometry, k_draw_check_u) and fz_nzmc_host.inc.

namespace {
int mw_limits(const char* who, int64_t W, int64_t M, bool dense) {
    if (W < 1 || M < 1) return fail(-4, "%s: rows of %lld entries over %lld models", who, (long long)W, (long long)M);
    if (W > FZ_DRAW_LMAX) return fail(-5, "%s: rows of %lld entries exceed FZ_DRAW_LMAX = %d", who, (long long)W, FZ_DRAW_LMAX);
    if (M >= ((int64_t)1 << 31)) return fail(-5, "%s: %lld models, the limit is M < 2^31 (FZ_MW_MMAX)", who, (long long)M);
    if (dense && W != M) return fail(-4, "%s: dense rows (no neighbors) have one entry per model: W = %lld, M = %lld", who, (long long)W, (long long)M);
    return 0;
}
// the error flags of a call: d_mw[0], zeroed here, read by mw_flags_check
int mw_flags_begin(fz_ctx* c, int** d_flags) {
    FZCHK(c->d_mw[0].ensure(64));
    HIPCHK(hipMemsetAsync(c->d_mw[0].p, 0, 64, c->stream));
    *d_flags = c->d_mw[0].as<int>();
    return 0;
}
int mw_flags_check(fz_ctx* c, const char* who, int64_t W, int64_t M) {
    int ef = 0;
    HIPCHK(hipGetLastError());
    FZCHK(copy_out(c, &ef, c->d_mw[0].p, sizeof(int)));
    if (ef & FZ_MW_ERR_ALPHA) return fail(-4, "%s: alpha must be finite and positive", who);
    if (ef & FZ_MW_ERR_NNB) return fail(-3, "%s: Nneighbors outside [0, %lld]", who, (long long)W);
    if (ef & FZ_MW_ERR_NBR) return fail(-3, "%s: a neighbour index outside [0, %lld)", who, (long long)M);
    if (ef & FZ_MW_ERR_TRIES) return fail(-7, "%s: a gamma draw was not accepted within %d attempts", who, FZ_MW_TRIES);
    if (ef & FZ_MW_ERR_ZERO) return fail(-7, "%s: every gamma draw underflowed to 0 (alpha too small for these counts): no weights to normalise", who);
    return 0;
}
// one sweep over n device rows, enqueued: the geometry is k_draw's, a function of L alone (FZ_DRAW_WPO = 1 / 4 forces one: tests)
int mw_launch_sweep(fz_ctx* c, int64_t n, int64_t L, const double* rows, const int64_t* nbr, const int64_t* nnb, int64_t M, const double* lnw,
                    const double* u, uint32_t k0, uint32_t k1, int64_t first, uint64_t sweep, unsigned long long* counts, int64_t* assign,
                    int* d_flags) {
    int wpo = L <= FZ_DRAW_WAVE_LMAX ? 1 : 4;
    const long long forced = fz_dbg_int("FZ_DRAW_WPO", 0);
    if (forced == 1 || forced == 4) wpo = (int)forced;
    const int opb = 4 / wpo;
    const size_t nsegL = (size_t)((L + FZ_DRAW_SEG - 1) / FZ_DRAW_SEG);
    const size_t lds = (FZ_DRAW_HDR + (size_t)opb * 2 * nsegL) * 8;
    if (lds > FZ_LDS_BYTES) return fail(-5, "model weights: rows of %lld entries need %zu bytes of LDS at this geometry", (long long)L, lds);
    // short rows (every default k-NN row): the row stays in registers (FZ_MW_REG=0: the re-reading form; the draws are the same)
    const bool reg = wpo == 1 && L <= FZ_MW_REG_LMAX && fz_dbg_int("FZ_MW_REG", 1) != 0;
    const void* kern = reg ? (const void*)fz::k_mw_sweep<1, true> : wpo == 1 ? (const void*)fz::k_mw_sweep<1, false> : (const void*)fz::k_mw_sweep<4, false>;
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const dim3 grid((unsigned)((n + opb - 1) / opb)), blk(256);
    if (reg) hipLaunchKernelGGL((fz::k_mw_sweep<1, true>), grid, blk, lds, c->stream, rows, n, L, nbr, nnb, M, lnw, u, k0, k1, first, sweep, counts, assign, d_flags);
    else if (wpo == 1) hipLaunchKernelGGL((fz::k_mw_sweep<1, false>), grid, blk, lds, c->stream, rows, n, L, nbr, nnb, M, lnw, u, k0, k1, first, sweep, counts, assign, d_flags);
    else hipLaunchKernelGGL((fz::k_mw_sweep<4, false>), grid, blk, lds, c->stream, rows, n, L, nbr, nnb, M, lnw, u, k0, k1, first, sweep, counts, assign, d_flags);
    return 0;
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
    if ((neighbors == nullptr) != (nnbr == nullptr)) return fail(-1, "fz_mw_sweep: neighbors and nnbr come together");
    FZCHK(mw_limits("fz_mw_sweep", W, M, neighbors == nullptr));
    if (N < 0) return fail(-4, "fz_mw_sweep: %lld objects", (long long)N);
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, lnw, u, counts, assign}));
    const StageRows rv(c, rows, (size_t)W * 8, c->d_draw[2], STAGE_IN), nv(c, neighbors, (size_t)W * 8, c->d_draw[0], STAGE_IN),
        cv(c, nnbr, 8, c->d_draw[1], STAGE_IN), uv(c, u, 8, c->d_draw[4], STAGE_IN), av(c, assign, 8, c->d_draw[5], STAGE_OUT);
    StageWhole st{c};
    const void* d_lnw; void* d_counts;
    FZCHK(st.in(lnw, (size_t)M * 8, &d_lnw)); FZCHK(st.out(counts, (size_t)M * 8, &d_counts));
    HIPCHK(hipMemsetAsync(d_counts, 0, (size_t)M * 8, c->stream));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    const int64_t per_obj = (rv.staged() ? W * 8 : 0) + (nv.staged() ? W * 8 + 8 : 0) + (uv.staged() ? 8 : 0) + (av.staged() ? 8 : 0);
    int64_t nc = per_obj ? std::min<int64_t>(std::max<int64_t>(1, c->ws_limit / per_obj), 1 << 18) : N;
    nc = std::max<int64_t>(1, std::min(nc, N));
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dr; const int64_t* dn; const int64_t* dc; const double* du; int64_t* da;
        FZCHK(rv.at(i0, n, &dr)); FZCHK(nv.at(i0, n, &dn)); FZCHK(cv.at(i0, n, &dc)); FZCHK(uv.at(i0, n, &du)); FZCHK(av.at(i0, n, &da));
        if (du) {
            int bad = 0;
            FZCHK(fz_flag_roundtrip(c, bad, [&](int* df) {
                hipLaunchKernelGGL(fz::k_draw_check_u, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, du, n, df);
                return 0;
            }));
            if (bad) return fail(-4, "fz_mw_sweep: a uniform outside [0, 1]");
        }
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            FZCHK(mw_launch_sweep(c, n, W, dr, dn, dc, M, (const double*)d_lnw, du, key0, key1, first + i0, sweep, (unsigned long long*)d_counts, da,
                                  d_flags));
        }
        FZCHK(av.back(i0, n));
    }
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
    if ((neighbors == nullptr) != (nnbr == nullptr)) return fail(-1, "fz_mw_chain: neighbors and nnbr come together");
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
