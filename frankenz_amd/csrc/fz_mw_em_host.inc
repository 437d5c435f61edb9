// Host side of EM over the model weights (fz_mw_em.h; docs/model_weights.md): fz_mw_em_index_bytes, fz_mw_em_index, fz_mw_loglike,
// fz_mw_em.  Included by frankenz_hip.hip after fz_rows_host.inc and fz_mw_host.inc (mw_limits, the error flags, mw_launch_rows).
// Scratch: d_mwem[0] ell, [1] partials of sum(ell), [2] segment sums, [3] partials of sum(a) and of the prior term + sum(a),
// [4] seg_off, [5] scan partials; the index build alone: [6] row starts, [7] [8] keys, [9] [10] objects / values in flight, [11] digit
// histograms -- released when the build returns.

#define FZ_MW_EM_NMAX ((int64_t)1 << 31)    // objects: col_obj is int32

namespace {
int em_flags_check(fz_ctx* c, const char* who, int64_t W, int64_t M) {
    int ef;
    FZCHK(mw_flags_read(c, &ef));
    if (ef & FZ_MW_ERR_ALPHA1) return fail(-4, "%s: alpha must be finite and >= 1 (below 1 the posterior has no maximum)", who);
    FZCHK(row_flags_check(who, ef, W, M));
    if (ef & FZ_MW_ERR_ZERO) return fail(-7, "%s: no object has a posterior under these weights and alpha == 1: no weights to normalise", who);
    return 0;
}
int em_limits(const char* who, int64_t N, int64_t W, int64_t M, bool dense) {
    FZCHK(mw_limits(who, W, M, dense));
    if (N < 1) return fail(-4, "%s: %lld objects", who, (long long)N);
    if (N >= FZ_MW_EM_NMAX) return fail(-5, "%s: %lld objects, the limit is N < 2^31 (FZ_MW_EM_NMAX)", who, (long long)N);
    return 0;
}
// the row pass over n device rows, enqueued
int em_launch_rows(fz_ctx* c, int64_t n, int64_t L, const double* rows, const int64_t* nbr, const int64_t* nnb, int64_t M, const double* lnw,
                   double* ell, int* d_flags) {
    decltype(fz::k_mw_em_rows<1, true>)* const kern[3] = {fz::k_mw_em_rows<1, true>, fz::k_mw_em_rows<1, false>, fz::k_mw_em_rows<4, false>};
    return mw_launch_rows(c, n, L, kern, rows, n, L, nbr, nnb, M, lnw, ell, d_flags);
}
// out[0..n] = the exclusive scan of in[0..n) and its total, enqueued (out may be in)
int em_scan(fz_ctx* c, const int64_t* in, int64_t n, int64_t* out) {
    const int64_t nb = (n + FZ_MW_EM_SCAN - 1) / FZ_MW_EM_SCAN;
    FZCHK(c->d_mwem[5].ensure((size_t)nb * 8));
    int64_t* part = c->d_mwem[5].as<int64_t>();
    hipLaunchKernelGGL(fz::k_mw_em_scan_part, dim3((unsigned)nb), dim3(256), 0, c->stream, in, n, part);
    hipLaunchKernelGGL(fz::k_mw_em_scan_top, dim3(1), dim3(256), 0, c->stream, part, nb);
    hipLaunchKernelGGL(fz::k_mw_em_scan_apply, dim3((unsigned)nb), dim3(256), 0, c->stream, in, n, (const int64_t*)part, out);
    return 0;
}
unsigned em_stride_grid(int64_t tot) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((tot + 255) / 256, 1 << 18)); }
}  // namespace

extern "C" int fz_mw_em_index_bytes(fz_ctx* c, int64_t N, int64_t W, const int64_t* nnbr, int64_t M, int64_t* entries, int64_t* bytes) {
    if (!c || !entries || !bytes) return fail(-1, "fz_mw_em_index_bytes: NULL argument");
    FZCHK(em_limits("fz_mw_em_index_bytes", N, W, M, false));
    *entries = 0; *bytes = 0;
    if (!nnbr) return 0;                                             // dense rows need no index
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {nnbr}));
    std::vector<int64_t> h;
    const int64_t* p = nnbr;
    if (is_device_ptr(nnbr)) {
        h.resize((size_t)N);
        FZCHK(copy_out(c, h.data(), nnbr, (size_t)N * 8));
        p = h.data();
    }
    int64_t E = 0;
    for (int64_t i = 0; i < N; ++i) {
        if (p[i] < 0 || p[i] > W) return fail(-3, "fz_mw_em_index_bytes: Nneighbors outside [0, %lld]", (long long)W);
        E += p[i];
    }
    *entries = E;
    *bytes = (M + 1) * 8 + E * 12;
    return 0;
}

extern "C" int fz_mw_em_index(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                              int64_t entries, int64_t* col_off, int32_t* col_obj, double* col_val) {
    if (!c || !rows || !neighbors || !nnbr || !col_off) return fail(-1, "fz_mw_em_index: NULL argument");
    FZCHK(em_limits("fz_mw_em_index", N, W, M, false));
    const int64_t E = entries;
    if (E < 0 || E > N * W || (E > 0 && (!col_obj || !col_val))) return fail(-4, "fz_mw_em_index: %lld entries", (long long)E);
    if (!is_device_ptr(rows) || !is_device_ptr(neighbors) || !is_device_ptr(nnbr) || !is_device_ptr(col_off) ||
        (E > 0 && (!is_device_ptr(col_obj) || !is_device_ptr(col_val))))
        return fail(-4, "fz_mw_em_index: rows, neighbors, nnbr and the index arrays must be device arrays");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, col_off, col_obj, col_val}));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    Timer t(c, &c->tm.ms_other, &c->tm.n_other);
    // column lengths (and the refusal of a bad table before anything is gathered), then their scan
    HIPCHK(hipMemsetAsync(col_off, 0, (size_t)(M + 1) * 8, c->stream));
    hipLaunchKernelGGL(fz::k_mw_em_count, dim3(em_stride_grid(N * W)), dim3(256), 0, c->stream, neighbors, nnbr, N, W, M, (unsigned long long*)col_off,
                       d_flags);
    FZCHK(em_flags_check(c, "fz_mw_em_index", W, M));
    FZCHK(em_scan(c, col_off, M, col_off));
    FZCHK(c->d_mwem[6].ensure((size_t)(N + 1) * 8));
    int64_t* rowstart = c->d_mwem[6].as<int64_t>();
    FZCHK(em_scan(c, nnbr, N, rowstart));
    int64_t Edev = -1;
    FZCHK(copy_out(c, &Edev, rowstart + N, 8));
    if (Edev != E) return fail(-4, "fz_mw_em_index: the tables hold %lld counted entries, the caller sized the index for %lld", (long long)Edev, (long long)E);
    int rc = 0;
    if (E > 0) {
        int bits = 0;
        while (bits < 31 && ((int64_t)1 << bits) < M) ++bits;
        const int P = (bits + 7) / 8;                                // passes of 8 bits that cover [0, M)
        const int64_t nT = (E + FZ_MW_EM_TILE - 1) / FZ_MW_EM_TILE;
        auto run = [&]() -> int {
            FZCHK(c->d_mwem[7].ensure((size_t)E * 4)); FZCHK(c->d_mwem[8].ensure((size_t)E * 4));
            if (P > 0) { FZCHK(c->d_mwem[9].ensure((size_t)E * 4)); FZCHK(c->d_mwem[10].ensure((size_t)E * 8)); FZCHK(c->d_mwem[11].ensure((size_t)(256 * nT + 1) * 8)); }
            // two sets of arrays, the caller's (OUT) and ours (TMP), take turns so that the last pass writes OUT
            int32_t* key[2] = {c->d_mwem[7].as<int32_t>(), c->d_mwem[8].as<int32_t>()};
            int32_t* obj[2] = {col_obj, c->d_mwem[9].as<int32_t>()};
            double* val[2] = {col_val, c->d_mwem[10].as<double>()};
            int cur = P & 1;                                         // the gather's side: P flips later it is OUT (0)
            hipLaunchKernelGGL(fz::k_mw_em_gather, dim3(em_stride_grid(N * W)), dim3(256), 0, c->stream, rows, neighbors, nnbr, (const int64_t*)rowstart, N,
                               W, E, key[cur], obj[cur], val[cur]);
            for (int p = 0; p < P; ++p) {
                int64_t* hist = c->d_mwem[11].as<int64_t>();
                hipLaunchKernelGGL(fz::k_mw_em_rhist, dim3((unsigned)nT), dim3(256), 0, c->stream, (const int32_t*)key[cur], E, 8 * p, nT, hist);
                FZCHK(em_scan(c, hist, 256 * nT, hist));
                hipLaunchKernelGGL(fz::k_mw_em_rscatter, dim3((unsigned)nT), dim3(64), 0, c->stream, (const int32_t*)key[cur], (const int32_t*)obj[cur],
                                   (const double*)val[cur], E, 8 * p, (const int64_t*)hist, nT, key[cur ^ 1], obj[cur ^ 1], val[cur ^ 1]);
                cur ^= 1;
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(c->stream));
            return 0;
        };
        rc = run();
    } else {
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    for (int b = 6; b < 12; ++b) c->d_mwem[b].release();             // up to 20 bytes per entry: not kept
    return rc;
}

extern "C" int fz_mw_loglike(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                             const double* lnw, double* ell, double* lnlike, int64_t* nskip) {
    if (!c || !rows || !lnw || !lnlike || !nskip) return fail(-1, "fz_mw_loglike: NULL argument");
    FZCHK(rows_together("fz_mw_loglike", neighbors, nnbr));
    FZCHK(em_limits("fz_mw_loglike", N, W, M, neighbors == nullptr));
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, lnw, ell, lnlike, nskip}));
    RowsIn in(c, rows, neighbors, nnbr, W, c->d_draw[2], c->d_draw[0], c->d_draw[1]);
    StageWhole st{c};
    const void* d_lnw; void *d_ell, *d_ll, *d_ns;
    FZCHK(st.in(lnw, (size_t)M * 8, &d_lnw)); FZCHK(st.out(ell, (size_t)N * 8, &d_ell));
    FZCHK(st.out(lnlike, 8, &d_ll)); FZCHK(st.out(nskip, 8, &d_ns));
    if (!d_ell) { FZCHK(c->d_mwem[0].ensure((size_t)N * 8)); d_ell = c->d_mwem[0].p; }
    HIPCHK(hipMemsetAsync(d_ns, 0, 8, c->stream));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    FZCHK(for_row_chunks(c, N, in, {}, [&](int64_t i0, int64_t n) {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        return em_launch_rows(c, n, W, in.rows(), in.nbr(), in.nnb(), M, (const double*)d_lnw, (double*)d_ell + i0, d_flags);
    }));
    const int64_t nblkL = (N + NZ_CHUNK - 1) / NZ_CHUNK;
    FZCHK(c->d_mwem[1].ensure((size_t)nblkL * 8));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_mw_em_lsum, dim3((unsigned)nblkL), dim3(NZ_NT), 0, c->stream, (const double*)d_ell, N, c->d_mwem[1].as<double>(),
                           (unsigned long long*)d_ns);
        hipLaunchKernelGGL(fz::k_mw_em_sums, dim3(1), dim3(NZ_NT), 0, c->stream, (const double*)c->d_mwem[1].as<double>(), nblkL, (const double*)nullptr,
                           (const double*)nullptr, (int64_t)0, (double*)d_ll, (double*)nullptr, d_flags);
    }
    FZCHK(em_flags_check(c, "fz_mw_loglike", W, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_mw_em(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                        const int64_t* col_off, const int32_t* col_obj, const double* col_val, int64_t entries, const double* alpha, double* lnw,
                        int32_t niter, double* pos, double* counts, double* trace, int64_t* nskip) {
    if (!c || !rows || !alpha || !lnw || !pos || !counts || !trace || !nskip) return fail(-1, "fz_mw_em: NULL argument");
    FZCHK(rows_together("fz_mw_em", neighbors, nnbr));
    const bool dense = neighbors == nullptr;
    FZCHK(em_limits("fz_mw_em", N, W, M, dense));
    if (niter < 1) return fail(-4, "fz_mw_em: %d iterations", (int)niter);
    const int64_t E = entries;
    if (!dense && (!col_off || E < 0 || E > N * W || (E > 0 && (!col_obj || !col_val))))
        return fail(-4, "fz_mw_em: sparse rows come with their index (fz_mw_em_index) of %lld entries", (long long)E);
    if (!is_device_ptr(rows) || (!dense && (!is_device_ptr(neighbors) || !is_device_ptr(nnbr) || !is_device_ptr(col_off) ||
                                            (E > 0 && (!is_device_ptr(col_obj) || !is_device_ptr(col_val))))))
        return fail(-4, "fz_mw_em: rows, neighbors, nnbr and the index must be device arrays (they stay resident over the iterations)");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, col_off, col_obj, col_val, alpha, lnw, pos, counts, trace, nskip}));
    StageWhole st{c};
    const void* d_al; void *d_lnw, *d_pos, *d_cn, *d_tr, *d_ns;
    FZCHK(st.in(alpha, (size_t)M * 8, &d_al)); FZCHK(st.inout(lnw, (size_t)M * 8, &d_lnw));
    FZCHK(st.out(pos, (size_t)M * 8, &d_pos)); FZCHK(st.out(counts, (size_t)M * 8, &d_cn));
    FZCHK(st.out(trace, (size_t)niter * 8, &d_tr)); FZCHK(st.out(nskip, (size_t)niter * 8, &d_ns));
    const int64_t nblkL = (N + NZ_CHUNK - 1) / NZ_CHUNK, nblkM = (M + NZ_NT - 1) / NZ_NT;
    const int64_t nrs = (N + FZ_MW_EM_RSEG - 1) / FZ_MW_EM_RSEG;
    const int64_t smax = dense ? M * nrs : E / FZ_MW_EM_CSEG + M;    // sum of ceil(len_j / CSEG) <= E / CSEG + M
    if (dense && nrs > 65535) return fail(-5, "fz_mw_em: dense rows of %lld objects exceed 65535 strips of %d rows", (long long)N, FZ_MW_EM_RSEG);
    FZCHK(c->d_mwem[0].ensure((size_t)N * 8)); FZCHK(c->d_mwem[1].ensure((size_t)nblkL * 8));
    FZCHK(c->d_mwem[2].ensure((size_t)smax * 8)); FZCHK(c->d_mwem[3].ensure((size_t)(2 * nblkM + 1) * 8));
    FZCHK(c->d_mwem[4].ensure((size_t)(M + 1) * 8));
    double *ell = c->d_mwem[0].as<double>(), *partL = c->d_mwem[1].as<double>(), *segsum = c->d_mwem[2].as<double>();
    double *partA = c->d_mwem[3].as<double>(), *partP = partA + nblkM, *total = partA + 2 * nblkM;
    int64_t* seg_off = dense ? nullptr : c->d_mwem[4].as<int64_t>();
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    HIPCHK(hipMemsetAsync(d_ns, 0, (size_t)niter * 8, c->stream));
    {
        // every iteration is enqueued without a host synchronisation: the order of the stream is the order of the iterations
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        if (!dense) {
            hipLaunchKernelGGL(fz::k_mw_em_nseg, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, col_off, M, seg_off);
            FZCHK(em_scan(c, seg_off, M, seg_off));
        }
        // measurement only (tools/mw_em_bench.py): FZ_MW_EM_STAGES = 1 stops every iteration after the row pass and its sum, 2 after the
        // column pass; the weights then do not move and the outputs mean nothing
        const long long stages = fz_dbg_int("FZ_MW_EM_STAGES", 3);
        for (int32_t it = 0; it < niter; ++it) {
            FZCHK(em_launch_rows(c, N, W, rows, neighbors, nnbr, M, (const double*)d_lnw, ell, d_flags));
            hipLaunchKernelGGL(fz::k_mw_em_lsum, dim3((unsigned)nblkL), dim3(NZ_NT), 0, c->stream, (const double*)ell, N, partL,
                               (unsigned long long*)d_ns + it);
            if (stages == 1) continue;
            if (dense)
                hipLaunchKernelGGL(fz::k_mw_em_cols_dense, dim3((unsigned)((M + 63) / 64), (unsigned)nrs), dim3(64), 0, c->stream, rows, N, M,
                                   (const double*)d_lnw, (const double*)ell, segsum);
            else
                hipLaunchKernelGGL(fz::k_mw_em_cols, dim3((unsigned)((smax + 3) / 4)), dim3(256), 0, c->stream, col_off, (const int64_t*)seg_off, M, E,
                                   col_obj, col_val, (const double*)d_lnw, (const double*)ell, N, segsum, smax);
            if (stages == 2) continue;
            hipLaunchKernelGGL(fz::k_mw_em_fin, dim3((unsigned)nblkM), dim3(NZ_NT), 0, c->stream, (const int64_t*)seg_off, nrs, (const double*)segsum,
                               (const double*)d_al, (const double*)d_lnw, M, (double*)d_cn, (double*)d_pos, partA, partP, d_flags);
            hipLaunchKernelGGL(fz::k_mw_em_sums, dim3(1), dim3(NZ_NT), 0, c->stream, (const double*)partL, nblkL, (const double*)partA,
                               (const double*)partP, nblkM, (double*)d_tr + it, total, d_flags);
            hipLaunchKernelGGL(fz::k_mw_norm, dim3((unsigned)nblkM), dim3(NZ_NT), 0, c->stream, (const double*)d_pos, M, (const double*)total,
                               (double*)d_pos, (double*)d_lnw);
        }
    }
    FZCHK(em_flags_check(c, "fz_mw_em", W, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
