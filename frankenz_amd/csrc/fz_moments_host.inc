// Host side of the posterior moments and the zero-point sums (fz_moments.h; docs/predictive.md): fz_row_moments, fz_phot_sums.
// Included by frankenz_hip.hip after fz_rows_host.inc (geometry, entry checks, the error flags of d_mw[0], the chunk loop).
// Scratch: d_mom[0..6] a host caller's staged rows, neighbours, counts, scales and the mean / var / share rows going back (fz_phot_sums:
// x, xe, xm, mean, var); d_mom[7] the strip partials of fz_phot_sums; d_mom[8] the model records of fz_row_moments.  The value tables
// as given and the small results go through d_net.

namespace {
template <int LB>
void mom_launch_lb(fz_ctx* c, int64_t n, int64_t W, const double* rows, const int64_t* nbr, const int64_t* nnb, const double* scale, int64_t M,
                   int L, const double* rec, int RS, bool has_ve, double* mean, double* var, double* share, unsigned long long* nskip, int* d_flags) {
    const RowGeometry geo = row_geometry(W);
    const dim3 grid = geo.grid(n), blk(256);
    if (geo.wpo == 1) hipLaunchKernelGGL((fz::k_row_moments<LB, 1>), grid, blk, 0, c->stream, rows, n, W, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else hipLaunchKernelGGL((fz::k_row_moments<LB, 4>), grid, blk, 0, c->stream, rows, n, W, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
}
// n device rows, enqueued: row_geometry's geometry; the column bucket is the smallest of 4, 8, 16, 32 that holds L
void mom_launch(fz_ctx* c, int64_t n, int64_t W, const double* rows, const int64_t* nbr, const int64_t* nnb, const double* scale, int64_t M, int L,
                const double* rec, int RS, bool has_ve, double* mean, double* var, double* share, unsigned long long* nskip, int* d_flags) {
    if (L <= 4) mom_launch_lb<4>(c, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else if (L <= 8) mom_launch_lb<8>(c, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else if (L <= 16) mom_launch_lb<16>(c, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else mom_launch_lb<32>(c, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
}
}  // namespace

extern "C" int fz_row_moments(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, const double* scale,
                              int64_t M, int32_t L, const double* values, const double* value_errs, const double* value_mask, double* mean,
                              double* var, double* share, int64_t* nskip) {
    if (!c || !rows || !values || !mean || !nskip) return fail(-1, "fz_row_moments: NULL argument");
    FZCHK(rows_entry("fz_row_moments", neighbors, nnbr, N, W, M));
    if (L < 1) return fail(-4, "fz_row_moments: %d value columns", (int)L);
    if (L > FZ_MOM_LMAX) return fail(-5, "fz_row_moments: %d value columns, the limit is %d (FZ_MOM_LMAX)", (int)L, FZ_MOM_LMAX);
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, scale, values, value_errs, value_mask, mean, var, share, nskip}));
    RowsIn in(c, rows, neighbors, nnbr, W, c->d_mom[0], c->d_mom[1], c->d_mom[2]);
    StageRows sv(c, scale, (size_t)W * 8, c->d_mom[3], STAGE_IN), mv(c, mean, (size_t)L * 8, c->d_mom[4], STAGE_OUT),
        vv(c, var, (size_t)L * 8, c->d_mom[5], STAGE_OUT), hv(c, share, (size_t)L * 8, c->d_mom[6], STAGE_OUT);
    StageWhole st{c};
    const void *d_v, *d_ve, *d_vm; void* d_ns;
    FZCHK(st.in(values, (size_t)M * L * 8, &d_v)); FZCHK(st.in(value_errs, (size_t)M * L * 8, &d_ve));
    FZCHK(st.in(value_mask, (size_t)M * L * 8, &d_vm)); FZCHK(st.out(nskip, 8, &d_ns));
    HIPCHK(hipMemsetAsync(d_ns, 0, 8, c->stream));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    // one record per model out of the three tables (fz_moments.h)
    const int RS = fz::mom_record_stride((int)L);
    FZCHK(c->d_mom[8].ensure((size_t)M * RS * 8));
    double* d_rec = c->d_mom[8].as<double>();
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_mom_pack, dim3((unsigned)((M * RS + 255) / 256)), dim3(256), 0, c->stream, (const double*)d_v, (const double*)d_ve,
                           (const double*)d_vm, M, (int)L, RS, d_rec);
    }
    FZCHK(for_row_chunks(c, N, in, {&sv, &mv, &vv, &hv}, [&](int64_t, int64_t n) {
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            mom_launch(c, n, W, in.rows(), in.nbr(), in.nnb(), sv.as<const double>(), M, (int)L, (const double*)d_rec, RS, value_errs != nullptr,
                       mv.as<double>(), vv.as<double>(), hv.as<double>(), (unsigned long long*)d_ns, d_flags);
        }
        HIPCHK(hipGetLastError());
        return 0;
    }));
    FZCHK(row_flags_check(c, "fz_row_moments", W, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_phot_sums(fz_ctx* c, const double* x, const double* xe, const double* xm, const double* mean, const double* var, int64_t N,
                            int32_t B, double clip, double* sums, int64_t* counts) {
    if (!c || !x || !xe || !xm || !mean || !var || !sums || !counts) return fail(-1, "fz_phot_sums: NULL argument");
    if (B < 1 || N < 0) return fail(-4, "fz_phot_sums: %lld objects in %d bands", (long long)N, (int)B);
    if (B > FZ_MOM_LMAX) return fail(-5, "fz_phot_sums: %d bands, the limit is %d", (int)B, FZ_MOM_LMAX);
    if (clip != clip || clip < 0.0) return fail(-4, "fz_phot_sums: clip must be 0 (off) or positive");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {x, xe, xm, mean, var, sums, counts}));
    const size_t row = (size_t)B * 8;
    const StageRows xv(c, x, row, c->d_mom[0], STAGE_IN), ev(c, xe, row, c->d_mom[1], STAGE_IN), mv(c, xm, row, c->d_mom[2], STAGE_IN),
        pv(c, mean, row, c->d_mom[3], STAGE_IN), vv(c, var, row, c->d_mom[4], STAGE_IN);
    StageWhole st{c};
    void *d_sums, *d_counts;
    FZCHK(st.out(sums, 3 * row, &d_sums)); FZCHK(st.out(counts, 2 * row, &d_counts));
    const int64_t nstrips = (N + NZ_CHUNK - 1) / NZ_CHUNK;
    FZCHK(c->d_mom[7].ensure((size_t)std::max<int64_t>(1, nstrips) * FZ_PHOT_NQ * row));
    double* partial = c->d_mom[7].as<double>();
    // chunks of whole strips, so that a strip is always the same NZ_CHUNK objects counted from the caller's object 0
    int64_t per_obj = 0;
    for (const StageRows* s : {&xv, &ev, &mv, &pv, &vv}) if (s->staged()) per_obj += (int64_t)row;
    int64_t nc = N;
    if (per_obj) nc = std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / per_obj / NZ_CHUNK, 256)) * NZ_CHUNK;
    nc = std::min<int64_t>(nc, (int64_t)32768 * NZ_CHUNK);          // (grid.x stays far below its limit)
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double *dx, *de, *dm, *dp, *dv;
        FZCHK(xv.at(i0, n, &dx)); FZCHK(ev.at(i0, n, &de)); FZCHK(mv.at(i0, n, &dm)); FZCHK(pv.at(i0, n, &dp)); FZCHK(vv.at(i0, n, &dv));
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_phot_sums, dim3((unsigned)((n + NZ_CHUNK - 1) / NZ_CHUNK), (unsigned)B), dim3(NZ_NT), 0, c->stream, dx, de, dm, dp, dv, n,
                           (int)B, clip, i0 / NZ_CHUNK, nstrips, partial);
    }
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_phot_fin, dim3((unsigned)(FZ_PHOT_NQ * B)), dim3(NZ_NT), 0, c->stream, (const double*)partial, nstrips, (int)B,
                           (double*)d_sums, (long long*)d_counts);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
