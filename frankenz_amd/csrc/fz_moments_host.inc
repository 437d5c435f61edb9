// Host side of the posterior moments and the zero-point sums (fz_moments.h; docs/predictive.md): fz_row_moments, fz_phot_sums.
// Included by frankenz_hip.hip after fz_mw_em_host.inc (mw_limits, the error flags of d_mw[0]).
// Scratch: d_mom[0..6] a host caller's staged rows, neighbours, counts, scales and the mean / var / share rows going back (fz_phot_sums:
// x, xe, xm, mean, var); d_mom[7] the strip partials of fz_phot_sums; d_mom[8] the model records of fz_row_moments.  The value tables
// as given and the small results go through d_net.

namespace {
int mom_flags_check(fz_ctx* c, const char* who, int64_t W, int64_t M) {
    int ef = 0;
    HIPCHK(hipGetLastError());
    FZCHK(copy_out(c, &ef, c->d_mw[0].p, sizeof(int)));
    if (ef & FZ_MW_ERR_NNB) return fail(-3, "%s: Nneighbors outside [0, %lld]", who, (long long)W);
    if (ef & FZ_MW_ERR_NBR) return fail(-3, "%s: a neighbour index outside [0, %lld)", who, (long long)M);
    return 0;
}
template <int LB>
void mom_launch_lb(fz_ctx* c, int wpo, int64_t n, int64_t W, const double* rows, const int64_t* nbr, const int64_t* nnb, const double* scale, int64_t M,
                   int L, const double* rec, int RS, bool has_ve, double* mean, double* var, double* share, unsigned long long* nskip, int* d_flags) {
    const int opb = 4 / wpo;
    const dim3 grid((unsigned)((n + opb - 1) / opb)), blk(256);
    if (wpo == 1) hipLaunchKernelGGL((fz::k_row_moments<LB, 1>), grid, blk, 0, c->stream, rows, n, W, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else hipLaunchKernelGGL((fz::k_row_moments<LB, 4>), grid, blk, 0, c->stream, rows, n, W, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
}
// n device rows, enqueued: the geometry is k_draw's, a function of W alone (FZ_DRAW_WPO = 1 / 4 forces one: tests); the column bucket
// is the smallest of 4, 8, 16, 32 that holds L
void mom_launch(fz_ctx* c, int64_t n, int64_t W, const double* rows, const int64_t* nbr, const int64_t* nnb, const double* scale, int64_t M, int L,
                const double* rec, int RS, bool has_ve, double* mean, double* var, double* share, unsigned long long* nskip, int* d_flags) {
    int wpo = W <= FZ_DRAW_WAVE_LMAX ? 1 : 4;
    const long long forced = fz_dbg_int("FZ_DRAW_WPO", 0);
    if (forced == 1 || forced == 4) wpo = (int)forced;
    if (L <= 4) mom_launch_lb<4>(c, wpo, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else if (L <= 8) mom_launch_lb<8>(c, wpo, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else if (L <= 16) mom_launch_lb<16>(c, wpo, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
    else mom_launch_lb<32>(c, wpo, n, W, rows, nbr, nnb, scale, M, L, rec, RS, has_ve, mean, var, share, nskip, d_flags);
}
}  // namespace

extern "C" int fz_row_moments(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, const double* scale,
                              int64_t M, int32_t L, const double* values, const double* value_errs, const double* value_mask, double* mean,
                              double* var, double* share, int64_t* nskip) {
    if (!c || !rows || !values || !mean || !nskip) return fail(-1, "fz_row_moments: NULL argument");
    if ((neighbors == nullptr) != (nnbr == nullptr)) return fail(-1, "fz_row_moments: neighbors and nnbr come together");
    if (L < 1) return fail(-4, "fz_row_moments: %d value columns", (int)L);
    if (L > FZ_MOM_LMAX) return fail(-5, "fz_row_moments: %d value columns, the limit is %d (FZ_MOM_LMAX)", (int)L, FZ_MOM_LMAX);
    FZCHK(mw_limits("fz_row_moments", W, M, neighbors == nullptr));
    if (N < 0) return fail(-4, "fz_row_moments: %lld objects", (long long)N);
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, scale, values, value_errs, value_mask, mean, var, share, nskip}));
    const StageRows rv(c, rows, (size_t)W * 8, c->d_mom[0], STAGE_IN), nv(c, neighbors, (size_t)W * 8, c->d_mom[1], STAGE_IN),
        cv(c, nnbr, 8, c->d_mom[2], STAGE_IN), sv(c, scale, (size_t)W * 8, c->d_mom[3], STAGE_IN),
        mv(c, mean, (size_t)L * 8, c->d_mom[4], STAGE_OUT), vv(c, var, (size_t)L * 8, c->d_mom[5], STAGE_OUT),
        hv(c, share, (size_t)L * 8, c->d_mom[6], STAGE_OUT);
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
    int64_t per_obj = 0;
    for (const StageRows* s : {&rv, &nv, &cv, &sv, &mv, &vv, &hv}) if (s->staged()) per_obj += (int64_t)s->row;
    int64_t nc = per_obj ? std::min<int64_t>(std::max<int64_t>(1, c->ws_limit / per_obj), 1 << 18) : N;
    nc = std::max<int64_t>(1, std::min(nc, N));
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double *dr, *ds; const int64_t *dn, *dc; double *dm, *dv, *dh;
        FZCHK(rv.at(i0, n, &dr)); FZCHK(nv.at(i0, n, &dn)); FZCHK(cv.at(i0, n, &dc)); FZCHK(sv.at(i0, n, &ds));
        FZCHK(mv.at(i0, n, &dm)); FZCHK(vv.at(i0, n, &dv)); FZCHK(hv.at(i0, n, &dh));
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            mom_launch(c, n, W, dr, dn, dc, ds, M, (int)L, (const double*)d_rec, RS, value_errs != nullptr, dm, dv, dh,
                       (unsigned long long*)d_ns, d_flags);
        }
        HIPCHK(hipGetLastError());
        FZCHK(mv.back(i0, n)); FZCHK(vv.back(i0, n)); FZCHK(hv.back(i0, n));
    }
    FZCHK(mom_flags_check(c, "fz_row_moments", W, M));
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
