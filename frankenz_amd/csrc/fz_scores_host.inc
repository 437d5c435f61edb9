// Host side of the posterior scoring rules (fz_scores.h; docs/scores.md): fz_row_scores.
// Included by frankenz_hip.hip after fz_quantile_host.inc; it shares d_bins with fz_bins_host.inc (no call of the two overlaps):
// d_bins[0..2] a host caller's staged rows, neighbours and counts; d_bins[3] its per-object points; d_bins[4..6] lnpdf, crps and spread
// going back; d_bins[7] the model records.  d_scores[0] sqnorm going back; d_scores[1] the included counts (the caller's ninc where it
// is a device array); d_scores[2] Z per object; d_scores[3] the chunk's compacted records, 24 W bytes per object -- the last three
// count towards the chunk loop's bytes per object.  The label tables as given, shared points and nskip go through d_net.

extern "C" int fz_row_scores(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                             const double* labels, const double* label_errs, const double* points, int64_t P, int32_t per_object,
                             double lncut, double* lnpdf, double* crps, double* spread, double* sqnorm, int64_t* ninc, int64_t* nskip) {
    const char* who = "fz_row_scores";
    if (!c || !rows || !labels || !label_errs || !points || !nskip) return fail(-1, "%s: NULL argument", who);
    FZCHK(rows_entry(who, neighbors, nnbr, N, W, M));
    if (P < 1) return fail(-4, "%s: %lld points", who, (long long)P);
    if (P > FZ_BINS_MAX) return fail(-5, "%s: %lld points, the limit is %d (FZ_BINS_MAX)", who, (long long)P, FZ_BINS_MAX);
    if (!(lncut < 0.0)) return fail(-4, "%s: the cut ln(wt_thresh) must be negative (-inf: none)", who);
    const bool pairs = crps || spread || sqnorm;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, labels, label_errs, points, lnpdf, crps, spread, sqnorm, ninc, nskip}));
    const size_t prow = (size_t)P * 8;
    RowsIn in(c, rows, neighbors, nnbr, W, c->d_bins[0], c->d_bins[1], c->d_bins[2]);
    StageRows pv(c, per_object ? points : nullptr, prow, c->d_bins[3], STAGE_IN), lv(c, lnpdf, prow, c->d_bins[4], STAGE_OUT),
        cv(c, crps, prow, c->d_bins[5], STAGE_OUT), sv(c, spread, 8, c->d_bins[6], STAGE_OUT), qv(c, sqnorm, 8, c->d_scores[0], STAGE_OUT),
        nv(c, ninc, 8, c->d_scores[1], STAGE_OUT, true), zv(c, nullptr, 8, c->d_scores[2], 0, true),
        kv(c, nullptr, (size_t)W * FZ_SCORES_REC * 8, c->d_scores[3], 0, pairs);
    StageWhole st{c};
    const void *d_y, *d_s, *d_x = nullptr; void* d_ns;
    FZCHK(st.in(labels, (size_t)M * 8, &d_y)); FZCHK(st.in(label_errs, (size_t)M * 8, &d_s)); FZCHK(st.out(nskip, 8, &d_ns));
    HIPCHK(hipMemsetAsync(d_ns, 0, 8, c->stream));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    unsigned long long* d_bad = (unsigned long long*)(d_flags + 2);  // the smallest refused model, then the smallest object over the
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 16, c->stream));              // cap: all ones = none

    // ---- the refusals that need no row: the points, then the label table ----
    if (!per_object) {
        std::vector<double> h((size_t)P);
        FZCHK(host_read(h.data(), points, prow));
        for (int64_t k = 0; k < P; ++k)
            if (!(h[k] - h[k] == 0.0)) return fail(-4, "%s: point %lld is not finite", who, (long long)k);
        FZCHK(st.in(points, prow, &d_x));
    } else if (N > 0) {
        if (pv.dev) {
            const int64_t cnt = N * P;
            hipLaunchKernelGGL(fz::k_bins_check_points, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 4096)), dim3(256), 0, c->stream, points, cnt, d_flags);
        } else {
            for (int64_t k = 0; k < N * P; ++k)
                if (!(points[k] - points[k] == 0.0)) return fail(-4, "%s: a point of object %lld is not finite", who, (long long)(k / P));
        }
    }
    FZCHK(c->d_bins[7].ensure((size_t)M * 32));
    double4* d_rec = c->d_bins[7].as<double4>();
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_scores_pack, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, (const double*)d_y, (const double*)d_s, M, d_rec, d_bad);
    }
    HIPCHK(hipGetLastError());
    {
        unsigned long long hf[2] = {0ull, 0ull};                     // the flags word (and its pad), the smallest refused model
        FZCHK(copy_out(c, hf, d_flags, 16));
        if ((int)hf[0] & FZ_BINS_ERR_POINT) return fail(-4, "%s: a point is not finite", who);
        if (hf[1] != ~0ull)
            return fail(-4, "%s: model %llu has a label that is not finite or an error that is negative, nan or inf", who, hf[1]);
    }

    // ---- the rows, in chunks under the workspace limit: the stage kernel, the cap, the pair kernel ----
    const RowGeometry geo = row_geometry(W);
    FZCHK(for_row_chunks(c, N, in, {&pv, &lv, &cv, &sv, &qv, &nv, &zv, &kv}, [&](int64_t i0, int64_t n) {
        const dim3 grid = geo.grid(n), blk(256);
        const double* x = per_object ? pv.as<const double>() : (const double*)d_x;
        const int64_t xstride = per_object ? P : 0;
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            if (geo.wpo == 1) hipLaunchKernelGGL((fz::k_scores_stage<1>), grid, blk, 0, c->stream, in.rows(), n, W, in.nbr(), in.nnb(), M, (const double4*)d_rec, x, xstride, (int)P, lncut, lv.as<double>(), cv.as<double>(), kv.as<double>(), zv.as<double>(), nv.as<int64_t>(), (int64_t)(pairs ? FZ_SCORES_NMAX : 0), i0, d_bad + 1, (unsigned long long*)d_ns, d_flags);
            else hipLaunchKernelGGL((fz::k_scores_stage<4>), grid, blk, 0, c->stream, in.rows(), n, W, in.nbr(), in.nnb(), M, (const double4*)d_rec, x, xstride, (int)P, lncut, lv.as<double>(), cv.as<double>(), kv.as<double>(), zv.as<double>(), nv.as<int64_t>(), (int64_t)(pairs ? FZ_SCORES_NMAX : 0), i0, d_bad + 1, (unsigned long long*)d_ns, d_flags);
        }
        HIPCHK(hipGetLastError());
        if (!pairs) return 0;
        // the host decides between the stages: a row over the cap, or a row error, and no pair kernel is launched
        unsigned long long hf[3] = {0ull, 0ull, 0ull};
        FZCHK(copy_out(c, hf, d_flags, 24));
        FZCHK(row_flags_check(who, (int)hf[0], W, M));
        if (hf[2] != ~0ull) {
            int64_t cnt = 0;
            FZCHK(copy_out(c, &cnt, nv.as<int64_t>() + ((int64_t)hf[2] - i0), 8));
            return fail(-5, "%s: object %llu has %lld included entries, the limit for the pair sums is %d (FZ_SCORES_NMAX)", who, hf[2],
                        (long long)cnt, FZ_SCORES_NMAX);
        }
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            if (geo.wpo == 1) hipLaunchKernelGGL((fz::k_scores_pairs<1>), grid, blk, 0, c->stream, kv.as<const double>(), zv.as<const double>(), nv.as<const int64_t>(), n, W, (int)P, cv.as<double>(), sv.as<double>(), qv.as<double>());
            else hipLaunchKernelGGL((fz::k_scores_pairs<4>), grid, blk, 0, c->stream, kv.as<const double>(), zv.as<const double>(), nv.as<const int64_t>(), n, W, (int)P, cv.as<double>(), sv.as<double>(), qv.as<double>());
        }
        HIPCHK(hipGetLastError());
        return 0;
    }));
    FZCHK(row_flags_check(c, who, W, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
