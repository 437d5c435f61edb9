// Host side of the posterior bin masses and mixture CDFs (fz_bins.h; docs/bins.md): fz_row_bins, fz_row_cdf.
// Included by frankenz_hip.hip after fz_rows_host.inc (geometry, entry checks, the error flags of d_mw[0], the chunk loop).
// Scratch: d_bins[0..2] a host caller's staged rows, neighbours and counts; d_bins[3] its per-object points; d_bins[4..6] the masses
// (CDF values), below and above going back; d_bins[7] the model records.  The label tables as given, the edges or shared points and
// nskip go through d_net.

namespace {
// n device rows, enqueued: row_geometry's geometry
template <bool CDF>
void bins_launch(fz_ctx* c, int64_t n, int64_t W, const double* rows, const int64_t* nbr, const int64_t* nnb, int64_t M, const double2* rec,
                 const double* x, int64_t xstride, int P, double lncut, bool normalize, double* out, double* below, double* above,
                 unsigned long long* nskip, int* d_flags) {
    const RowGeometry geo = row_geometry(W);
    const dim3 grid = geo.grid(n), blk(256);
    if (geo.wpo == 1) hipLaunchKernelGGL((fz::k_row_bins<1, CDF>), grid, blk, 0, c->stream, rows, n, W, nbr, nnb, M, rec, x, xstride, P, lncut, normalize, out, below, above, nskip, d_flags);
    else hipLaunchKernelGGL((fz::k_row_bins<4, CDF>), grid, blk, 0, c->stream, rows, n, W, nbr, nnb, M, rec, x, xstride, P, lncut, normalize, out, below, above, nskip, d_flags);
}

// points: P shared values (per_object false: read on the host, edges must also increase strictly) or (N, P) rows
template <bool CDF>
int bins_run(fz_ctx* c, const char* who, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
             const double* labels, const double* label_errs, const double* points, int64_t P, bool per_object, double lncut, bool normalize,
             double* out, double* below, double* above, int64_t* nskip) {
    if (!c || !rows || !labels || !label_errs || !points || !out || !nskip) return fail(-1, "%s: NULL argument", who);
    FZCHK(rows_entry(who, neighbors, nnbr, N, W, M));
    if (CDF ? P < 1 : P < 2) return fail(-4, CDF ? "%s: %lld points" : "%s: %lld bin edges, a bin needs two", who, (long long)P);
    const int64_t NB = CDF ? P : P - 1;
    if (NB > FZ_BINS_MAX) return fail(-5, "%s: %lld %s, the limit is %d (FZ_BINS_MAX)", who, (long long)NB, CDF ? "points" : "bins", FZ_BINS_MAX);
    if (!(lncut < 0.0)) return fail(-4, "%s: the cut ln(wt_thresh) must be negative (-inf: none)", who);
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, labels, label_errs, points, out, below, above, nskip}));
    const size_t orow = (size_t)NB * 8;
    RowsIn in(c, rows, neighbors, nnbr, W, c->d_bins[0], c->d_bins[1], c->d_bins[2]);
    StageRows pv(c, per_object ? points : nullptr, (size_t)P * 8, c->d_bins[3], STAGE_IN), ov(c, out, orow, c->d_bins[4], STAGE_OUT),
        bv(c, below, 8, c->d_bins[5], STAGE_OUT), av(c, above, 8, c->d_bins[6], STAGE_OUT);
    StageWhole st{c};
    const void *d_y, *d_s, *d_x = nullptr; void* d_ns;
    FZCHK(st.in(labels, (size_t)M * 8, &d_y)); FZCHK(st.in(label_errs, (size_t)M * 8, &d_s)); FZCHK(st.out(nskip, 8, &d_ns));
    HIPCHK(hipMemsetAsync(d_ns, 0, 8, c->stream));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    unsigned long long* d_bad = (unsigned long long*)(d_flags + 2);  // the smallest refused model: all ones = none
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));

    // ---- the refusals that need no row: edges and points, then the label table ----
    if (!per_object) {
        std::vector<double> h((size_t)P);
        FZCHK(host_read(h.data(), points, (size_t)P * 8));
        for (int64_t k = 0; k < P; ++k) {
            if (!(h[k] - h[k] == 0.0)) return fail(-4, "%s: %s %lld is not finite", who, CDF ? "point" : "bin edge", (long long)k);
            if (!CDF && k && !(h[k] > h[k - 1])) return fail(-4, "%s: the bin edges must increase strictly (edge %lld)", who, (long long)k);
        }
        FZCHK(st.in(points, (size_t)P * 8, &d_x));
    } else if (N > 0) {
        if (pv.dev) {
            const int64_t cnt = N * P;
            hipLaunchKernelGGL(fz::k_bins_check_points, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 4096)), dim3(256), 0, c->stream, points, cnt, d_flags);
        } else {
            for (int64_t k = 0; k < N * P; ++k)
                if (!(points[k] - points[k] == 0.0)) return fail(-4, "%s: a point of object %lld is not finite", who, (long long)(k / P));
        }
    }
    FZCHK(c->d_bins[7].ensure((size_t)M * 16));
    double2* d_rec = c->d_bins[7].as<double2>();
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_bins_pack, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, (const double*)d_y, (const double*)d_s, M, d_rec, d_bad);
    }
    HIPCHK(hipGetLastError());
    {
        unsigned long long hf[2] = {0ull, 0ull};                     // the flags word (and its pad), the smallest refused model
        FZCHK(copy_out(c, hf, d_flags, 16));
        if ((int)hf[0] & FZ_BINS_ERR_POINT) return fail(-4, "%s: a point is not finite", who);
        if (hf[1] != ~0ull) return fail(-4, "%s: model %llu has a label that is not finite or an error that is negative or nan", who, hf[1]);
    }

    // ---- the rows, in chunks under the workspace limit ----
    FZCHK(for_row_chunks(c, N, in, {&pv, &ov, &bv, &av}, [&](int64_t, int64_t n) {
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            bins_launch<CDF>(c, n, W, in.rows(), in.nbr(), in.nnb(), M, (const double2*)d_rec, per_object ? pv.as<const double>() : (const double*)d_x,
                             per_object ? P : 0, (int)P, lncut, normalize, ov.as<double>(), bv.as<double>(), av.as<double>(),
                             (unsigned long long*)d_ns, d_flags);
        }
        HIPCHK(hipGetLastError());
        return 0;
    }));
    FZCHK(row_flags_check(c, who, W, M));
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
}  // namespace

extern "C" int fz_row_bins(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                           const double* labels, const double* label_errs, const double* edges, int64_t E, double lncut, int32_t normalize,
                           double* p, double* below, double* above, int64_t* nskip) {
    return bins_run<false>(c, "fz_row_bins", rows, N, W, neighbors, nnbr, M, labels, label_errs, edges, E, false, lncut, normalize != 0, p, below,
                           above, nskip);
}

extern "C" int fz_row_cdf(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                          const double* labels, const double* label_errs, const double* points, int64_t P, int32_t per_object, double lncut,
                          double* cdf, int64_t* nskip) {
    return bins_run<true>(c, "fz_row_cdf", rows, N, W, neighbors, nnbr, M, labels, label_errs, points, P, per_object != 0, lncut, false, cdf, nullptr,
                          nullptr, nskip);
}
