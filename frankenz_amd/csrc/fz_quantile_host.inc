// Host side of the posterior quantiles (fz_quantile.h; docs/quantiles.md): fz_row_quantiles.
// Included by frankenz_hip.hip after fz_bins_host.inc, whose scratch it shares (no call of the two overlaps): d_bins[0..2] a host
// caller's staged rows, neighbours and counts; d_bins[3] the call's counters; d_bins[4] the quantiles going back; d_bins[7] the model
// records.  The label tables as given and the probabilities go through d_net.

extern "C" int fz_row_quantiles(fz_ctx* c, const double* rows, int64_t N, int64_t W, const int64_t* neighbors, const int64_t* nnbr, int64_t M,
                                const double* labels, const double* label_errs, const double* probs, int64_t Q, double lncut, double* out,
                                int64_t* nskip, int64_t* nfail, int64_t* niter) {
    const char* who = "fz_row_quantiles";
    if (!c || !rows || !labels || !label_errs || !probs || !out || !nskip || !nfail || !niter) return fail(-1, "%s: NULL argument", who);
    FZCHK(rows_entry(who, neighbors, nnbr, N, W, M));
    if (Q < 1) return fail(-4, "%s: %lld probabilities", who, (long long)Q);
    if (Q > FZ_BINS_MAX) return fail(-5, "%s: %lld probabilities, the limit is %d (FZ_BINS_MAX)", who, (long long)Q, FZ_BINS_MAX);
    if (!(lncut < 0.0)) return fail(-4, "%s: the cut ln(wt_thresh) must be negative (-inf: none)", who);
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {rows, neighbors, nnbr, labels, label_errs, probs, out, nskip, nfail, niter}));

    // ---- the refusals that need no row: the probabilities, then the label table ----
    {
        std::vector<double> h((size_t)Q);
        FZCHK(host_read(h.data(), probs, (size_t)Q * 8));
        for (int64_t k = 0; k < Q; ++k)
            if (!(h[k] > 0.0 && h[k] < 1.0)) return fail(-4, "%s: probability %lld is not inside (0, 1)", who, (long long)k);
    }
    RowsIn in(c, rows, neighbors, nnbr, W, c->d_bins[0], c->d_bins[1], c->d_bins[2]);
    StageRows ov(c, out, (size_t)Q * 8, c->d_bins[4], STAGE_OUT);
    StageWhole st{c};
    const void *d_y, *d_s, *d_p;
    FZCHK(st.in(labels, (size_t)M * 8, &d_y)); FZCHK(st.in(label_errs, (size_t)M * 8, &d_s)); FZCHK(st.in(probs, (size_t)Q * 8, &d_p));
    const size_t cbytes = (size_t)FZ_QUANT_SLOTS * 16 * 8;
    FZCHK(c->d_bins[3].ensure(cbytes));
    unsigned long long* d_cnt = c->d_bins[3].as<unsigned long long>();
    HIPCHK(hipMemsetAsync(d_cnt, 0, cbytes, c->stream));
    int* d_flags;
    FZCHK(mw_flags_begin(c, &d_flags));
    unsigned long long* d_bad = (unsigned long long*)(d_flags + 2);  // the smallest refused model: all ones = none
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    FZCHK(c->d_bins[7].ensure((size_t)M * 32));
    double4* d_rec = c->d_bins[7].as<double4>();
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_quant_pack, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, (const double*)d_y, (const double*)d_s, M, d_rec, d_bad);
    }
    HIPCHK(hipGetLastError());
    {
        unsigned long long hf[2] = {0ull, 0ull};                     // the flags word (and its pad), the smallest refused model
        FZCHK(copy_out(c, hf, d_flags, 16));
        if (hf[1] != ~0ull)
            return fail(-4, "%s: model %llu has a label that is not finite, an error that is negative, nan or inf, or an overflowing |y| + 40 s", who, hf[1]);
    }

    // ---- the rows, in chunks under the workspace limit ----
    const RowGeometry geo = row_geometry(W);
    FZCHK(for_row_chunks(c, N, in, {&ov}, [&](int64_t, int64_t n) {
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            const dim3 grid = geo.grid(n), blk(256);
            if (geo.wpo == 1) hipLaunchKernelGGL((fz::k_row_quantiles<1>), grid, blk, 0, c->stream, in.rows(), n, W, in.nbr(), in.nnb(), M, (const double4*)d_rec, (const double*)d_p, (int)Q, lncut, ov.as<double>(), d_cnt, d_flags);
            else hipLaunchKernelGGL((fz::k_row_quantiles<4>), grid, blk, 0, c->stream, in.rows(), n, W, in.nbr(), in.nnb(), M, (const double4*)d_rec, (const double*)d_p, (int)Q, lncut, ov.as<double>(), d_cnt, d_flags);
        }
        HIPCHK(hipGetLastError());
        return 0;
    }));
    FZCHK(row_flags_check(c, who, W, M));
    std::vector<unsigned long long> hc((size_t)FZ_QUANT_SLOTS * 16);
    FZCHK(copy_out(c, hc.data(), d_cnt, cbytes));
    HIPCHK(hipStreamSynchronize(c->stream));
    int64_t tot[3] = {0, 0, 0};
    for (int s = 0; s < FZ_QUANT_SLOTS; ++s) for (int k = 0; k < 3; ++k) tot[k] += (int64_t)hc[(size_t)s * 16 + k];
    FZCHK(host_write(nskip, &tot[0], 8)); FZCHK(host_write(nfail, &tot[1], 8)); FZCHK(host_write(niter, &tot[2], 8));
    return 0;
}
