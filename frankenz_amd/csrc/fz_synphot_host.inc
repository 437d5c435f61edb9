// Host side of fz_synphot_upload / fz_synphot (kernel in fz_synphot.h; docs/simulate.md).

extern "C" int fz_synphot_upload(fz_ctx* c, int64_t Nf, const int64_t* foff, const double* fwave, const double* flw, const double* fwt,
                                 const double* ftab, int64_t Nt, const int64_t* toff, const double* tlw, const double* tasinh) {
    if (!c || !foff || !fwave || !flw || !fwt || !ftab || !toff || !tlw || !tasinh) return fail(-1, "fz_synphot_upload: NULL argument");
    if (is_device_ptr(foff) || is_device_ptr(fwave) || is_device_ptr(flw) || is_device_ptr(fwt) || is_device_ptr(ftab) || is_device_ptr(toff) ||
        is_device_ptr(tlw) || is_device_ptr(tasinh))
        return fail(-1, "fz_synphot_upload: the tables are host arrays");
    if (Nf < 1 || Nf > (1 << 16) || Nt < 1 || Nt >= ((int64_t)1 << 31)) return fail(-1, "fz_synphot_upload: bad number of filters or templates");
    c->sp_Nf = c->sp_Nt = 0;                                   // nothing is left half uploaded
    if (foff[0] != 0 || toff[0] != 0) return fail(-1, "fz_synphot_upload: offsets do not start at 0");
    for (int64_t f = 0; f < Nf; ++f) {
        const int64_t n = foff[f + 1] - foff[f];
        if (n < 2) return fail(-4, "fz_synphot_upload: filter %lld has %lld points (at least 2 are needed)", (long long)f, (long long)n);
        if (foff[f + 1] >= ((int64_t)1 << 31)) return fail(-1, "fz_synphot_upload: too many filter points");
        for (int64_t k = foff[f]; k < foff[f + 1]; ++k)
            if (!(fwave[k] > 0.0) || !std::isfinite(fwave[k]) || !std::isfinite(flw[k]))
                return fail(-4, "fz_synphot_upload: filter %lld: wavelength %lld is not positive and finite", (long long)f, (long long)(k - foff[f]));
    }
    for (int64_t t = 0; t < Nt; ++t) {
        const int64_t n = toff[t + 1] - toff[t];
        if (n < 2) return fail(-4, "fz_synphot_upload: template %lld has %lld points (at least 2 are needed)", (long long)t, (long long)n);
        if (n >= ((int64_t)1 << 30)) return fail(-1, "fz_synphot_upload: template %lld is too long", (long long)t);
        for (int64_t k = toff[t]; k < toff[t + 1]; ++k) {
            if (!std::isfinite(tlw[k]))
                return fail(-4, "fz_synphot_upload: template %lld: wavelength %lld is not positive and finite", (long long)t, (long long)(k - toff[t]));
            if (k > toff[t] && tlw[k] < tlw[k - 1])
                return fail(-4, "fz_synphot_upload: template %lld: wavelengths decrease at point %lld", (long long)t, (long long)(k - toff[t]));
        }
    }
    const int64_t Np = foff[Nf], Ntp = toff[Nt];
    HIPCHK(hipSetDevice(c->device));
    // one block: foff | toff | fwave | flw | fwt | ftab | tlw | tasinh (all 8-byte items)
    const int64_t words = (Nf + 1) + (Nt + 1) + Np * (3 + FZ_SYN_TABW) + 2 * Ntp;
    FZCHK(c->d_sp.ensure((size_t)words * 8));
    char* d = (char*)c->d_sp.p;
    auto put = [&](const void* src, int64_t n) -> int { FZCHK(copy_in(c, d, src, (size_t)n * 8)); d += n * 8; return 0; };
    FZCHK(put(foff, Nf + 1)); FZCHK(put(toff, Nt + 1)); FZCHK(put(fwave, Np)); FZCHK(put(flw, Np)); FZCHK(put(fwt, Np));
    FZCHK(put(ftab, Np * FZ_SYN_TABW)); FZCHK(put(tlw, Ntp)); FZCHK(put(tasinh, Ntp));
    c->h_sp_foff.assign(foff, foff + Nf + 1);
    c->h_sp_toff.assign(toff, toff + Nt + 1);
    c->sp_Nf = Nf; c->sp_Nt = Nt;
    return 0;
}

static fz::SynView syn_view(fz_ctx* c) {
    const int64_t Nf = c->sp_Nf, Nt = c->sp_Nt, Np = c->h_sp_foff[Nf], Ntp = c->h_sp_toff[Nt];
    fz::SynView v; v.Nf = (int)Nf;
    const double* d = c->d_sp.as<double>();
    v.foff = (const int64_t*)d; d += Nf + 1;
    v.toff = (const int64_t*)d; d += Nt + 1;
    v.fwave = d; d += Np; v.flw = d; d += Np; v.fwt = d; d += Np; v.ftab = d; d += Np * FZ_SYN_TABW;
    v.tlw = d; d += Ntp; v.tas = d;
    return v;
}

extern "C" int fz_synphot(fz_ctx* c, int64_t Npair, const int64_t* tmpl, const double* z, const double* ln1pz, int32_t igm, double* out) {
    if (!c || (Npair > 0 && (!tmpl || !z || !ln1pz || !out))) return fail(-1, "fz_synphot: NULL argument");
    if (c->sp_Nf <= 0 || c->sp_Nt <= 0) return fail(-1, "fz_synphot: no filters and templates uploaded (fz_synphot_upload)");
    if (igm != 0 && igm != 1) return fail(-1, "fz_synphot: igm %d not in {0 (none), 1 (Madau)}", igm);
    if (Npair < 0) return fail(-1, "fz_synphot: bad number of pairs");
    if (is_device_ptr(tmpl) || is_device_ptr(z) || is_device_ptr(ln1pz)) return fail(-1, "fz_synphot: the per-pair arrays (tmpl, z, ln1pz) are host arrays");
    // everything the kernel indexes with or branches on is checked here, before anything is written
    for (int64_t p = 0; p < Npair; ++p) {
        if (tmpl[p] < 0 || tmpl[p] >= c->sp_Nt) return fail(-3, "fz_synphot: pair %lld asks for template %lld of %lld", (long long)p, (long long)tmpl[p], (long long)c->sp_Nt);
        const double x = 1. + z[p];
        if (!std::isfinite(x) || x < 0.0 || std::isnan(ln1pz[p])) return fail(-4, "fz_synphot: pair %lld: 1 + z = %g is negative or not finite", (long long)p, x);
    }
    if (Npair == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {out}));
    const int Nf = (int)c->sp_Nf;
    const StageRows ov(c, out, (size_t)Nf * 8, c->d_pl[0], STAGE_OUT);
    const fz::SynView v = syn_view(c);
    // chunks of pairs in the caller's order, each sorted by template on its own: a pair's result is one wave's work whatever the cut
    int64_t nc = std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / ((int64_t)Nf * 8 + (int64_t)sizeof(fz::SynPair) + 16), (int64_t)1 << 24));
    nc = std::min(nc, Npair);
    std::vector<int32_t> order; std::vector<fz::SynPair> pairs; std::vector<fz::SynItem> items[2];
    for (int64_t i0 = 0; i0 < Npair; i0 += nc) {
        const int64_t n = std::min(nc, Npair - i0);
        order.resize(n);
        for (int64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return tmpl[i0 + a] < tmpl[i0 + b]; });
        pairs.resize(n);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t s = i0 + order[i];
            pairs[i] = fz::SynPair{z[s], ln1pz[s], (int32_t)tmpl[s], order[i]};
        }
        // a block takes up to `per` pairs of one template: enough blocks to fill the card, few enough to share a staged table
        const int64_t per = std::max<int64_t>(1, std::min<int64_t>(64, (n + (int64_t)4 * c->cu_count - 1) / ((int64_t)4 * c->cu_count)));
        items[0].clear(); items[1].clear();
        int64_t lds_len = 0;
        for (int64_t a = 0; a < n;) {
            int64_t b = a;
            while (b < n && pairs[b].tmpl == pairs[a].tmpl) ++b;
            const int64_t len = c->h_sp_toff[pairs[a].tmpl + 1] - c->h_sp_toff[pairs[a].tmpl];
            const int which = len <= FZ_SYN_LDS_MAX ? 0 : 1;               // 0: table in LDS, 1: searched in global memory
            if (which == 0) lds_len = std::max(lds_len, len);
            for (int64_t p0 = a; p0 < b; p0 += per) items[which].push_back(fz::SynItem{pairs[a].tmpl, (int32_t)p0, (int32_t)std::min(p0 + per, b), 0});
            a = b;
        }
        FZCHK(c->d_net[0].ensure((size_t)n * sizeof(fz::SynPair))); FZCHK(copy_in(c, c->d_net[0].p, pairs.data(), (size_t)n * sizeof(fz::SynPair)));
        double* dout;
        FZCHK(ov.at(i0, n, &dout));
        for (int which = 0; which < 2; ++which) {
            const int ni = (int)items[which].size();
            if (!ni) continue;
            FZCHK(c->d_net[1 + which].ensure((size_t)ni * sizeof(fz::SynItem)));
            FZCHK(copy_in(c, c->d_net[1 + which].p, items[which].data(), (size_t)ni * sizeof(fz::SynItem)));
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            if (which == 0) {
                const size_t lds = (size_t)lds_len * 8;
                HIPCHK(hipFuncSetAttribute((const void*)fz::k_synphot<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(fz::k_synphot<true>, dim3((unsigned)ni), dim3(FZ_SYN_THREADS), lds, c->stream, v, c->d_net[0].as<fz::SynPair>(),
                                   c->d_net[1].as<fz::SynItem>(), (int)igm, dout);
            } else {
                hipLaunchKernelGGL(fz::k_synphot<false>, dim3((unsigned)ni), dim3(FZ_SYN_THREADS), 0, c->stream, v, c->d_net[0].as<fz::SynPair>(),
                                   c->d_net[2].as<fz::SynItem>(), (int)igm, dout);
            }
        }
        HIPCHK(hipGetLastError());
        FZCHK(ov.back(i0, n));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
