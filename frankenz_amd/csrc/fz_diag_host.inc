// Host side of fz_stack2d / fz_recentre_rows / fz_cdf_draws (kernels in fz_diag.h; docs/diagnostics.md).

extern "C" int fz_stack2d(fz_ctx* c, const double* pdfs, int64_t Nrows, int64_t Gy, int64_t nsel, const int64_t* rows,
                          const int64_t* cent, const int64_t* eidx, const double* weff, double pdf_thresh, int32_t prepared,
                          int32_t full_range, int32_t accumulate, double* stack) {
    if (!c || !pdfs || !stack || (nsel > 0 && (!rows || !cent || !eidx || !weff))) return fail(-1, "fz_stack2d: NULL argument");
    if (c->D <= 0 || c->dict_G <= 0) return fail(-1, "fz_stack2d: no dictionary uploaded (fz_kdedict_upload)");
    if (Nrows < 0 || Gy < 1 || Gy > (1 << 24) || nsel < 0 || nsel >= ((int64_t)1 << 31)) return fail(-1, "fz_stack2d: bad shape");
    if (is_device_ptr(rows) || is_device_ptr(cent) || is_device_ptr(eidx) || is_device_ptr(weff))
        return fail(-1, "fz_stack2d: the per-object arrays (rows, cent, eidx, weff) are host arrays");
    const int64_t Gx = c->dict_G;
    // every index the kernels form is checked here
    int64_t wmax = 0;
    for (int64_t k = 0; k < nsel; ++k) {
        if (rows[k] < 0 || rows[k] >= Nrows) return fail(-3, "fz_stack2d: object %lld reads row %lld of %lld", (long long)k, (long long)rows[k], (long long)Nrows);
        if (eidx[k] < 0 || eidx[k] >= c->D) return fail(-3, "fz_stack2d: object at row %lld has dictionary index %lld of %lld", (long long)rows[k], (long long)eidx[k], (long long)c->D);
        const int64_t w = c->h_widths[eidx[k]], len = c->h_offsets[eidx[k] + 1] - c->h_offsets[eidx[k]];
        if (w < 0 || len != 2 * w + 1) return fail(-4, "fz_stack2d: object at row %lld: dictionary entry %lld is malformed (%lld taps for half-width %lld)", (long long)rows[k], (long long)eidx[k], (long long)len, (long long)w);
        if (cent[k] + w < 0 || cent[k] - w > Gx - 1 || cent[k] < -((int64_t)1 << 30) || cent[k] > ((int64_t)1 << 30))
            return fail(-4, "fz_stack2d: object at row %lld: window [%lld, %lld] does not meet the grid [0, %lld)", (long long)rows[k], (long long)(cent[k] - w), (long long)(cent[k] + w), (long long)Gx);
        if (k > 0 && cent[k] < cent[k - 1]) return fail(-1, "fz_stack2d: objects are not sorted by centre");
        wmax = std::max(wmax, w);
    }
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, stack}));
    const StageRows pv(c, pdfs, (size_t)Gy * 8, c->d_pdfs, STAGE_IN);
    const bool p_dev = pv.dev, s_dev = is_device_ptr(stack);
    const int ntx = (int)((Gx + FZ_GEMM_BM - 1) / FZ_GEMM_BM), nty = (int)((Gy + FZ_GEMM_BN - 1) / FZ_GEMM_BN);
    const size_t tile_bytes = (size_t)FZ_GEMM_BM * FZ_GEMM_BN * 8;
    double* d_out = stack;
    if (!s_dev) { FZCHK(c->d_pl[1].ensure((size_t)Gx * Gy * 8)); d_out = c->d_pl[1].as<double>(); }
    if (!s_dev && accumulate) FZCHK(copy_in(c, d_out, stack, (size_t)Gx * Gy * 8));
    // host rows are staged in chunks of whole rows (half of the workspace; the other half is for the partial tiles)
    int64_t nc = p_dev ? std::max<int64_t>(Nrows, 1) : std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / 2 / (Gy * 8), (int64_t)1 << 22));
    nc = std::min(nc, std::max<int64_t>(Nrows, 1));
    const size_t lds = (size_t)2 * 2 * FZ_GEMM_BK * FZ_GEMM_LD * 8;
    HIPCHK(hipFuncSetAttribute((const void*)k_stack2d, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<StackObj> objs; std::vector<StackItem> items; std::vector<int2> tiles(ntx);
    bool first = true;
    for (int64_t i0 = 0; first || i0 < Nrows; i0 += nc) {
        const int64_t n = std::min(nc, Nrows - i0);
        objs.clear();
        for (int64_t k = 0; k < nsel; ++k) {
            if (rows[k] < i0 || rows[k] >= i0 + n) continue;
            const int64_t w = c->h_widths[eidx[k]];
            StackObj o; o.cut = 0.0; o.scale = weff[k]; o.row = p_dev ? rows[k] : rows[k] - i0; o.koff = c->h_offsets[eidx[k]];
            o.start = (int32_t)(cent[k] - w); o.len = (int32_t)(2 * w + 1);
            objs.push_back(o);
        }
        const int ns = (int)objs.size();
        // object range of every x tile: the sorted objects whose window can reach it, by the largest half-width
        items.clear();
        std::vector<std::pair<int, int>> range(ntx);
        int64_t total = 0;
        for (int tx = 0; tx < ntx; ++tx) {
            int lo = 0, hi = ns;
            if (!full_range) {
                const int64_t xlo = (int64_t)tx * FZ_GEMM_BM - wmax, xhi = (int64_t)tx * FZ_GEMM_BM + FZ_GEMM_BM - 1 + wmax;
                lo = (int)(std::lower_bound(objs.begin(), objs.end(), xlo, [&](const StackObj& o, int64_t v) { return (int64_t)o.start + (o.len >> 1) < v; }) - objs.begin());
                hi = (int)(std::upper_bound(objs.begin(), objs.end(), xhi, [&](int64_t v, const StackObj& o) { return v < (int64_t)o.start + (o.len >> 1); }) - objs.begin());
            }
            range[tx] = {lo, std::max(lo, hi)};
            total += range[tx].second - lo;
        }
        // ... split over blocks so that the tiles fill the card; a split is a whole number of k-steps
        const int64_t max_items = std::max<int64_t>(ntx, c->ws_limit / 2 / (int64_t)(tile_bytes * nty));
        int64_t want = std::min<int64_t>(max_items, std::max<int64_t>(ntx, (int64_t)2 * c->cu_count / nty));
        int64_t per = std::max<int64_t>(1, (total + want - 1) / want);
        per = (per + FZ_GEMM_BK - 1) / FZ_GEMM_BK * FZ_GEMM_BK;
        for (;;) {
            items.clear();
            for (int tx = 0; tx < ntx; ++tx) {
                tiles[tx].x = (int)items.size();
                for (int64_t k0 = range[tx].first; k0 < range[tx].second; k0 += per)
                    items.push_back(StackItem{tx, (int32_t)k0, (int32_t)std::min<int64_t>(k0 + per, range[tx].second), 0});
                tiles[tx].y = (int)items.size() - tiles[tx].x;
            }
            if ((int64_t)items.size() <= max_items + ntx) break;
            per *= 2;
        }
        const int ni = (int)items.size();
        if (ns > 0) {
            const double* dp;
            FZCHK(pv.at(i0, n, &dp));                              // (device rows: one chunk, i0 = 0, and o.row counts from the first row)
            FZCHK(c->d_net[0].ensure((size_t)ns * sizeof(StackObj))); FZCHK(copy_in(c, c->d_net[0].p, objs.data(), (size_t)ns * sizeof(StackObj)));
            FZCHK(c->d_net[1].ensure((size_t)std::max(ni, 1) * sizeof(StackItem))); FZCHK(copy_in(c, c->d_net[1].p, items.data(), (size_t)ni * sizeof(StackItem)));
            FZCHK(c->d_net[3].ensure(8));
            int bad = 0x7fffffff;
            FZCHK(copy_in(c, c->d_net[3].p, &bad, 4));
            FZCHK(c->d_pl[0].ensure((size_t)std::max(ni, 1) * nty * tile_bytes));
            {
                Timer t(c, &c->tm.ms_other, &c->tm.n_other);
                hipLaunchKernelGGL(k_stack_rows, dim3((unsigned)((ns + 3) / 4)), dim3(256), 0, c->stream, dp, (int)Gy, (int)Gx, c->d_kern.as<double>(),
                                   c->d_net[0].as<StackObj>(), ns, pdf_thresh, prepared ? 1 : 0, c->d_net[3].as<int>());
            }
            HIPCHK(hipGetLastError());
            FZCHK(copy_out(c, &bad, c->d_net[3].p, 4));
            if (bad != 0x7fffffff) return fail(-4, "fz_stack2d: the PDF of the object at row %lld holds a value that is not finite", (long long)(objs[bad].row + (p_dev ? 0 : i0)));
            if (ni > 0) {
                Timer t(c, &c->tm.ms_other, &c->tm.n_other);
                hipLaunchKernelGGL(k_stack2d, dim3((unsigned)ni, (unsigned)nty), dim3(256), lds, c->stream, dp, (int)Gy, (int)Gx, c->d_kern.as<double>(),
                                   c->d_net[0].as<StackObj>(), c->d_net[1].as<StackItem>(), c->d_pl[0].as<double>());
            }
            HIPCHK(hipGetLastError());
        } else {
            for (int tx = 0; tx < ntx; ++tx) tiles[tx] = int2{0, 0};
            FZCHK(c->d_pl[0].ensure(tile_bytes));
        }
        FZCHK(c->d_net[2].ensure((size_t)ntx * sizeof(int2))); FZCHK(copy_in(c, c->d_net[2].p, tiles.data(), (size_t)ntx * sizeof(int2)));
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            hipLaunchKernelGGL(k_stack_add, dim3((unsigned)((Gx * Gy + 255) / 256)), dim3(256), 0, c->stream, c->d_pl[0].as<double>(), c->d_net[2].as<int2>(), nty,
                               (int)Gx, (int)Gy, (accumulate || !first) ? 1 : 0, d_out);
        }
        HIPCHK(hipGetLastError());
        first = false;
        if (Nrows <= 0) break;
    }
    if (!s_dev) FZCHK(copy_out(c, stack, d_out, (size_t)Gx * Gy * 8));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_recentre_rows(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, const double* pgrid, const double* cent,
                                int32_t disp, int64_t Gd, const double* dgrid, double* out) {
    if (!c || !pdfs || !pgrid || !cent || !dgrid || !out) return fail(-1, "fz_recentre_rows: NULL argument");
    if (G < 1 || Gd < 1 || G >= ((int64_t)1 << 30) || Gd >= ((int64_t)1 << 30)) return fail(-1, "fz_recentre_rows: bad grid");
    if (disp != 0 && disp != 1) return fail(-1, "fz_recentre_rows: dispersion %d not in {0, 1}", disp);
    if (N <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, pgrid, cent, dgrid, out}));
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_IN), cv(c, cent, 8, c->d_lmap, STAGE_IN), ov(c, out, (size_t)Gd * 8, c->d_pl[0], STAGE_OUT);
    FZCHK(c->d_sgrid.ensure((size_t)(G + Gd) * 8));
    FZCHK(copy_in(c, c->d_sgrid.p, pgrid, (size_t)G * 8));
    FZCHK(copy_in(c, c->d_sgrid.as<double>() + G, dgrid, (size_t)Gd * 8));
    int64_t nc = std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / ((G + Gd) * 8 + 8), (int64_t)1 << 20));
    nc = std::min(nc, N);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dp; const double* dc; double* dout;
        FZCHK(pv.at(i0, n, &dp)); FZCHK(cv.at(i0, n, &dc)); FZCHK(ov.at(i0, n, &dout));
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            hipLaunchKernelGGL(k_recentre, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, dp, n, (int)G, c->d_sgrid.as<double>(), dc, (int)disp,
                               (int)Gd, c->d_sgrid.as<double>() + G, dout);
        }
        HIPCHK(hipGetLastError());
        FZCHK(ov.back(i0, n));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_cdf_draws(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, const double* grid, const double* mc, int64_t Nmc,
                            const double* weights, const double* edges, int64_t Nbins, double* draws, double* hist) {
    if (!c || !pdfs || !grid || !mc) return fail(-1, "fz_cdf_draws: NULL argument");
    if (!draws && !hist) return fail(-1, "fz_cdf_draws: neither the draws nor the histogram is asked for");
    if (hist && (!weights || !edges || Nbins < 1 || Nbins > 4096)) return fail(-1, "fz_cdf_draws: the histogram needs weights and 1..4096 bins with their edges");
    if (G < 2 || G > FZ_SUM_MAXG) return fail(-5, "fz_cdf_draws: grid of %lld points unsupported (2..%d: one CDF row per wave in LDS)", (long long)G, FZ_SUM_MAXG);
    if (Nmc < 1 || Nmc >= ((int64_t)1 << 30)) return fail(-1, "fz_cdf_draws: bad number of draws");
    if (N <= 0) { if (hist && !is_device_ptr(hist)) std::fill(hist, hist + Nbins, 0.0); return 0; }
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, grid, mc, weights, edges, draws, hist}));
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_IN), mv(c, mc, (size_t)Nmc * 8, c->d_pl[0], STAGE_IN);
    const StageRows dv(c, draws, (size_t)Nmc * 8, c->d_pl[1], STAGE_OUT), wv(c, hist ? weights : nullptr, 8, c->d_lmap, STAGE_IN);
    const int nb = hist ? (int)Nbins : 0;
    FZCHK(c->d_sgrid.ensure((size_t)(G + nb + 1) * 8));
    FZCHK(copy_in(c, c->d_sgrid.p, grid, (size_t)G * 8));
    if (hist) FZCHK(copy_in(c, c->d_sgrid.as<double>() + G, edges, (size_t)(nb + 1) * 8));
    const int64_t per_obj = (pv.dev ? 0 : G * 8) + (mv.dev ? 0 : Nmc * 8) + (dv.staged() ? Nmc * 8 : 0) + 8;
    int64_t nc = std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / per_obj, (int64_t)1 << 22));
    nc = std::min(nc, N);
    const int wpb = G <= 4800 ? 4 : (G <= 9600 ? 2 : 1);               // waves per block: one CDF row each in LDS (as k_summarize)
    const size_t lds = (size_t)wpb * (G * 8 + (size_t)nb * 12) + 8;
    if (lds > 160 * 1024) return fail(-5, "fz_cdf_draws: %lld grid points with %d bins do not fit the LDS", (long long)G, nb);
    HIPCHK(hipFuncSetAttribute((const void*)k_cdf_draws, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<double> total(nb, 0.0), chunk(nb);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double *dp, *dm, *dw; double* dd;
        FZCHK(pv.at(i0, n, &dp)); FZCHK(mv.at(i0, n, &dm)); FZCHK(dv.at(i0, n, &dd)); FZCHK(wv.at(i0, n, &dw));
        // a block serves a run of objects, so that the histogram has a few thousand partial rows whatever N
        const int64_t opb = std::max<int64_t>(wpb, (n + (int64_t)4 * c->cu_count - 1) / ((int64_t)4 * c->cu_count));
        const int64_t nblk = (n + opb - 1) / opb, P = nblk * wpb;
        double* hp = nullptr;
        if (hist) { FZCHK(c->d_pl[2].ensure((size_t)(P + 1) * nb * 8)); hp = c->d_pl[2].as<double>(); }
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            hipLaunchKernelGGL(k_cdf_draws, dim3((unsigned)nblk), dim3(wpb * 64), lds, c->stream, dp, n, (int)G, c->d_sgrid.as<double>(), dm, (int)Nmc, dw,
                               c->d_sgrid.as<double>() + G, nb, (int)opb, dd, hp);
            for (int b = 0; b < nb; ++b)
                hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, hp + (int64_t)b * P, P, hp + P * nb + b);
        }
        HIPCHK(hipGetLastError());
        FZCHK(dv.back(i0, n));
        if (hist) {
            FZCHK(copy_out(c, chunk.data(), hp + P * nb, (size_t)nb * 8));
            for (int b = 0; b < nb; ++b) total[b] += chunk[b];
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (hist) FZCHK(host_write(hist, total.data(), (size_t)nb * 8));
    return 0;
}
