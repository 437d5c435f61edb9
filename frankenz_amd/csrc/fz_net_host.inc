// ---- networks.py ABI: inference through a trained network (fz_net.h) --------------------------------
// Every array may live in host or device memory; host arrays are staged through the context's buffers (StageWhole, fz_stage.h).

extern "C" int fz_net_select(fz_ctx* c, const double* lnprob, int64_t N, int32_t Nn, int32_t use_wt, double wt_thresh, double cdf_thresh,
                             const int32_t* match, const int64_t* csr_off, int64_t Nnodes, int32_t* nsel, int32_t* sel, int64_t* rawlen,
                             double* lmap, double* levid) {
    if (!c || !lnprob || !nsel || !sel) return fail(-1, "fz_net_select: NULL argument");
    if (N <= 0) return 0;
    if (Nn <= 0 || Nn > 4096) return fail(-5, "fz_net_select: %d nodes unsupported (limit: 1..4096 matched nodes, an object's row of node ln-probabilities sits in LDS)", Nn);
    if (!use_wt && !(cdf_thresh > 0.0 && cdf_thresh < 1.0)) return fail(-4, "cdf_thresh must lie in (0, 1)");
    if (rawlen && !csr_off) return fail(-1, "fz_net_select: rawlen needs the node lists' offsets");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {lnprob, match, csr_off, nsel, sel, rawlen, lmap, levid}));
    StageWhole st{c};
    const void *d_lp, *d_match, *d_off; void *d_nsel, *d_sel, *d_raw, *d_lm, *d_le;
    FZCHK(st.in(lnprob, (size_t)N * Nn * 8, &d_lp)); FZCHK(st.in(match, (size_t)Nn * 4, &d_match));
    FZCHK(st.in(csr_off, csr_off ? (size_t)(Nnodes + 1) * 8 : 0, &d_off));
    FZCHK(st.out(nsel, (size_t)N * 4, &d_nsel)); FZCHK(st.out(sel, (size_t)N * Nn * 4, &d_sel)); FZCHK(st.out(rawlen, (size_t)N * 8, &d_raw));
    FZCHK(st.out(lmap, (size_t)N * 8, &d_lm)); FZCHK(st.out(levid, (size_t)N * 8, &d_le));
    // a wave per object, 16 Nn bytes of LDS each (the row, and the CDF rule's order): four waves a block up to 2 560 nodes (160 KB),
    // two up to 4 096 (128 KB)
    const int waves = Nn <= 2560 ? 4 : 2;
    const size_t lds = (size_t)waves * 2 * Nn * 8;
    HIPCHK(hipFuncSetAttribute((const void*)fz::k_net_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_net_select, dim3((unsigned)((N + waves - 1) / waves)), dim3(64 * waves), lds, c->stream, (const double*)d_lp, N, (int)Nn, (int)use_wt,
                           wt_thresh, cdf_thresh, (const int32_t*)d_match, (const int64_t*)d_off, (int32_t*)d_nsel, (int32_t*)d_sel, (int64_t*)d_raw,
                           (double*)d_lm, (double*)d_le);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_net_table(fz_ctx* c, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn, const int32_t* match,
                            const int64_t* csr_off, const int64_t* csr_items, int64_t Nnodes, int64_t W, int64_t* idx) {
    if (!c || !nsel || !sel || !csr_off || !csr_items || !idx) return fail(-1, "fz_net_table: NULL argument");
    if (N <= 0 || W <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {nsel, sel, match, csr_off, csr_items, idx}));
    StageWhole st{c};
    const void *d_nsel, *d_sel, *d_match, *d_off, *d_items; void* d_idx;
    int64_t nitems = 0;
    FZCHK(host_read(&nitems, csr_off + Nnodes, 8));
    FZCHK(st.in(nsel, (size_t)N * 4, &d_nsel)); FZCHK(st.in(sel, (size_t)N * Nn * 4, &d_sel)); FZCHK(st.in(match, (size_t)Nn * 4, &d_match));
    FZCHK(st.in(csr_off, (size_t)(Nnodes + 1) * 8, &d_off)); FZCHK(st.in(csr_items, (size_t)nitems * 8, &d_items));
    FZCHK(st.out(idx, (size_t)N * W * 8, &d_idx));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_net_table, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, (const int32_t*)d_nsel, (const int32_t*)d_sel, N, (int)Nn,
                           (const int32_t*)d_match, (const int64_t*)d_off, (const int64_t*)d_items, W, (int64_t*)d_idx);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_net_union(fz_ctx* c, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn, const int32_t* match,
                            const int64_t* csr_off, const int64_t* csr_items, int64_t Nnodes, int64_t M, int64_t W, int64_t* nuniq, int64_t* idx) {
    if (!c || !nsel || !sel || !csr_off || !csr_items || !nuniq) return fail(-1, "fz_net_union: NULL argument");
    if (M < 1 || Nn < 1 || Nnodes < 1) return fail(-4, "fz_net_union: %lld models, %d columns, %lld nodes", (long long)M, Nn, (long long)Nnodes);
    if (M > FZ_NET_UNION_MMAX)
        return fail(-5, "fz_net_union: %lld models exceed FZ_NET_UNION_MMAX = %d (an object's bitmap of M bits sits in LDS)", (long long)M, FZ_NET_UNION_MMAX);
    if (idx && W < 1) return fail(-4, "fz_net_union: a table of width %lld", (long long)W);
    if (N <= 0) return 0;
    if (N >= ((int64_t)1 << 31)) return fail(-5, "fz_net_union: %lld objects in one call", (long long)N);
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {nsel, sel, match, csr_off, csr_items, nuniq, idx}));
    StageWhole st{c};
    const void *d_nsel, *d_sel, *d_match, *d_off, *d_items; void *d_nu, *d_idx, *d_reach;
    int64_t nitems = 0;
    FZCHK(host_read(&nitems, csr_off + Nnodes, 8));
    if (nitems < 0) return fail(-4, "fz_net_union: the node lists end at %lld", (long long)nitems);
    FZCHK(st.in(nsel, (size_t)N * 4, &d_nsel)); FZCHK(st.in(sel, (size_t)N * Nn * 4, &d_sel)); FZCHK(st.in(match, (size_t)Nn * 4, &d_match));
    FZCHK(st.in(csr_off, (size_t)(Nnodes + 1) * 8, &d_off)); FZCHK(st.in(csr_items, (size_t)nitems * 8, &d_items));
    FZCHK(st.out(nuniq, (size_t)N * 8, &d_nu));
    FZCHK(st.out(idx, idx ? (size_t)N * W * 8 : 0, &d_idx));
    FZCHK(st.slot((size_t)Nnodes * 4, &d_reach));
    // every index the selection reaches is checked before a row is written: the nodes some object selects, then their lists
    HIPCHK(hipMemsetAsync(d_reach, 0, (size_t)Nnodes * 4, c->stream));
    int ef = 0;
    FZCHK(fz_flag_roundtrip(c, ef, [&](int* d_flags) {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_net_reach, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, (const int32_t*)d_nsel, (const int32_t*)d_sel, N,
                           (int)Nn, (const int32_t*)d_match, Nnodes, (int32_t*)d_reach, (int32_t*)d_flags);
        hipLaunchKernelGGL(fz::k_net_check, dim3((unsigned)((Nnodes + 3) / 4)), dim3(256), 0, c->stream, (const int32_t*)d_reach, Nnodes,
                           (const int64_t*)d_off, (const int64_t*)d_items, nitems, M, (int32_t*)d_flags);
        return 0;
    }));
    if (ef & 2) return fail(-3, "fz_net_union: the selection, `match` or the lists' offsets point outside their tables");
    if (ef & 1) return fail(-3, "fz_net_union: a list that a selected node reaches holds a model index outside [0, %lld)", (long long)M);
    // a wave per object, a bitmap of ceil(M / 32) words each: four waves a block while four bitmaps fit in LDS, then two, then one
    const int waves = fz::fz_net_union_waves(M);
    const size_t lds = (size_t)waves * fz::fz_net_union_words(M) * 4;
    const void* kern = idx ? (const void*)fz::k_net_union<true> : (const void*)fz::k_net_union<false>;
    HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        const dim3 grid((unsigned)((N + waves - 1) / waves)), blk(64 * waves);
        if (idx) hipLaunchKernelGGL(fz::k_net_union<true>, grid, blk, lds, c->stream, (const int32_t*)d_nsel, (const int32_t*)d_sel, N, (int)Nn,
                                    (const int32_t*)d_match, (const int64_t*)d_off, (const int64_t*)d_items, M, W, (int64_t*)d_nu, (int64_t*)d_idx);
        else hipLaunchKernelGGL(fz::k_net_union<false>, grid, blk, lds, c->stream, (const int32_t*)d_nsel, (const int32_t*)d_sel, N, (int)Nn,
                                (const int32_t*)d_match, (const int64_t*)d_off, (const int64_t*)d_items, M, (int64_t)0, (int64_t*)d_nu, (int64_t*)nullptr);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_net_gather(fz_ctx* c, const void* plane, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn, int32_t W,
                             uint64_t pad_bits, void* out) {
    if (!c || !plane || !nsel || !sel || !out) return fail(-1, "fz_net_gather: NULL argument");
    if (N <= 0 || W <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {plane, nsel, sel, out}));
    StageWhole st{c};
    const void *d_pl, *d_nsel, *d_sel; void* d_out;
    FZCHK(st.in(plane, (size_t)N * Nn * 8, &d_pl)); FZCHK(st.in(nsel, (size_t)N * 4, &d_nsel)); FZCHK(st.in(sel, (size_t)N * Nn * 4, &d_sel));
    FZCHK(st.out(out, (size_t)N * W * 8, &d_out));
    const int64_t tot = N * W;
    hipLaunchKernelGGL(fz::k_net_gather, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)d_pl, (const int32_t*)d_nsel,
                       (const int32_t*)d_sel, N, (int)Nn, (int)W, (unsigned long long)pad_bits, (unsigned long long*)d_out);
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_net_stack(fz_ctx* c, const double* lnprob, const int32_t* nsel, const int32_t* sel, int64_t N, int32_t Nn, const int32_t* match,
                            const double* node_pdfs, int64_t Nnodes, int64_t G, double* pdfs, double* lmap, double* levid) {
    if (!c || !lnprob || !nsel || !sel || !node_pdfs || !pdfs) return fail(-1, "fz_net_stack: NULL argument");
    if (N <= 0 || G <= 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {lnprob, nsel, sel, match, node_pdfs, pdfs, lmap, levid}));
    StageWhole st{c};
    const void *d_lp, *d_nsel, *d_sel, *d_match, *d_np; void *d_pdf, *d_lm, *d_le;
    FZCHK(st.in(lnprob, (size_t)N * Nn * 8, &d_lp)); FZCHK(st.in(nsel, (size_t)N * 4, &d_nsel)); FZCHK(st.in(sel, (size_t)N * Nn * 4, &d_sel));
    FZCHK(st.in(match, (size_t)Nn * 4, &d_match)); FZCHK(st.in(node_pdfs, (size_t)Nnodes * G * 8, &d_np));
    FZCHK(st.out(pdfs, (size_t)N * G * 8, &d_pdf)); FZCHK(st.out(lmap, (size_t)N * 8, &d_lm)); FZCHK(st.out(levid, (size_t)N * 8, &d_le));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_net_stack, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, c->stream, (const double*)d_lp, (const int32_t*)d_nsel,
                           (const int32_t*)d_sel, N, (int)Nn, (const int32_t*)d_match, (const double*)d_np, (int)G, (double*)d_pdf, (double*)d_lm, (double*)d_le);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
