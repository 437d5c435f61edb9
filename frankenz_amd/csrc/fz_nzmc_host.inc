// ---- samplers.py ABI: the n(z) samplers' chains (kernels in fz_nzmc.h; docs/samplers.md) ----------------------
// The stack (N, G) and the per-object state (overlap, the pair's difference column) are DEVICE arrays of the caller: they stay
// resident over a whole chain.  The G-sized and table arguments may live in host or device memory (StageWhole, fz_stage.h).
namespace {
// scratch of a chain call: block partials of two sums, and the NzState
int nz_scratch(fz_ctx* c, int64_t nblk, double** partial, fz::NzState** st) {
    FZCHK(c->d_pl[1].ensure((size_t)nblk * 2 * 8 + 64));
    FZCHK(c->d_flags.ensure(sizeof(fz::NzState) > 64 ? sizeof(fz::NzState) : 64));
    *partial = c->d_pl[1].as<double>(); *st = c->d_flags.as<fz::NzState>();
    return 0;
}
int nz_check_resident(const char* fn, const double* pdfs, const double* overlap, const double* dcol, int64_t N, int64_t G) {
    if (N <= 0 || G < 2 || G >= ((int64_t)1 << 24)) return fail(-4, "%s: bad shape (%lld objects, %lld bins; at least two bins)", fn, (long long)N, (long long)G);
    if (!is_device_ptr(pdfs) || !is_device_ptr(overlap) || !is_device_ptr(dcol))
        return fail(-4, "%s: pdfs, overlap and the difference column must be device arrays (they stay resident over the chain)", fn);
    return 0;
}
}  // namespace

// device memory for state that outlives a call (the samplers' resident stack and per-object state)
extern "C" int fz_dev_alloc(fz_ctx* c, int64_t bytes, void** out) {
    if (!c || !out || bytes < 0) return fail(-1, "fz_dev_alloc: bad argument");
    HIPCHK(hipSetDevice(c->device));
    *out = nullptr;
    if (hipMalloc(out, (size_t)(bytes ? bytes : 8)) != hipSuccess) { (void)hipGetLastError(); return fail(-2, "fz_dev_alloc: %lld bytes of device memory refused", (long long)bytes); }
    return 0;
}
extern "C" int fz_dev_free(fz_ctx* c, void* p) {
    if (!c) return fail(-1, "fz_dev_free: NULL context");
    if (p) { HIPCHK(hipSetDevice(c->device)); HIPCHK(hipFree(p)); }
    return 0;
}
// bytes from src to dst, either side in host or device memory, complete on return
extern "C" int fz_dev_copy(fz_ctx* c, void* dst, const void* src, int64_t bytes) {
    if (!c || !dst || !src || bytes < 0) return fail(-1, "fz_dev_copy: bad argument");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {dst, src}));
    if (bytes) HIPCHK(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDefault, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_pdfs_colsum(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, double* colsum) {
    if (!c || !pdfs || !colsum) return fail(-1, "fz_pdfs_colsum: NULL argument");
    if (N <= 0 || G <= 0 || G >= ((int64_t)1 << 24)) return fail(-4, "fz_pdfs_colsum: bad shape");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, colsum}));
    // block b owns rows [b * NZ_COLROWS, ...) of the WHOLE stack, also when a host stack is staged in pieces: one summation order
    const int64_t nblk = (N + NZ_COLROWS - 1) / NZ_COLROWS;
    FZCHK(c->d_pl[0].ensure((size_t)nblk * G * 8));
    double* part = c->d_pl[0].as<double>();
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_IN);
    int64_t nc = pv.dev ? N : std::max<int64_t>(NZ_COLROWS, std::min<int64_t>(c->ws_limit / (G * 8), (int64_t)1 << 22) / NZ_COLROWS * NZ_COLROWS);
    nc = std::min(nc, N);
    StageWhole st{c};
    void* d_out; FZCHK(st.out(colsum, (size_t)G * 8, &d_out));
    {
        for (int64_t i0 = 0; i0 < N; i0 += nc) {
            const int64_t n = std::min(nc, N - i0);
            const double* dp;
            FZCHK(pv.at(i0, n, &dp));
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            hipLaunchKernelGGL(fz::k_colsum_part, dim3((unsigned)((n + NZ_COLROWS - 1) / NZ_COLROWS)), dim3(NZ_NT), 0, c->stream, dp, n, (int)G,
                               part + (i0 / NZ_COLROWS) * G);
        }
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(fz::k_colsum_fin, dim3((unsigned)((G + NZ_NT - 1) / NZ_NT)), dim3(NZ_NT), 0, c->stream, part, nblk, (int)G, (double*)d_out);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int fz_nz_pairs(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, double* pos, double* overlap, double* dcol, double* lnpost,
                           const int64_t* pairs, const double* normals, const double* expo, int64_t nsamp, int32_t thin, int32_t mh_steps,
                           int64_t s0, int64_t s1, double* samples, double* samples_lnp, int32_t* accept, double* gscale) {
    if (!c || !pdfs || !pos || !overlap || !dcol || !lnpost || !pairs || !normals || !expo || !samples || !samples_lnp || !accept || !gscale)
        return fail(-1, "fz_nz_pairs: NULL argument");
    FZCHK(nz_check_resident("fz_nz_pairs", pdfs, overlap, dcol, N, G));
    if (thin <= 0 || mh_steps <= 0 || nsamp <= 0) return fail(-4, "fz_nz_pairs: thin, mh_steps and the number of samples must be positive");
    if (s0 < 0 || s1 > nsamp || s0 > s1) return fail(-4, "fz_nz_pairs: sample range [%lld, %lld) outside [0, %lld)", (long long)s0, (long long)s1, (long long)nsamp);
    if (s0 == s1) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, pos, overlap, dcol, lnpost, pairs, normals, expo, samples, samples_lnp, accept, gscale}));
    const int64_t P = nsamp * thin, p0 = s0 * thin, p1 = s1 * thin;
    // the pairs index the stack's columns on the device: checked here
    {
        std::vector<int64_t> pr((size_t)(p1 - p0) * 2);
        FZCHK(host_read(pr.data(), pairs + 2 * p0, pr.size() * 8));
        for (int64_t v : pr) if (v < 0 || v >= G) return fail(-3, "fz_nz_pairs: bin %lld of a pair outside [0, %lld)", (long long)v, (long long)G);
    }
    StageWhole st{c};
    const void *d_pairs, *d_nrm, *d_exp; void *d_pos, *d_lnp, *d_smp, *d_slnp, *d_acc, *d_gs;
    FZCHK(st.in(pairs, (size_t)P * 16, &d_pairs)); FZCHK(st.in(normals, (size_t)P * mh_steps * 8, &d_nrm)); FZCHK(st.in(expo, (size_t)P * mh_steps * 8, &d_exp));
    // in/out and partly written arrays: a staged copy starts from the caller's values
    FZCHK(st.inout(pos, (size_t)G * 8, &d_pos)); FZCHK(st.inout(lnpost, 8, &d_lnp));
    FZCHK(st.inout(samples, (size_t)nsamp * G * 8, &d_smp)); FZCHK(st.inout(samples_lnp, (size_t)nsamp * 8, &d_slnp));
    FZCHK(st.inout(accept, (size_t)P * mh_steps * 4, &d_acc)); FZCHK(st.inout(gscale, (size_t)P * 8, &d_gs));
    const int64_t nblk = (N + NZ_CHUNK - 1) / NZ_CHUNK;
    double* part; fz::NzState* ns;
    FZCHK(nz_scratch(c, nblk, &part, &ns));
    fz::NzChain ch;
    ch.pairs = (const int64_t*)d_pairs; ch.normals = (const double*)d_nrm; ch.expo = (const double*)d_exp; ch.pos = (double*)d_pos;
    ch.lnpost = (double*)d_lnp; ch.samples = (double*)d_smp; ch.samples_lnp = (double*)d_slnp; ch.accept = (int32_t*)d_acc;
    ch.gscale = (double*)d_gs; ch.G = (int)G; ch.thin = thin; ch.mh = mh_steps;
    {
        // the whole segment is enqueued without a host synchronisation: the order of the stream is the chain's order
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        const dim3 grid((unsigned)nblk), blk(NZ_NT);
        hipLaunchKernelGGL(fz::k_pair_begin, dim3(1), dim3(1), 0, c->stream, ch, p0, ns);
        for (int64_t p = p0; p < p1; ++p) {
            hipLaunchKernelGGL(fz::k_pair_open, grid, blk, 0, c->stream, pdfs, N, (int)G, (const fz::NzState*)ns, overlap, dcol, part, nblk);
            hipLaunchKernelGGL(fz::k_pair_grad, dim3(1), blk, 0, c->stream, ch, p, (const double*)part, nblk, ns);
            for (int k = 0; k < mh_steps; ++k) {
                hipLaunchKernelGGL(fz::k_pair_try, grid, blk, 0, c->stream, N, (const fz::NzState*)ns, overlap, (const double*)dcol, part);
                hipLaunchKernelGGL(fz::k_pair_decide, dim3(1), blk, 0, c->stream, ch, p, k, p1, (const double*)part, nblk, ns);
            }
        }
        hipLaunchKernelGGL(fz::k_pair_flush, dim3((unsigned)((N + NZ_NT - 1) / NZ_NT)), blk, 0, c->stream, N, (const fz::NzState*)ns, overlap,
                           (const double*)dcol);
        hipLaunchKernelGGL(fz::k_pair_flushed, dim3(1), dim3(1), 0, c->stream, ns);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// The per-evaluation form (a user's ln-prior is a Python callable on pos: the host takes every decision).  what = 0: a new pair
// (pair_i, pair_j) -- the pending step is applied with the previous pair's column, the column gathered, sums[0..1] =
// sum(log(overlap +- step * d)); what = 1: sums[0] = sum(log(overlap + step * d)) after the pending step; what = 2: the pending step
// only.  pend_step is the accepted step not yet applied (has_pend != 0).
extern "C" int fz_nz_pair_eval(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, double* overlap, double* dcol, int32_t what,
                               int64_t pair_i, int64_t pair_j, int32_t has_pend, double pend_step, double step, double* sums) {
    if (!c || !pdfs || !overlap || !dcol || !sums) return fail(-1, "fz_nz_pair_eval: NULL argument");
    FZCHK(nz_check_resident("fz_nz_pair_eval", pdfs, overlap, dcol, N, G));
    if (what < 0 || what > 2) return fail(-4, "fz_nz_pair_eval: unknown request %d", (int)what);
    if (what == 0 && (pair_i < 0 || pair_j < 0 || pair_i >= G || pair_j >= G)) return fail(-3, "fz_nz_pair_eval: pair index out of range");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, overlap, dcol}));
    const int64_t nblk = (N + NZ_CHUNK - 1) / NZ_CHUNK;
    double* part; fz::NzState* ns;
    FZCHK(nz_scratch(c, nblk, &part, &ns));
    fz::NzState h;
    std::memset(&h, 0, sizeof h);
    h.pi = (int32_t)pair_i; h.pj = (int32_t)pair_j; h.has_pend = has_pend ? 1 : 0; h.pend = pend_step; h.h = step; h.z = step; h.valid = what == 1;
    FZCHK(copy_in(c, ns, &h, sizeof h));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        const dim3 grid((unsigned)nblk), blk(NZ_NT);
        if (what == 0) {
            hipLaunchKernelGGL(fz::k_pair_open, grid, blk, 0, c->stream, pdfs, N, (int)G, (const fz::NzState*)ns, overlap, dcol, part, nblk);
            hipLaunchKernelGGL(fz::k_pair_sums, dim3(1), blk, 0, c->stream, (const double*)part, nblk, 2, ns);
        } else if (what == 1) {
            hipLaunchKernelGGL(fz::k_pair_try, grid, blk, 0, c->stream, N, (const fz::NzState*)ns, overlap, (const double*)dcol, part);
            hipLaunchKernelGGL(fz::k_pair_sums, dim3(1), blk, 0, c->stream, (const double*)part, nblk, 1, ns);
        } else {
            hipLaunchKernelGGL(fz::k_pair_flush, dim3((unsigned)((N + NZ_NT - 1) / NZ_NT)), blk, 0, c->stream, N, (const fz::NzState*)ns, overlap,
                               (const double*)dcol);
        }
    }
    HIPCHK(hipGetLastError());
    FZCHK(copy_out(c, &h, ns, sizeof h));
    sums[0] = h.sum[0]; sums[1] = h.sum[1];
    return 0;
}

extern "C" int fz_nz_sweep(fz_ctx* c, const double* pdfs, int64_t N, int64_t G, const double* nz, const double* u, int32_t use_philox,
                           uint32_t key0, uint32_t key1, uint64_t sweep, int64_t* counts) {
    if (!c || !pdfs || !nz || !counts) return fail(-1, "fz_nz_sweep: NULL argument");
    if (!use_philox && !u) return fail(-1, "fz_nz_sweep: no uniforms and no generator");
    if (N <= 0 || G <= 0 || G >= ((int64_t)1 << 24)) return fail(-4, "fz_nz_sweep: bad shape");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {pdfs, nz, u, counts}));
    const StageRows pv(c, pdfs, (size_t)G * 8, c->d_pdfs, STAGE_IN), uv(c, use_philox ? nullptr : u, 8, c->d_lmap, STAGE_IN);
    const bool c_dev = is_device_ptr(counts);
    FZCHK(c->d_sgrid.ensure((size_t)G * 8)); FZCHK(copy_in(c, c->d_sgrid.p, nz, (size_t)G * 8));
    FZCHK(c->d_sloss.ensure((size_t)G * 8));
    HIPCHK(hipMemsetAsync(c->d_sloss.p, 0, (size_t)G * 8, c->stream));
    int64_t nc = pv.dev ? N : std::max<int64_t>(1, std::min<int64_t>(c->ws_limit / (G * 8 + 32), (int64_t)1 << 22));
    nc = std::min(nc, N);
    const size_t rows_lds = (size_t)4 * G * 8;                  // as fz_nz_assign: four rows of p * nz in LDS up to 48 KB
    const int staged = rows_lds <= 48 * 1024;
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double* dp; const double* du;
        FZCHK(pv.at(i0, n, &dp)); FZCHK(uv.at(i0, n, &du));
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        const dim3 grid((unsigned)((n + 3) / 4)), blk(256);
        if (use_philox)
            hipLaunchKernelGGL(fz::k_nz_sweep<true>, grid, blk, staged ? rows_lds : 0, c->stream, dp, n, (int)G, c->d_sgrid.as<double>(), du, key0, key1,
                               sweep, i0, c->d_sloss.as<unsigned long long>(), staged);
        else
            hipLaunchKernelGGL(fz::k_nz_sweep<false>, grid, blk, staged ? rows_lds : 0, c->stream, dp, n, (int)G, c->d_sgrid.as<double>(), du, key0, key1,
                               sweep, i0, c->d_sloss.as<unsigned long long>(), staged);
    }
    HIPCHK(hipGetLastError());
    if (c_dev) HIPCHK(hipMemcpyAsync(counts, c->d_sloss.p, (size_t)G * 8, hipMemcpyDeviceToDevice, c->stream));
    else FZCHK(copy_out(c, counts, c->d_sloss.p, (size_t)G * 8));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
