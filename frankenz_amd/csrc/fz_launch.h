// Launch geometry of the softmax / KDE kernels (templates over the ln-weight source).
#pragma once
#include "fz_ctx.h"
#include "fz_grid.h"
#include "fz_kernels.h"
#include "fz_nolist.h"
#include "fz_hist.h"
#include "fz_hist_order.h"
#include "fz_plane.h"

// ---- launch helpers ------------------------------------------------------------
// What every launcher of a chunk passes on: the context, the chunk's objects and models, the KDE options and the three outputs
struct fz_call { fz_ctx* c; int64_t n, M; const fz_kde_opts* ko; double *lmap, *levid, *pdfs; };

// Run-time pair -> template arguments: r = f(fz_pair<A, B>{}) of the listed pair that matches (a, b); false when none does
template <int A_, int B_> struct fz_pair { static constexpr int A = A_, B = B_; };
template <class... P, class F> bool fz_pick(int a, int b, int& r, F&& f) {
    return (... || (a == P::A && b == P::B ? (r = f(P{}), true) : false));
}

// 0: `kern` with `dyn` bytes of dynamic LDS fits the LDS of a CU (static + dynamic); +1: it does not
template <class K>
int fz_fits_lds(K kern, size_t dyn) {
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, (const void*)kern));
    return fa.sharedSizeBytes + dyn > FZ_LDS_BYTES ? 1 : 0;
}

// The KDE table view of a launch goes to c->d_kv (slot 0; `second`, when given, to slot 1).  Waits for the copy: the views are stack
// objects of the caller.
inline int fz_upload_kv(fz_ctx* c, const fz::KdeView& kv, const fz::KdeView* second = nullptr) {
    FZCHK(c->d_kv.ensure((second ? 2 : 1) * sizeof(fz::KdeView)));
    HIPCHK(hipMemcpyAsync(c->d_kv.p, &kv, sizeof(fz::KdeView), hipMemcpyHostToDevice, c->stream));
    if (second) HIPCHK(hipMemcpyAsync(c->d_kv.as<fz::KdeView>() + 1, second, sizeof(fz::KdeView), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// Grid of a kernel whose blocks stay resident: allows `lds` bytes of dynamic LDS, asks how many blocks of `threads` one CU holds
// (*bpc_out, at least 1) and answers min(need, that * CUs).
template <class K>
int fz_resident_blocks(fz_ctx* c, K kern, int threads, size_t lds, int64_t need, int64_t& blocks, int* bpc_out = nullptr) {
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int bpc = 1;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, (const void*)kern, threads, lds));
    bpc = std::max(1, bpc);
    if (bpc_out) *bpc_out = bpc;
    blocks = std::min<int64_t>(need, (int64_t)bpc * c->cu_count);
    return 0;
}
// ... of one that also keeps candidate lists in the workspace, those of `fit` blocks inside the budget (fz_grid.h has the rule); +1: none
template <class K>
int fz_resident_grid(fz_ctx* c, K kern, int threads, size_t lds, int64_t need, int64_t fit, int64_t& blocks) {
    int bpc = 1;
    FZCHK(fz_resident_blocks(c, kern, threads, lds, need, blocks, &bpc));
    return fz_grid_resident(need, bpc, fit, c->cu_count, blocks);
}

// One launch that reports through the device flag word: c->d_flags is cleared, `launch(int* d_flags)` queues the kernel (non-zero: its
// error), the word is read back into `flags` (waits for the stream).  What a set bit means, and the error text, is the caller's.
template <class L>
int fz_flag_roundtrip(fz_ctx* c, int& flags, L&& launch) {
    FZCHK(c->d_flags.ensure(64));
    HIPCHK(hipMemsetAsync(c->d_flags.p, 0, 64, c->stream));
    FZCHK(launch(c->d_flags.as<int>()));
    HIPCHK(hipGetLastError());
    return copy_out(c, &flags, c->d_flags.p, sizeof(int));
}

inline int fz_kde_view(fz_ctx* c, fz::KdeView& kv) {
    using namespace fz;
    if (c->label_mode == 0) return fail(-1, "labels have not been uploaded");
    if (c->label_M != c->M)
        return fail(-1, "labels (%lld) do not match the model count (%lld)", (long long)c->label_M, (long long)c->M);
    memset(&kv, 0, sizeof kv);
    kv.G = c->G;
    kv.norm = c->d_norm.as<double>();
    if (c->label_mode == 1) {
        kv.pos = c->d_pos.as<int32_t>(); kv.cls = c->d_cls.as<int32_t>();
        kv.widths = c->d_widths.as<int64_t>(); kv.offsets = c->d_offsets.as<int64_t>(); kv.kern = c->d_kern.as<double>();
        kv.w0 = c->w0; kv.koff0 = c->h_offsets[c->cls0];
        kv.kmode = c->single_cls ? KDE_HIST : KDE_DICT;
        kv.normtab = c->single_cls ? c->d_normtab.as<double>() : nullptr;
        kv.acc_stride = (int)(kv.kmode == KDE_HIST ? c->G + 2 * c->w0 : c->G);
    } else {
        kv.ly = c->d_ly.as<double>(); kv.lstd = c->d_lstd.as<double>(); kv.lo = c->d_lo.as<int32_t>(); kv.hi = c->d_hi.as<int32_t>();
        kv.grid = c->d_grid.as<double>();
        kv.gstep = fz_dbg_int("FZ_GRID_RECUR", 1) == 0 ? 0.0 : c->grid_step;
        kv.lrec = c->d_lrec.as<double>();
        kv.kmode = KDE_GRID; kv.acc_stride = (int)c->G;
    }
    kv.lane_window = (int)fz_dbg_int("FZ_LANE_WINDOW", FZ_LANE_WINDOW);
    if ((size_t)kv.acc_stride * 8 > FZ_LDS_BYTES)
        return fail(-5, "PDF grid of %lld points needs %zu B of LDS per object (> 160 KiB)", (long long)kv.G,
                    (size_t)kv.acc_stride * 8);
    return 0;
}

template <class SRC>
int fz_launch_stats(const fz_call& a, const SRC& src, int linear) {
    constexpr int TW = 4, WPB = 4;
    const int64_t per = TW * WPB;
    fz_ctx* c = a.c;
    Timer t(c, &c->tm.ms_stats, &c->tm.n_stats);
    hipLaunchKernelGGL((fz::k_stats<SRC, TW>), dim3((unsigned)((a.n + per - 1) / per)), dim3(WPB * 64), 0, c->stream, src, a.n, a.M,
                       linear, a.lmap, a.levid);
    HIPCHK(hipGetLastError());
    return 0;
}

template <class SRC, int TW>
int fz_launch_kde_tw(const fz_call& a, const SRC& src, const fz::KdeView& kv, int wpb, int linear) {
    fz_ctx* c = a.c;
    const int64_t per = (int64_t)TW * wpb;
    const size_t lds = (size_t)wpb * TW * kv.acc_stride * 8;
    auto kern = fz::k_kde<SRC, TW>;
    HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Timer t(c, &c->tm.ms_kde, &c->tm.n_kde);
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.n + per - 1) / per)), dim3(wpb * 64), lds, c->stream, src, kv, a.n, a.M, linear,
                       (const double*)a.lmap, (const double*)a.levid, a.ko->wt_thresh, a.ko->normalize, a.pdfs);
    HIPCHK(hipGetLastError());
    return 0;
}

template <class SRC>
int fz_launch_kde(const fz_call& a, const SRC& src, int linear) {
    fz::KdeView kv;
    FZCHK(fz_kde_view(a.c, kv));
    const fz_kde_geom g = fz_kde_geometry(kv.acc_stride);
    return g.tw == 2 ? fz_launch_kde_tw<SRC, 2>(a, src, kv, g.wpb, linear) : fz_launch_kde_tw<SRC, 1>(a, src, kv, g.wpb, linear);
}

// register-resident rows (fz_plane.h); +1 = not applicable
template <int NW, int E2>
int fz_launch_plane_rows_g(const fz_call& a, const double* plane, const fz::KdeView& kv) {
    fz_ctx* c = a.c;
    auto kern = fz::k_plane_rows<NW, E2>;
    constexpr size_t NT = (size_t)NW * 64;
    // exp table | three histogram rows + 1 / mass | exchange words (two parities) | flags, tie counts | label indices of the lanes'
    // columns | parked ties | the kernel taps as matrix operands
    const size_t lds = ((size_t)FZ_HEXP_K + 4 * (size_t)kv.acc_stride + 6 * NW + 2) * 8 + (2 * NW + 2) * 4 + NT * E2 * 4 + NT * 12 +
                       (size_t)fz::plane_conv_ksteps(2 * kv.w0) * 64 * 8;
    if (lds > FZ_LDS_BYTES) return 1;
    int64_t blocks = 0;
    FZCHK(fz_resident_blocks(c, kern, NW * 64, lds, a.n, blocks));
    FZCHK(fz_upload_kv(c, kv));
    Timer t(c, &c->tm.ms_fused, &c->tm.n_fused);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(NW * 64), lds, c->stream, plane, a.M, c->d_kv.as<fz::KdeView>(), kv.acc_stride, a.n,
                       (int)a.M, a.ko->wt_thresh, a.ko->normalize, a.lmap, a.levid, a.pdfs);
    HIPCHK(hipGetLastError());
#ifdef FZ_PLANE_STATS
    fz::plane_stats_print(c->stream, NW, E2);
#endif
    c->last_form = "k_plane_rows";
    return 0;
}
inline int fz_launch_plane_rows(const fz_call& a, const double* plane, const fz::KdeView& kv) {
    const fz_rows_shape s = fz_plane_rows_shape(a.M, kv.G, 2 * (int64_t)kv.w0, kv.acc_stride);
    int r = 1;
    fz_pick<fz_pair<8, 5>, fz_pair<8, 10>, fz_pair<16, 10>>(s.nw, s.e2, r, [&](auto p) { return fz_launch_plane_rows_g<decltype(p)::A, decltype(p)::B>(a, plane, kv); });
    return r;
}

// predict from a stored ln-weight plane: one pass (k_plane_fused) when its candidate lists fit the
// workspace budget, else / for linear weights / FZ_PLANE_TWOPASS=1 the two-pass kernels
inline int fz_launch_plane_predict(const fz_call& a, const double* plane, int linear) {
    using namespace fz;
    fz_ctx* c = a.c; const int64_t n = a.n, M = a.M; const fz_kde_opts* ko = a.ko;
    PlaneSrc ps; ps.p = plane; ps.ld = M;
    KdeView kv;
    FZCHK(fz_kde_view(c, kv));
    constexpr int NW = 8;          // 8 waves share one LDS copy of the log / exp tables: two blocks per CU at G = 701
    const size_t lds = ((size_t)FZ_TABS_DOUBLES + (size_t)NW * kv.acc_stride) * 8;
    const bool vec2 = (M % 2 == 0) && (((uintptr_t)plane & 15) == 0);
    const bool ho = kv.kmode == KDE_HIST;              // single-kernel label sets: the instantiation without the window code
    // the weights below wt_thresh of the best in fp32 unless the caller asked for the all-fp64 logsumexp (or thresholds nothing)
    const bool x32 = !ko->exact_evidence && !c->exact_evidence && !fz_dbg_set("FZ_EXACT_EVIDENCE") && ko->wt_thresh > 0.0;
    static constexpr decltype(&k_plane_fused<NW, 2, true, true>) kerns[8] = {           // [!x32][!vec2][!ho]
        k_plane_fused<NW, 2, true, true>,  k_plane_fused<NW, 2, false, true>,  k_plane_fused<NW, 1, true, true>,  k_plane_fused<NW, 1, false, true>,
        k_plane_fused<NW, 2, true, false>, k_plane_fused<NW, 2, false, false>, k_plane_fused<NW, 1, true, false>, k_plane_fused<NW, 1, false, false>};
    auto kern = kerns[(x32 ? 0 : 4) + (vec2 ? 0 : 2) + (ho ? 0 : 1)];
    const bool onepass = !linear && !c->force_twopass && !fz_dbg_set("FZ_PLANE_TWOPASS");
    // rows that fit one block's registers: exact maximum first, then fp64 weights straight into the LDS histogram (fz_plane.h)
    if (onepass && vec2 && ho && kv.normtab && ko->wt_thresh >= 0.0 && fz_dbg_int("FZ_PLANE_ROWS", 1) != 0) {
        const int r = fz_launch_plane_rows(a, plane, kv);
        if (r <= 0) return r;
    }
    int64_t blocks = 0;
    if (onepass && lds <= FZ_LDS_BYTES && M < ((int64_t)1 << 31)) {
        FZCHK(fz_resident_blocks(c, kern, NW * 64, lds, (n + NW - 1) / NW, blocks));
        const int64_t fit = (int64_t)(c->ws_limit / ((size_t)M * sizeof(Cand) * NW));
        if (fit < blocks) blocks = (fit >= c->cu_count) ? (fit / c->cu_count) * c->cu_count : 0;   // whole CUs or not at all
        if (blocks > 0 && c->d_cand.ensure((size_t)blocks * NW * M * sizeof(Cand)) != 0) blocks = 0;
    }
    if (blocks <= 0) {
        c->last_form = "k_stats + k_kde";
        FZCHK(fz_launch_stats(a, ps, linear));
        return fz_launch_kde(a, ps, linear);
    }
    FZCHK(fz_upload_kv(c, kv));
    Timer t(c, &c->tm.ms_fused, &c->tm.n_fused);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(NW * 64), lds, c->stream, plane, M, c->d_kv.as<KdeView>(),
                       kv.acc_stride, n, (int)M, ko->wt_thresh, ko->normalize, c->d_cand.as<Cand>(), M, a.lmap, a.levid, a.pdfs);
    HIPCHK(hipGetLastError());
    c->last_form = "k_plane_fused";
    return 0;
}

// class-sorted copy of the model records (many dictionary widths, k_fused MC): row j' <- row perm[j'], pads in place
static __global__ void k_permute_records(const double* __restrict__ in, const int* __restrict__ perm, int64_t M, int64_t Mp, int rw,
                                         double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= Mp * rw) return;
    const int64_t j = e / rw; const int r = (int)(e - j * rw);
    out[e] = in[(j < M ? (int64_t)perm[j] : j) * rw + r];
}
inline int fz_mc_records(fz_ctx* c, bool rec0) {
    bool& valid = rec0 ? c->mc_rec0_valid : c->mc_rec1_valid;
    if (valid) return 0;
    const int rw = rec0 ? fz_rec_width(2 * c->BT) : fz_rec_width(c->BT);
    DevBuf& dst = rec0 ? c->d_rec0p : c->d_rec1p;
    FZCHK(dst.ensure((size_t)c->Mp * rw * 8));
    const int64_t tot = c->Mp * rw;
    hipLaunchKernelGGL(k_permute_records, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream,
                       (rec0 ? c->d_rec0 : c->d_rec1).as<double>(), c->d_mc_perm.as<int>(), c->M, c->Mp, rw, dst.as<double>());
    HIPCHK(hipGetLastError());
    valid = true;
    return 0;
}

// The sweep over handed-back objects: the fp64 ln-space body k_fused<SWS, 1, 4, false, HOS> over exactly the objects listed behind the
// counter in c->d_redo (their chunk-level indices are the object map; the count stays on the device, so nothing waits for it), with
// candidate lists of M entries per wave in c->d_cand and its KDE view in slot 1 of c->d_kv.
// HOS: its KDE stage knows one dictionary kernel only (false: the general window stack -- many widths)
template <class SWS> struct fz_sweep_on { SWS src; fz::KdeView kv; int64_t M; };      // the sweep's own source, view and model count
template <class SWS, bool HOS>
struct fz_sweep {
    static constexpr int SW = 4;                                  // waves per block, one object each
    static constexpr size_t TDB = (size_t)SWS::template tile_doubles<SWS::template tile_len<SW>()>();
    static constexpr auto kern = fz::k_fused<SWS, 1, SW, false, HOS>;
    size_t lds = 0;
    bool ok = false;                                              // false: cannot run, the objects keep their (flagged) rows
    static size_t block_bytes(int64_t M) { return (size_t)SW * M * sizeof(fz::Cand); }      // workspace of one block
    // the PDF rows live inside the (static) tile buffers when half of the waves' rows fit in one, else in dynamic LDS
    int plan(const fz::KdeView& kv) {
        lds = ((size_t)((SW + 1) / 2) * kv.acc_stride <= TDB) ? 0 : (size_t)SW * kv.acc_stride * 8;
        const int f = fz_fits_lds(kern, lds);
        ok = f == 0;
        return f < 0 ? f : 0;
    }
    int allow_lds() const { HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); return 0; }
    void launch(const fz_call& a, const fz_sweep_on<SWS>& on, int64_t blocks) const {
        fz_ctx* c = a.c;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(SW * 64), lds, c->stream, on.src, c->d_kv.as<fz::KdeView>() + 1, on.kv.acc_stride, a.n,
                           (int)on.M, a.ko->wt_thresh, a.ko->normalize, c->d_cand.as<fz::Cand>(), on.M, a.lmap, a.levid, a.pdfs,
                           c->d_redo.as<int>() + 1, (int*)nullptr, c->d_redo.as<int>());
    }
};

// single-pass kernel; returns +1 (not an error) when its candidate workspace does
// not fit the budget and the caller should take the two-pass route
template <class SRC, int TW, int NW, bool WM>
int fz_launch_fused_wm(const fz_call& a, const SRC& src_in, const fz::KdeView& kv_in) {
    fz_ctx* c = a.c; const int64_t n = a.n, M = a.M; const fz_kde_opts* ko = a.ko;
    SRC src = src_in;
    fz::KdeView kv = kv_in;
    // many dictionary widths on the weight-space body: class-sorted records, one histogram, one convolution per class
    // present (fz_kernels.h, pdf_stage_mc); FZ_NO_MC=1 keeps the per-model window adds
    bool mc = false;
    if constexpr (WM && (NW == 12 || NW == 4)) {      // (2,16) spills inside the model loop with this PDF stage: the dispatcher sends it to (2,12)
        if (kv.kmode == fz::KDE_DICT && c->mc_ok && !fz_dbg_set("FZ_NO_MC")) {
            FZCHK(fz_mc_records(c, SRC::LMODE == 0));
            src.mv.rec0 = c->d_rec0p.as<double>(); src.mv.rec1 = c->d_rec1p.as<double>();
            kv.mc_tag = c->d_mc_tag.as<int32_t>(); kv.mc_width = c->d_mc_width.as<int32_t>(); kv.mc_off = c->d_mc_off.as<int64_t>();
            kv.mc_norm = c->d_mc_norm.as<double>(); kv.mc_gp = c->mc_gp; kv.mc_w0 = c->mc_w0;
            kv.acc_stride = c->mc_gp + 16;            // + the tail pad the sliding window of the convolution reads into
            mc = true;
        }
    }
    // the PDF rows live inside the (static) tile buffers when half of the waves' rows fit in one, else in dynamic LDS
    const size_t TDB = (size_t)SRC::template tile_doubles<SRC::template tile_len<NW>()>() +
                       ((WM && (kv.kmode == fz::KDE_HIST || mc)) ? SRC::template tile_len<NW>() / 2 : 0);       // + the index words (k_fused, POSW)
    const size_t lds = ((size_t)((NW + 1) / 2) * kv.acc_stride <= TDB) ? 0 : (size_t)NW * kv.acc_stride * 8;
    auto kern = (kv.kmode == fz::KDE_HIST) ? fz::k_fused<SRC, TW, NW, WM, true> : fz::k_fused<SRC, TW, NW, WM, false>;
    if constexpr (WM && (NW == 12 || NW == 4)) { if (mc) kern = fz::k_fused<SRC, TW, NW, WM, true, true>; }
    FZCHK(fz_fits_lds(kern, lds));
    const int64_t groups = (n + TW - 1) / TW;
    const size_t per_wave = (size_t)TW * M * sizeof(fz::Cand);
    int64_t blocks = 0;
    FZCHK(fz_resident_grid(c, kern, NW * 64, lds, (groups + NW - 1) / NW, (int64_t)(c->ws_limit / (per_wave * NW)), blocks));
    if (c->d_cand.ensure((size_t)blocks * NW * per_wave) != 0) return 1;      // no room for the lists: two-pass route
    // objects the weight-space body hands back (no candidate / no fp32 weight at all): counter + list
    if (WM) {
        FZCHK(c->d_redo.ensure(((size_t)n + 1) * sizeof(int)));
        HIPCHK(hipMemsetAsync(c->d_redo.p, 0, sizeof(int), c->stream));
    }
    // slot 0: the view of the main launch; slot 1: the caller's view (the sweep below always runs the general kernels)
    FZCHK(fz_upload_kv(c, kv, &kv_in));
    {
        Timer t(c, &c->tm.ms_fused, &c->tm.n_fused);
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(NW * 64), lds, c->stream, src, c->d_kv.as<fz::KdeView>(),
                           kv.acc_stride, n, (int)M, ko->wt_thresh, ko->normalize, c->d_cand.as<fz::Cand>(), M, a.lmap, a.levid, a.pdfs,
                           c->omap, c->d_redo.as<int>(), (const int*)nullptr);
        if constexpr (WM) {
            // the sweep, on the caller's source and view: at most one block per CU, inside the main launch's lists
            const auto sweep = [&](auto sw) -> int {
                FZCHK(sw.plan(kv_in));
                const int64_t sblocks = std::min<int64_t>(std::min<int64_t>(c->cu_count, (n + sw.SW - 1) / sw.SW),
                                                          (int64_t)((size_t)blocks * NW * per_wave / sw.block_bytes(M)));
                if (!sw.ok || sblocks < 1) return 0;
                FZCHK(sw.allow_lds());
                sw.launch(a, fz_sweep_on<SRC>{src_in, kv_in, M}, sblocks);
                return 0;
            };
            FZCHK(kv_in.kmode == fz::KDE_HIST ? sweep(fz_sweep<SRC, true>{}) : sweep(fz_sweep<SRC, false>{}));
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// the weight-space kernel body is used for the chi2^(k/2) likelihoods of the exact band counts
// (4-8 bands unmasked, dimensionality prior on) in modes A / Ai; with the free scale (mode B) it
// is used at 4 and 5 bands (5 bands: 100.0 vs 110.7 ms per 262 144 x 1e5 launch once the kernel
// no longer carried the window-scatter code; at 6 bands the ln-space body is faster, 108.9 vs
// 120.8 ms); from 7 bands up only mode Ai keeps it (register budget)
// (FZ_NO_WSPACE=1 forces the ln-space body: A/B aid)
template <class SRC>
constexpr bool fz_has_wspace() {
    return SRC::WPOW >= 1 && SRC::WPOW <= 6 && (SRC::LMODE != 2 || SRC::NB <= 5) && (SRC::NB < 7 || SRC::LMODE == 1);
}
// exact: the call asks for the exact evidence (fz_launch_fitpredict decides it), so the fp32-remainder bodies are not used
template <class SRC>
bool fz_use_wspace(const SRC& src, bool exact) {
    if constexpr (fz_has_wspace<SRC>()) return src.lp.dim_prior && !fz_dbg_set("FZ_NO_WSPACE") && !exact;
    return false;
}
template <class SRC, int TW, int NW>
int fz_launch_fused_tw(const fz_call& a, const SRC& src, const fz::KdeView& kv, bool exact) {
    if constexpr (fz_has_wspace<SRC>()) {
        if (fz_use_wspace(src, exact)) return fz_launch_fused_wm<SRC, TW, NW, true>(a, src, kv);
    }
    return fz_launch_fused_wm<SRC, TW, NW, false>(a, src, kv);
}

// share of the launch's (object, model) pairs within the weight threshold, from a sample (fz_nolist.h); < 0: not applicable.
// The sample of THIS launch is queued and read back by the NEXT one (pinned word + event), so only the first launch after a
// model upload waits for the device; consecutive chunks / steps of one data set have the same statistics.
template <class SRC>
double fz_nolist_probe(const fz_call& a, const SRC& src, const fz::KdeView& kv) {
    if constexpr (!fz_has_wspace<SRC>()) return -1.0;
    else {
        fz_ctx* c = a.c; const int64_t n = a.n, M = a.M; const fz_kde_opts* ko = a.ko;
        if (!src.lp.dim_prior || fz_dbg_set("FZ_NO_WSPACE") || kv.kmode != fz::KDE_HIST || !kv.normtab || !(ko->wt_thresh > 0.0)) return -1.0;
        const int S = 256;
        const double denom = (double)S * (double)((M + 255) / 256) * 64.0;
        if (!c->h_probe) {
            if (hipHostMalloc((void**)&c->h_probe, 8) != hipSuccess) { (void)hipGetLastError(); c->h_probe = nullptr; return -1.0; }
            if (hipEventCreateWithFlags(&c->ev_probe, hipEventDisableTiming) != hipSuccess) return -1.0;
        }
        if (c->probe_pending) {                                   // the previous launch's sample has long landed
            if (hipEventSynchronize(c->ev_probe) != hipSuccess) return -1.0;
            c->probe_share = (double)*c->h_probe / denom;
            c->probe_pending = false;
        }
        if (c->d_flags.ensure(64) != 0) return -1.0;
        if (hipMemsetAsync(c->d_flags.p, 0, 8, c->stream) != hipSuccess) return -1.0;
        hipLaunchKernelGGL((fz::k_nl_probe<SRC>), dim3(S / 4), dim3(256), 0, c->stream, src, n, (int)M, S, ko->wt_thresh, c->omap,
                           c->d_flags.as<unsigned long long>());
        if (hipMemcpyAsync(c->h_probe, c->d_flags.p, 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1.0;
        if (hipEventRecord(c->ev_probe, c->stream) != hipSuccess) return -1.0;
        c->probe_pending = true;
        if (c->probe_share < 0.0) {                               // nothing known yet: this once, wait
            if (hipEventSynchronize(c->ev_probe) != hipSuccess) return -1.0;
            c->probe_share = (double)*c->h_probe / denom;
            c->probe_pending = false;
        }
        return c->probe_share;
    }
}

// ---- k_hist: one gate, one choice of form, one name ------------------------------------------
// May a form of k_hist run here?  What all forms ask: not forced to two passes, FZ_HIST=0 (keeps k_fused) not set, a weight threshold,
// model indices that fit an int, and one dictionary kernel with its norm table -- or, where the form takes them, many widths
// (every form of k_hist forms and sums its weights in fp64: a request for the exact evidence needs no other kernel)
inline bool fz_hist_gate(const fz_call& a, const fz::KdeView& kv, bool many_widths = false) {
    if (a.c->force_twopass || fz_dbg_int("FZ_HIST", 1) == 0) return false;
    if (!(a.ko->wt_thresh > 0.0) || a.M >= ((int64_t)1 << 31)) return false;
    return many_widths || (kv.kmode == fz::KDE_HIST && kv.normtab);
}
// Direct form (true: every pair weighed in fp64 straight away) or screen form, where nothing else decides.  The classifier pays when
// it drops most pairs: with 7 % of the pairs within wt_thresh of the best (41 % above the drop bar) it runs level with the direct form
// (53.4 vs 54.9 ms per 2.6e10 pairs), with 3 % ahead of it (46.0 vs 55.2); for broader likelihoods (faint data: the reference's own
// mock sits at 41 %; bench.py --noise-scale 3 / 10: 53 % / 95 %) the direct form is the faster one.  So: by the sampled share of pairs
// within the threshold (`kv`: the view the sample is taken with); FZ_NOLIST=1 / 0 forces / forbids the switch.
template <class SRC>
bool fz_hist_broad(const fz_call& a, const SRC& src, const fz::KdeView& kv) {
    const int want = (int)fz_dbg_int("FZ_NOLIST", -1);
    if (want < 0 && a.n >= 16384) return fz_nolist_probe<SRC>(a, src, kv) > 0.12;
    return want == 1;
}
// What fz_last_form reports.  exact: the direct form because the likelihood or the caller asks for it; broad: because of the sample
inline std::string fz_hist_form(bool exact, bool broad, const char* suffix = "") {
    return std::string(exact ? "k_hist<exact>" : broad ? "k_hist<exact> (broad likelihoods)" : "k_hist<screen>") + suffix;
}

// single pass with in-kernel LDS histograms and no candidate lists (fz_hist.h); +1 = not applicable / does not fit.
// exact: every weight in fp64 (the all-fp64 evidence, and the form for broad likelihoods)
// OBJK / SWS: per-object band counts (fz_hist.h); the sweep over handed-back objects then runs on `own->src`, the MASKED variant of
// the same likelihood when objects may have unobserved bands (the mask-free arithmetic of `src` does not know N_dim per object)
// SEG (segmented model layout): `src` / `kv` / `a.M` are the segment-ordered records, their view and padded length; the sweep runs on
// the caller's own records, view and model count: `own`
// HOS: see fz_sweep
template <class SRC, int TW, int NW, bool EXACT, bool OBJK = (SRC::NB > 8), class SWS = SRC, bool SEG = false, bool HOS = true>
int fz_launch_hist_g(const fz_call& a, const SRC& src, const fz::KdeView& kv, const fz_sweep_on<SWS>* own = nullptr) {
    fz_ctx* c = a.c; const int64_t n = a.n, M = a.M; const fz_kde_opts* ko = a.ko;
    auto kern = fz::k_hist<SRC, TW, NW, EXACT, OBJK, SEG>;
    fz_sweep_on<SWS> on;
    if constexpr (std::is_same<SWS, SRC>::value) on = own ? *own : fz_sweep_on<SWS>{src, kv, M};
    else on = *own;
    const size_t lds = (size_t)NW * TW * kv.acc_stride * 8;
    FZCHK(fz_fits_lds(kern, lds));
    const int64_t groups = (n + TW - 1) / TW;
    const int64_t acap = fz_amb_cap(M, fz_dbg_set("FZ_HIST_AMBCAP"), fz_dbg_int("FZ_HIST_AMBCAP", 1));      // the ambiguous lists (fz_grid.h)
    const size_t per_wave = (size_t)TW * acap * sizeof(fz::Cand);
    int64_t blocks = 0;
    FZCHK(fz_resident_grid(c, kern, NW * 64, lds, (groups + NW - 1) / NW, (int64_t)(c->ws_limit / (per_wave * NW)), blocks));
    // the sweep (candidate lists of M entries per wave): as many blocks as stay resident and fit the workspace (with per-object
    // band counts a few per cent of a chunk can land there), at least one per CU
    fz_sweep<SWS, HOS> sw;
    FZCHK(sw.plan(on.kv));
    int bps = 1;
    if (sw.ok) {
        FZCHK(sw.allow_lds());
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bps, (const void*)sw.kern, sw.SW * 64, sw.lds));
    }
    const size_t sweep_blk = sw.block_bytes(on.M);
    bps = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(bps, 4), (int64_t)(c->ws_limit / (sweep_blk * c->cu_count))));
    const size_t sweep_ws = (size_t)bps * c->cu_count * sweep_blk;
    if (c->d_cand.ensure(std::max((size_t)blocks * NW * per_wave, sweep_ws)) != 0) return 1;
    FZCHK(c->d_redo.ensure(((size_t)n + 1) * sizeof(int)));
    HIPCHK(hipMemsetAsync(c->d_redo.p, 0, sizeof(int), c->stream));
    FZCHK(fz_upload_kv(c, kv, &on.kv));
    // the screen form without segments, more than one round: the slots are dealt in the order of their expected settle cost
    // (fz_hist_order.h), computed here from this launch's objects -- nothing is kept from call to call.  FZ_HIST_ORDER=0 deals them in
    // catalogue order as every other form does; FZ_HIST_ORDER_STRIDE / _OFFSET: the model sample (every 256th from the first).
    bool dealt = false;
    if constexpr (!EXACT && !SEG) dealt = n > blocks * NW * TW && n < ((int64_t)1 << 31) && fz_dbg_int("FZ_HIST_ORDER", 1) != 0;
    const int* order = nullptr;
    Timer t(c, &c->tm.ms_fused, &c->tm.n_fused);
    if constexpr (!EXACT && !SEG) {
        if (dealt) FZCHK((fz_hist_order_build<SRC, OBJK>(c, src, n, M, ko->wt_thresh, fz_dbg_int("FZ_HIST_ORDER_STRIDE", 256),
                                                         fz_dbg_int("FZ_HIST_ORDER_OFFSET", 0), &order)));
    }
    // (the screen form without segments reads its KDE view from the argument itself; the uploaded copies serve the segmented kernels and the sweep)
    fz::HistArgs<SRC> ha;
    ha.src = src; ha.kv = kv; ha.N = n; ha.lmap = a.lmap; ha.levid = a.levid; ha.pdfs = a.pdfs;
    ha.omap = c->omap; ha.redo = c->d_redo.as<int>(); ha.order = order; ha.normalize = ko->normalize;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(NW * 64), lds, c->stream, ha, c->d_kv.as<fz::KdeView>(), kv.acc_stride, (int)M, ko->wt_thresh,
                       c->d_cand.as<fz::Cand>(), acap);
    if (sw.ok) sw.launch(a, on, std::min<int64_t>((int64_t)bps * c->cu_count, (n + sw.SW - 1) / sw.SW));
    HIPCHK(hipGetLastError());
#ifdef FZ_HIST_WSTATS
    if constexpr (!EXACT && !OBJK && !SEG && SRC::NB <= 8 && SRC::RW <= 6) fz::hist_wstats_print(c->stream, SRC::NB, n, M, blocks, NW);
#endif
    return 0;
}
// the plain forms (no masks) or nothing (+1).  sample: the direct form also where fz_hist_broad says so
template <class SRC>
int fz_launch_hist(const fz_call& a, const SRC& src, const fz::KdeView& kv, bool sample) {
    // exact band counts without masks: 4-8 bands, and the wide sets (16, 32 bands) except 32 bands with per-model errors, whose
    // object and record (192 doubles) leave the register file no room (k_fused keeps that case)
    if constexpr (!(SRC::WPOW >= 1 && SRC::WPOW <= 30) || (SRC::NB > 16 && SRC::LMODE == 0)) return 1;
    else {
        if (!fz_hist_gate(a, kv) || !src.lp.dim_prior) return 1;
        // FZ_EXACT_EVIDENCE=1 (tests): the form that weighs every pair without classifying it first
        const bool forced = fz_dbg_int("FZ_EXACT_EVIDENCE", 0) != 0;
        const bool broad = sample && !forced && fz_hist_broad(a, src, kv);
        // the free scale (mode B) weighs every pair in fp64 straight away: its chi2 takes two passes over the bands, and screening with
        // the closed form first was slower (fz_hist.h)
        const bool ex = forced || broad || SRC::LMODE == 2;
        int r = 1;
        if constexpr (SRC::NB > 8) {
            // wide records: one object per wave, eight waves per block (up to 256 registers per lane)
            if (fz_dbg_int("FZ_HIST_WIDE", 1) == 0) return 1;      // (tests: the masked kernels of round 2)
            r = ex ? fz_launch_hist_g<SRC, 1, 8, true>(a, src, kv) : fz_launch_hist_g<SRC, 1, 8, false>(a, src, kv);
        } else {
            if (ex) r = fz_launch_hist_g<SRC, 1, 16, true>(a, src, kv);
            else if constexpr (SRC::LMODE != 2) r = fz_launch_hist_g<SRC, 1, 16, false>(a, src, kv);
        }
        if (r <= 0) a.c->last_form = fz_hist_form(forced || SRC::LMODE == 2, broad);
        return r;
    }
}

// k_hist with per-object band counts or nothing (+1): a chunk whose objects have unobserved bands, unmasked models, modes Ai / B
// (4-8 bands; the wide sets take this form anyway).  `src`: the mask-free variant, `sws`: the masked one (sweep).
template <class SRC, class SWS>
int fz_launch_hist_objmask(const fz_call& a, const SRC& src, const SWS& sws) {
    if constexpr (!(SRC::WPOW >= 1 && SRC::WPOW <= 30) || SRC::LMODE == 0) return 1;
    else {
        fz::KdeView kv;
        FZCHK(fz_kde_view(a.c, kv));
        if (!fz_hist_gate(a, kv) || fz_dbg_int("FZ_HIST_OBJMASK", 1) == 0) return 1;
        if (!src.lp.dim_prior && fz_dbg_int("FZ_HIST_NODIMPRIOR", 1) == 0) return 1;
        constexpr int NWH = SRC::NB > 8 ? 8 : 16;
        constexpr bool EX = SRC::LMODE == 2;
        const fz_sweep_on<SWS> on{sws, kv, a.M};
        const int r = fz_launch_hist_g<SRC, 1, NWH, EX, true, SWS>(a, src, kv, &on);
        if (r <= 0) a.c->last_form = fz_hist_form(EX, false, " (per-object band counts)");
        return r;
    }
}

// k_hist on the segmented model layout or nothing (+1): masked models (any mode), objects with unobserved bands against per-model
// errors.  `src`: the mask-free variant (its records are replaced by the segment-ordered copy), `sws`: the masked one (sweep over
// the handed-back objects, on the caller's own records).  FZ_HIST_SEG=0 (tests) keeps the masked kernels of k_fused.
template <class SRC, class SWS>
int fz_launch_hist_seg(const fz_call& a, const SRC& src, const SWS& sws) {
    if constexpr (!(SRC::WPOW >= 1 && SRC::WPOW <= 6) || SRC::NB > 8) return 1;
    else {
        fz_ctx* c = a.c;
        fz::KdeView kv0;
        FZCHK(fz_kde_view(c, kv0));
        // one dictionary kernel (histogram + one convolution), or many through the class-ordered segments (one convolution per class)
        const bool mcw = kv0.kmode == fz::KDE_DICT && c->mc_ok && fz_dbg_int("FZ_HIST_SEG_MC", 1) != 0;
        if (!fz_hist_gate(a, kv0, mcw) || fz_dbg_int("FZ_HIST_SEG", 1) == 0) return 1;
        // without the dimensionality prior the ln-like of mode A carries sum_b ln(xe^2 + ye^2) of the PAIR (pdf.py:96-98): not a power-0 form
        if (!src.lp.dim_prior && SRC::LMODE == 0) return 1;
        if (SRC::LMODE == 0 && c->models_big) return 1;           // (fluxes beyond 1e9: the bound on an unobserved object band's term, fz_hist.h)
        const int rs = fz_segments(c, SRC::LMODE == 0);
        if (rs != 0) return rs;
        fz::KdeView kv = kv0;
        kv.mc_tag = c->d_seg_tag.as<int32_t>(); kv.seg_mask = c->d_seg_mask.as<uint32_t>(); kv.seg_rank = c->d_seg_rank.as<int32_t>();
        kv.seg_start = c->d_seg_start.as<int32_t>(); kv.seg_n = c->seg_n; kv.seg_nrank = c->seg_nrank;
        if (mcw != (c->seg_nrank > 1)) return 1;                  // (cannot happen: both say "more than one class present")
        if (mcw) {
            kv.mc_width = c->d_mc_width.as<int32_t>(); kv.mc_off = c->d_mc_off.as<int64_t>(); kv.mc_norm = c->d_mc_rnorm.as<double>();      // (reciprocals)
            kv.mc_gp = c->mc_gp; kv.mc_w0 = c->mc_w0;
            kv.acc_stride = c->mc_gp + 16;                       // + the tail pad the sliding window of the convolution reads into
        }
        SRC s2 = src;
        s2.mv.rec0 = c->d_seg_rec0.as<double>(); s2.mv.rec1 = c->d_seg_rec1.as<double>();
        // direct form: the free scale always (fz_hist.h), FZ_EXACT_EVIDENCE=1 (tests), else by the sample, taken on the caller's own records
        // and view (its mask-free arithmetic is an estimate here, which is all the choice needs)
        const bool ex = SRC::LMODE == 2 || fz_dbg_int("FZ_EXACT_EVIDENCE", 0) != 0 || fz_hist_broad(a, src, kv0);
        fz_call as = a;
        as.M = c->seg_Ms;
        const fz_sweep_on<SWS> on{sws, kv0, a.M};
        int r = 1;
        constexpr int NWS = (SRC::LMODE == 0) ? FZ_HIST_SEG_NW0 : 16;      // waves per block (per-model errors: see FZ_HIST_SEG_NW0)
        // many widths: 12 waves per block (a histogram row of G + 2 W0 + 16 entries: 16 of them do not fit beside the tiles)
        if (mcw) {
            if (ex) r = fz_launch_hist_g<SRC, 1, 12, true, true, SWS, true, false>(as, s2, kv, &on);
            else if constexpr (SRC::LMODE != 2) r = fz_launch_hist_g<SRC, 1, 12, false, true, SWS, true, false>(as, s2, kv, &on);
        }
        else if (ex) r = fz_launch_hist_g<SRC, 1, NWS, true, true, SWS, true>(as, s2, kv, &on);
        else if constexpr (SRC::LMODE != 2) r = fz_launch_hist_g<SRC, 1, NWS, false, true, SWS, true>(as, s2, kv, &on);
        if (r <= 0) c->last_form = fz_hist_form(ex, false, mcw ? " (segmented models, many widths)" : " (segmented models)");
        return r;
    }
}

// k_hist or nothing (+1): the wide band sets (16 / 32 real bands, no masks), whose other kernels exist in the masked variants only
template <class SRC>
int fz_launch_hist_only(const fz_call& a, const SRC& src) {
    fz::KdeView kv;
    FZCHK(fz_kde_view(a.c, kv));
    return fz_launch_hist<SRC>(a, src, kv, false);
}

// fit_predict on a prepared chunk: single pass when possible, else two passes
template <class SRC>
int fz_launch_fitpredict(const fz_call& a, const SRC& src) {
    fz_ctx* c = a.c; const int64_t n = a.n;
    fz::KdeView kv;
    FZCHK(fz_kde_view(c, kv));
    if (!c->force_twopass) {
        // the default where it applies: one pass, LDS histograms, no candidate lists, every weight and sum in fp64 (fz_hist.h); FZ_HIST=0
        // keeps k_fused
        int r = fz_launch_hist<SRC>(a, src, kv, true);
        if (r <= 0) return r;
        // like_opts.exact_evidence (and FZ_EXACT_EVIDENCE=1) matters to k_fused's weight-space body only (fp32 remainder of the evidence there)
        const bool exact = fz_dbg_int("FZ_EXACT_EVIDENCE", 0) != 0 || c->exact_evidence;
        // (objects per wave, waves per block).  Few objects: one per wave so that the
        // chunk spreads over the chip.  FZ_FUSED_CFG=tw,nw overrides (tuning aid).
        if constexpr (SRC::NB > 16) {
            // wide records (17-32 bands): one object per wave keeps the kernel inside the register file
            r = fz_launch_fused_tw<SRC, 1, 4>(a, src, kv, exact);
        } else if constexpr (SRC::HAS_PRIOR) {
            // ln-prior rows are streamed from HBM beside the LDS model tiles: two geometries per body
            if (n < (int64_t)c->cu_count * 64) r = fz_launch_fused_tw<SRC, 1, 4>(a, src, kv, exact);
            else if constexpr (SRC::PREF_2x16) r = fz_launch_fused_tw<SRC, 2, 16>(a, src, kv, exact);
            else r = fz_launch_fused_tw<SRC, 4, 8>(a, src, kv, exact);
        } else {
            const bool ws = fz_use_wspace(src, exact);
            int tw = (n >= (int64_t)c->cu_count * 64) ? 4 : 1, nw = (tw == 1) ? 4 : 8;
            // measured best geometry per kernel body (profiles/README.md): up to 6 bands 16 waves x
            // 2 objects (128 VGPRs) for the weight-space body and every ln-space body except
            // unmasked mode A and masked mode B, which want the 256-VGPR budget of 8 waves x 4;
            // wider records spill at 128 VGPRs (PREF_2x16 / PREF_2x8 in PhotSrc)
            if (tw == 4 && (ws || SRC::PREF_2x16)) { tw = 2; nw = 16; }
            // weight-space body with wide records (general mode A: y and ye^2; 7 and 8 bands): 16 waves leave
            // 128 VGPRs, and the body then spills inside the model loop (3-4x slower); 12 waves (168 VGPRs) do not
            if (tw == 2 && nw == 16 && ws && (SRC::LMODE == 0 || SRC::NB >= 7)) nw = 12;
            // ... and so does the class-sorted stack of many dictionary widths (its PDF stage keeps a 12-register result row)
            if (tw == 2 && nw == 16 && ws && kv.kmode == fz::KDE_DICT && c->mc_ok && !fz_dbg_set("FZ_NO_MC")) nw = 12;
            else if (tw == 4 && SRC::PREF_2x8) { tw = 2; nw = 8; }
            if (fz_dbg_set("FZ_FUSED_CFG")) sscanf(fz_dbg_str("FZ_FUSED_CFG").c_str(), "%d,%d", &tw, &nw);
            const auto go = [&](auto p) { return fz_launch_fused_tw<SRC, decltype(p)::A, decltype(p)::B>(a, src, kv, exact); };
            if (!fz_pick<fz_pair<4, 8>, fz_pair<2, 8>, fz_pair<2, 16>, fz_pair<2, 12>, fz_pair<1, 4>>(tw, nw, r, go))      // the instantiated geometries
                return fail(-1, "FZ_FUSED_CFG=%d,%d is not an instantiated configuration", tw, nw);
        }
        if (r <= 0) { c->last_form = "k_fused"; return r; }
    }
    c->last_form = "k_stats + k_kde";
    if (c->omap) return 2;          // an object subset: only the fused kernel takes one; the caller redoes the whole chunk
    FZCHK(fz_launch_stats(a, src, 0));
    return fz_launch_kde(a, src, 0);
}
