// Per-band-count instantiations of the photometric kernels.  Compiled once per band count of FZ_BT_LIST (fz_ctx.h), as separate
// translation units so they build in parallel; each exports one table of its entry points (fz_bt_unit_<BT>, at the end).
#ifndef FZ_BT
#error "compile with -DFZ_BT=<a band count of FZ_BT_LIST, fz_ctx.h>"
#endif
#include "fz_ctx.h"
#include "fz_kernels.h"
#include "fz_launch.h"
#include "fz_modec.h"

using namespace fz;

#define FZ_BT_OR(N) || FZ_BT == N
static_assert(false FZ_BT_LIST(FZ_BT_OR), "FZ_BT is not a band count of FZ_BT_LIST (fz_ctx.h)");
#undef FZ_BT_OR

// VAR_FAST exists only when BT can equal the real band count (B in 4..8): padded band
// counts always carry mask bits.
#define FZ_EXACT_BT (FZ_BT >= 4 && FZ_BT <= 8)

// The ln-weight source of likelihood MODE in arithmetic variant VAR (PRI 1: with the chunk's additive ln-prior, 2: with its
// interpolated prior) on the models and the prepared chunk of c: the one place a PhotSrc is filled in.
template <int MODE, int VAR, int PRI = 0>
static PhotSrc<FZ_BT, MODE, VAR, PRI> phot_src(fz_ctx* c, int dim_prior) {
    PhotSrc<FZ_BT, MODE, VAR, PRI> ph;
    ph.mv = model_view(c); ph.ov = obj_view(c); ph.lp = like_params(c, MODE, dim_prior);
    if constexpr (PRI) ph.pv = c->prior;
    return ph;
}

// Run-time likelihood mode (0 A, 1 Ai, 2 B) to compile-time: f(std::integral_constant<int, MODE>{})
template <int N> using Int = std::integral_constant<int, N>;
template <class F>
static int with_mode(int mode, F&& f) {
    switch (mode) {
        case 0: return f(Int<0>{});
        case 1: return f(Int<1>{});
        case 2: return f(Int<2>{});
        default: return fail(-1, "internal: bad likelihood mode %d", mode);
    }
}
// ... and the arithmetic variant that serves `var` among the ones this unit compiles: f(Int<MODE>{}, Int<VAR>{})
template <class F>
static int with_mode_var(int mode, int var, F&& f) {
    return with_mode(mode, [&](auto MODE) -> int {
#if defined(FZ_DEV_FAST)
        // development builds (tools/devbuild.sh): the mask-free variant only, no ln-prior instantiations -- a quarter of the compile time
        if (var == VAR_FAST) return f(MODE, Int<VAR_FAST>{});
        return fail(-1, "FZ_DEV_FAST build: variant %d not compiled", var);
#elif FZ_EXACT_BT
        switch (var) {
            case VAR_FAST: return f(MODE, Int<VAR_FAST>{});
            case VAR_MASKED: return f(MODE, Int<VAR_MASKED>{});
            default: return f(MODE, Int<VAR_SAFE>{});
        }
#else
        switch (var) {
            case VAR_SAFE: return f(MODE, Int<VAR_SAFE>{});
            default: return f(MODE, Int<VAR_MASKED>{});
        }
#endif
    });
}

static int fz_planes_bt(fz_ctx* c, int mode, int var, int dim_prior, int64_t n, double* lnl, double* chi2, int64_t* ndim, double* scale,
                        double* serr) {
    const int64_t M = c->M;
    // two adjacent models per thread (16-B stores) when every plane row starts 16-B aligned
    const uintptr_t al = (uintptr_t)lnl | (uintptr_t)chi2 | (uintptr_t)ndim | (uintptr_t)scale | (uintptr_t)serr;
    const int MPT = (M % 2 == 0 && (al & 15) == 0 && fz_dbg_int("FZ_PLANES_MPT", 0) != 1) ? 2 : 1;
    const int64_t mblocks = (M + 256 * MPT - 1) / (256 * MPT);
    // objects per block: 256 when the grid still holds >= 4 blocks per CU (+11 % at 1e5 x 1e4), else 16
    const bool big = ((n + 255) / 256) * mblocks >= 4 * (int64_t)c->cu_count;
    const int TO = big ? 256 : 16;
    dim3 grid((unsigned)((n + TO - 1) / TO), (unsigned)mblocks);
    Timer t(c, &c->tm.ms_planes, &c->tm.n_planes);
    FZCHK(with_mode_var(mode, var, [&](auto MODE, auto VAR) -> int {
        auto ph = phot_src<decltype(MODE)::value, decltype(VAR)::value>(c, dim_prior);
        using PH_ = decltype(ph);
        auto kern = MPT == 2 ? (dim_prior ? (big ? k_planes<PH_, 256, 1, 2> : k_planes<PH_, 16, 1, 2>)
                                          : (big ? k_planes<PH_, 256, 0, 2> : k_planes<PH_, 16, 0, 2>))
                             : (dim_prior ? (big ? k_planes<PH_, 256, 1, 1> : k_planes<PH_, 16, 1, 1>)
                                          : (big ? k_planes<PH_, 256, 0, 1> : k_planes<PH_, 16, 0, 1>));
        hipLaunchKernelGGL(kern, grid, dim3(256), 0, c->stream, ph, n, M, lnl, chi2, ndim, scale, serr);
        return 0;
    }));
    HIPCHK(hipGetLastError());
    return 0;
}

static int fz_fitpredict_bt(fz_ctx* c, int mode, int var, int dim_prior, int64_t n, const fz_kde_opts* ko, double* lmap, double* levid,
                            double* pdfs) {
    const fz_call a{c, n, c->M, ko, lmap, levid, pdfs};
#if FZ_EXACT_BT
    if (var == VAR_SEG) {
        // masked models / unobserved object bands against per-model errors: k_hist on the segmented model layout (mask-free arithmetic,
        // the handed-back objects are swept by the masked variant); +1: not applicable, the caller takes the masked route
        const int r = with_mode(mode, [&](auto MODE) -> int {
            constexpr int MD = decltype(MODE)::value;
            return fz_launch_hist_seg(a, phot_src<MD, VAR_FAST>(c, dim_prior), phot_src<MD, VAR_MASKED>(c, dim_prior));
        });
        return r < 0 ? r : (r == 0 ? 0 : 1);
    }
#else
    if (var == VAR_SEG) return 1;
#endif
#if !defined(FZ_DEV_FAST)
    // (also: no dimensionality prior on mask-free data in modes Ai / B -- the power-0 form of the same kernel, pdf.py:94-98)
    const bool nodp_fast = !dim_prior && (var == VAR_FAST || var == VAR_PAD) && (mode == 1 || mode == 2) && !c->prior.tab;
    if (var == VAR_OBJMASK || nodp_fast) {
        // objects with unobserved bands against unmasked models, modes Ai / B: k_hist with per-object band counts on the mask-free
        // arithmetic (the handed-back objects are swept by the masked variant); +1: not applicable, the caller takes the masked route
        const int r = with_mode(mode, [&](auto MODE) -> int {
            constexpr int MD = decltype(MODE)::value;
            if constexpr (MD == 0) return 1;                     // (the form is not compiled for mode A)
            else return fz_launch_hist_objmask(a, phot_src<MD, VAR_FAST>(c, dim_prior), phot_src<MD, VAR_MASKED>(c, dim_prior));
        });
        if (var == VAR_OBJMASK) return r < 0 ? r : (r == 0 ? 0 : 1);
        if (r <= 0) return r;
    }
#else
    if (var == VAR_OBJMASK) return 1;
#endif
#if !FZ_EXACT_BT
    // 9-32 bands without a masked REAL band on tame data: the one-pass histogram kernel in its mask-free form (fz_hist.h: the pad
    // bands up to 16 / 32 are zeros, the power of chi2 follows the real band count); every other case of these band counts --
    // masks, a prior, the KDE forms k_hist does not take -- runs the masked variants
    if ((var == VAR_FAST || var == VAR_PAD) && !c->prior.tab) {
        const int r = with_mode(mode, [&](auto MODE) -> int {
            return fz_launch_hist_only(a, phot_src<decltype(MODE)::value, VAR_FAST>(c, dim_prior));
        });
        if (r <= 0) return r;
    }
#endif
    return with_mode_var(mode, var, [&](auto MODE, auto VAR) -> int {
        constexpr int MD = decltype(MODE)::value, VR = decltype(VAR)::value;
#if !defined(FZ_DEV_FAST)
        if (c->prior.tab && c->prior.frac) return fz_launch_fitpredict(a, phot_src<MD, VR, 2>(c, dim_prior));
        if (c->prior.tab) return fz_launch_fitpredict(a, phot_src<MD, VR, 1>(c, dim_prior));
#endif
        return fz_launch_fitpredict(a, phot_src<MD, VR>(c, dim_prior));
    });
}

// ---------------------------------------------------------------------------
// mode C driver on a prepared chunk: leaves converged state in c->d_mc[*]
// ---------------------------------------------------------------------------
template <int BT, bool MASKED>
static int run_modec(fz_ctx* c, int64_t n, const fz_like_opts* o, const SubsetView& sub, bool tame, bool* lnl_final) {
    const int64_t M = sub.nbr ? sub.W : c->M;
    const size_t pl = (size_t)n * M * 8;
    for (int k = 0; k < 4; ++k) FZCHK(c->d_mc[k].ensure(pl));
    FZCHK(c->d_mcerr.ensure(2 * n * 8)); FZCHK(c->d_mcfn.ensure(n * 4)); FZCHK(c->d_mcact.ensure(4 * n * 4)); FZCHK(c->d_mccnt.ensure(64));
    if (n > 0x7fffffffLL) return fail(-1, "mode C chunk too large");
    ModeCState st; st.s = c->d_mc[0].as<double>(); st.l = c->d_mc[1].as<double>(); st.c = c->d_mc[2].as<double>();
    st.sh = c->d_mc[3].as<double>(); st.err = c->d_mcerr.as<unsigned long long>(); st.errhi = st.err + n; st.firstnan = c->d_mcfn.as<int>();
    st.lnl_only = 0; st.lgtab = c->d_lgB.as<double>();
    st.qhead = nullptr; st.rfixed = (int)fz_dbg_int("FZ_MODEC_RFIXED", 0);
    FZCHK(c->d_mcniter.ensure(n * 4)); st.niter = c->d_mcniter.as<int>(); c->mc_niter_n = n;
    HIPCHK(hipMemsetAsync(st.niter, 0, n * 4, c->stream));
    // Active-object lists and their lengths live on the device and alternate between two slots; the host
    // queues FZ_MODEC_BURST iterations (step + stop rule, launched for the object count it last saw: blocks
    // of objects that stopped since exit at once) before it looks at the count again, so the loop is not
    // paced by one host round trip per iteration (a quarter of the time before).
    int* lists[2] = {c->d_mcact.as<int>(), c->d_mcact.as<int>() + n};
    int* counts = c->d_mccnt.as<int>();                  // [0], [1]: list lengths; [2]: last iteration that left objects active; [3]: ambiguous objects
    HIPCHK(hipMemsetAsync(counts, 0, 16, c->stream));
    HIPCHK(hipMemsetAsync(st.err, 0, 2 * n * 8, c->stream));
    HIPCHK(hipMemsetAsync(st.firstnan, 0, n * 4, c->stream));
    // the reciprocal-based solve for mask-free tame data (fz_modec.h); FZ_MODEC_IEEE=1 keeps the IEEE divisions throughout
    const bool fast = !MASKED && tame && !fz_dbg_set("FZ_MODEC_IEEE");
    st.amb = fast ? c->d_mcact.as<int>() + 2 * n : nullptr; st.namb = counts + 3; st.ambflag = fast ? c->d_mcact.as<int>() + 3 * n : nullptr;
    if (fast) HIPCHK(hipMemsetAsync(st.ambflag, 0, n * 4, c->stream));
    ModeC<BT, MASKED> mc; mc.mv = model_view(c); mc.ov = obj_view(c); mc.nband = c->B; mc.sub = sub;
    const int64_t tiles = (M + 255) / 256;
    if (n * tiles > 0x7fffffffLL) return fail(-1, "mode C chunk too large");
    const int max_iter = o->max_iter > 0 ? o->max_iter : 10000;
    const int burst = std::max(1, (int)fz_dbg_int("FZ_MODEC_BURST", 8));
    Timer t(c, &c->tm.ms_modec, &c->tm.n_modec);
    const bool want_lnl_only = lnl_final && *lnl_final;
    if (lnl_final) *lnl_final = false;                   // honoured below by the one-block-per-object path only (and not for neighbour subsets)
    // counters of the device, read back (waits for the stream)
    auto read_back = [&](int* dst, const int* src, int nwords) -> int {
        HIPCHK(hipMemcpyAsync(dst, src, 4 * nwords, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    };
    // the one failure of the driver (nact < 0: the one-block-per-object kernels do not say how many objects are left)
    auto not_converged = [&](int nact) -> int {
        char who[32] = "objects";
        if (nact >= 0) snprintf(who, sizeof who, "%d objects", nact);
        return fail(-7, "mode C (free_scale with model errors): %s not converged after %d iterations "
                        "(the reference loop at pdf.py:199 would not terminate)", who, max_iter);
    };
    // one run of the fixed point over `n0` objects (all of the chunk, or the listed ones), to convergence
    auto iterate = [&](const int* list0, int n0, bool fst) -> int {
        auto step = [&](const ModeCState& s2, int nobj, int init) {
            if (fst) hipLaunchKernelGGL((k_modec_step<ModeC<BT, MASKED>, true>), dim3((unsigned)(nobj * tiles)), dim3(256), 0, c->stream, mc, s2, nobj, M, init);
            else hipLaunchKernelGGL((k_modec_step<ModeC<BT, MASKED>, false>), dim3((unsigned)(nobj * tiles)), dim3(256), 0, c->stream, mc, s2, nobj, M, init);
        };
        ModeCState s2 = st;
        if (!fst) s2.amb = nullptr;
        s2.list = list0; s2.ncur = nullptr; s2.list_next = lists[0]; s2.nactive = counts; s2.last_iter = counts + 2;
        HIPCHK(hipMemsetAsync(counts, 0, 8, c->stream));
        step(s2, n0, 1);
        // iteration 0 runs on the initial set; iteration t >= 1 on list t & 1 ... written by the check of t - 1
        int it = 0, nact = n0;        // nact: an upper bound of the active count
        bool first = true;
        while (nact > 0) {
            if (it >= max_iter) return not_converged(nact);
            for (int b = 0; b < burst && it < max_iter; ++b, ++it) {
                const int cur = it & 1, nxt = cur ^ 1;
                s2.list = first ? list0 : lists[cur]; s2.ncur = first ? nullptr : counts + cur;
                s2.list_next = lists[nxt]; s2.nactive = counts + nxt;
                HIPCHK(hipMemsetAsync(counts + nxt, 0, 4, c->stream));
                step(s2, nact, 0);
                hipLaunchKernelGGL(k_modec_check, dim3((unsigned)((nact + 255) / 256)), dim3(256), 0, c->stream, s2, nact, o->ltol, it + 1);
                first = false;
            }
            FZCHK(read_back(&nact, counts + (it & 1), 1));
        }
        return 0;
    };
    // k_modec_rounds with the scales in the scale plane (see below).  Named here and not inside the generic lambda that launches it:
    // the compiler lays kernels out in the order it meets them, and this place keeps the units' machine code what it was
    using MCT = ModeC<BT, MASKED>;
    void (*rounds_wide)(MCT, ModeCState, int64_t, int, double, int, int*) = nullptr;
    if constexpr (!MASKED) rounds_wide = k_modec_rounds<MCT, 512, false>;
    // What the chunk is reported as (fz_modec_info): ambiguous objects re-run, iterations of the slowest object, path, block shape
    int64_t namb = 0, slowest = 0, kind = 2, tpb = 0;
    // One block per object, the whole fixed point inside it (fz_modec.h): no state planes through HBM.  Up to FZ_MCP_MAXM models the
    // previous scale of every model sits in LDS (k_modec_persist, k_modec_rounds); beyond, on mask-free tame data, k_modec_rounds keeps
    // the scales in the scale plane instead -- no limit on M.  FZ_MODEC_ROUNDS=0: one iteration per record read (k_modec_persist)
    // instead of several (k_modec_rounds); FZ_MODEC_PLANES: the state-plane kernels throughout.
    const bool rounds = fz_dbg_str("FZ_MODEC_ROUNDS")[0] != '0';
    const bool wide = M > FZ_MCP_MAXM;
    if (!fz_dbg_set("FZ_MODEC_PLANES") && (wide ? fast && rounds : true)) {
        if (!wide && want_lnl_only && !sub.nbr && !fz_dbg_set("FZ_MODEC_FINAL")) { st.lnl_only = o->dim_prior ? 2 : 1; *lnl_final = true; }
        // the persistent launch of every shape: as many blocks as stay resident, objects handed out through the queue head counts[4]
        auto launch = [&](auto kern, int T, size_t lds, const int* list, int64_t nobj) -> int {
            int64_t blocks = 0;
            FZCHK(fz_resident_blocks(c, kern, T, lds, nobj, blocks));
            ModeCState s2 = st; s2.last_iter = counts + 2; s2.list = list; s2.namb = counts + 3; s2.qhead = counts + 4;
            hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(T), lds, c->stream, mc, s2, nobj, (int)M, o->ltol, max_iter, counts + 1);
            return 0;
        };
        auto run = [&](auto fastc, const int* list, int64_t nobj) -> int {
            constexpr bool F = decltype(fastc)::value;
            const size_t lds = (size_t)M * 8;                    // the previous scale of every model
            if constexpr (F && !MASKED) {
                if (rounds) {
                    kind = 3;
                    HIPCHK(hipMemsetAsync(counts + 4, 0, 4, c->stream));
                    if (wide) { tpb = 512; return launch(rounds_wide, 512, 0, list, nobj); }
                    if (M <= 1024) { tpb = 256; return launch(k_modec_rounds<MCT, 256, true>, 256, lds, list, nobj); }
                    if (M <= 4096) { tpb = 512; return launch(k_modec_rounds<MCT, 512, true>, 512, lds, list, nobj); }
                    tpb = 1024;
                    return launch(k_modec_rounds<MCT, 1024, true>, 1024, lds, list, nobj);
                }
            }
            kind = 1;
            if (M <= 1024) { tpb = 1024; return launch(k_modec_persist<MCT, F, 1024, 1>, 1024, lds, list, nobj); }
            if (M <= 4096) { tpb = 1024; return launch(k_modec_persist<MCT, F, 1024, 4>, 1024, lds, list, nobj); }
            if (M <= 768 * 14) { tpb = 768; return launch(k_modec_persist<MCT, F, 768, 14>, 768, lds, list, nobj); }
            tpb = 512;
            return launch(k_modec_persist<MCT, F, 512, 32>, 512, lds, list, nobj);
        };
        if (fast) FZCHK(run(std::true_type{}, nullptr, n)); else FZCHK(run(std::false_type{}, nullptr, n));
        const int64_t kind0 = kind, tpb0 = tpb;                  // (the re-run below is not what the call is reported as)
        int res[3] = {0, 0, 0};                              // status, slowest object's iterations, ambiguous objects
        FZCHK(read_back(res, counts + 1, 3));
        if (fast && res[2] > 0 && !res[0]) {
            // objects whose error came within rounding of ltol: once more from the start, IEEE divisions
            if (wide) {
                // ... by the state-plane kernels (their state planes are simply overwritten)
                HIPCHK(hipMemsetAsync(st.err, 0, n * 8, c->stream));
                HIPCHK(hipMemsetAsync(counts + 2, 0, 4, c->stream));
                FZCHK(iterate(st.amb, res[2], false));
                int it2 = 0;
                FZCHK(read_back(&it2, counts + 2, 1));
                res[1] = std::max(res[1], it2 + 1);
            } else {
                FZCHK(run(std::false_type{}, st.amb, res[2]));
                FZCHK(read_back(res, counts + 1, 2));        // (status and slowest object; the ambiguous count stays the first run's)
            }
        }
        if (res[0]) return not_converged(-1);
        namb = fast ? res[2] : 0; slowest = res[1]; kind = kind0; tpb = tpb0;
    } else {
        // state planes (k_modec_step / k_modec_check)
        FZCHK(iterate(nullptr, (int)n, fast));
        int na = 0, it_max = 0;
        if (fast) {
            FZCHK(read_back(&na, counts + 3, 1));
            if (na > 0) {
                // objects whose error came within rounding of ltol: once more from the start, IEEE divisions (their state planes are
                // simply overwritten; the list lives behind the two active lists)
                HIPCHK(hipMemsetAsync(st.err, 0, n * 8, c->stream));
                FZCHK(iterate(st.amb, na, false));
            }
        }
        FZCHK(read_back(&it_max, counts + 2, 1));            // iterations the slowest object took, minus one
        namb = na; slowest = it_max + 1;
    }
    HIPCHK(hipGetLastError());
    c->mc_info[0] += namb; c->mc_info[1] = std::max<int64_t>(c->mc_info[1], slowest); c->mc_info[2] = kind; c->mc_info[3] = tpb;
    // iterations of the slowest object of the chunk (the timed scopes add the counts bench.py subtracts: +1 per scope, the initial pass)
    c->tm.n_modec += slowest;
    return 0;
}

static int fz_modec_bt(fz_ctx* c, int var, int64_t n, const fz_like_opts* o, const int64_t* nbr, const int64_t* nnb, int W, bool* lnl_final) {
    SubsetView sub; sub.nbr = nbr; sub.nnb = nnb; sub.W = W;
#if FZ_EXACT_BT
    return var == VAR_FAST ? run_modec<FZ_BT, false>(c, n, o, sub, true, lnl_final) : run_modec<FZ_BT, true>(c, n, o, sub, false, lnl_final);
#else
    (void)var;
    return run_modec<FZ_BT, true>(c, n, o, sub, false, lnl_final);
#endif
}

// ---------------------------------------------------------------------------
// k-NN: brute-force search over the K feature sets and the subset likelihood/PDF
// ---------------------------------------------------------------------------
static int fz_knnquery_bt(fz_ctx* c, const double* q, int64_t n, int k, double bound2, int64_t* idx, int pnorm) {
    constexpr int TQ = (FZ_BT <= 5) ? 4 : (FZ_BT <= 8 ? 2 : 1);     // queries per wave (register budget)
    const bool screen = pnorm == 2 && !fz_dbg_set("FZ_KNN_FP64");
    const int64_t per = (int64_t)(screen ? (TQ >= 2 ? TQ : 2) : TQ) * 4;
    dim3 grid((unsigned)((n + per - 1) / per), (unsigned)c->knn_K);
    Timer t(c, &c->tm.ms_knn, &c->tm.n_knn);
    if (screen) {
        // Euclidean norm: packed-fp32 screen + exact fp64 re-check (same result, ~2x fewer fp64 instructions)
        constexpr int TQ2 = TQ >= 2 ? TQ : 2;                          // screened in pairs (8 per wave measured slower: registers)
        hipLaunchKernelGGL((k_knn_query32<FZ_BT, TQ2>), grid, dim3(256), 0, c->stream, c->d_trees.as<float>(), c->Mp, (int)c->knn_M, q, n,
                           c->knn_F, k, bound2, idx, c->knn_K);
    } else {
        hipLaunchKernelGGL((k_knn_query<FZ_BT, TQ>), grid, dim3(256), 0, c->stream, c->d_trees.as<float>(), c->Mp, (int)c->knn_M, q, n,
                           c->knn_F, k, bound2, idx, c->knn_K, pnorm);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

static int fz_knnsubset_bt(fz_ctx* c, int mode, int var, int dim_prior, int64_t n, const int64_t* idx, int W, const fz_kde_opts* ko,
                           const KnnOut* out, int* errflag) {
    KdeView kv;
    memset(&kv, 0, sizeof kv);
    if (out->pdfs) FZCHK(fz_kde_view(c, kv));
    else kv.acc_stride = 8;
    FZCHK(fz_upload_kv(c, kv));
    const size_t per_wave = fz_knn_subset_lds_doubles(kv.acc_stride, W);      // list | hash table, then ln-likelihoods + accumulation row (fz_knn.h)
    int wpb = 4;
    while (wpb > 1 && per_wave * 8 * wpb > 53 * 1024) wpb >>= 1;             // (three blocks per CU)
    const size_t lds = per_wave * 8 * wpb;
    if (lds > FZ_LDS_BYTES) return fail(-5, "k-NN PDF grid too large for LDS");
    Timer t(c, &c->tm.ms_knn, &c->tm.n_knn);
    FZCHK(with_mode_var(mode, var, [&](auto MODE, auto VAR) -> int {
        auto ph = phot_src<decltype(MODE)::value, decltype(VAR)::value>(c, dim_prior);
        auto kern = k_knn_subset<decltype(ph)>;
        HIPCHK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)((n + wpb - 1) / wpb)), dim3(wpb * 64), lds, c->stream, ph,
                           c->d_kv.as<KdeView>(), kv.acc_stride, n, (int)c->M, idx, W, mode == 2 ? 1 : 0, ko->wt_thresh,
                           ko->normalize, *out, errflag);
        return 0;
    }));
    HIPCHK(hipGetLastError());
    return 0;
}

// what this unit exports (fz_ctx.h)
#define FZ_CAT_(a, b) a##b
#define FZ_CAT(a, b) FZ_CAT_(a, b)
const fz_bt_table* FZ_CAT(fz_bt_unit_, FZ_BT)() {
    static const fz_bt_table t = {FZ_BT, fz_planes_bt, fz_fitpredict_bt, fz_modec_bt, fz_knnsubset_bt, fz_knnquery_bt};
    return &t;
}
