// ---- networks.py ABI: training of a self-organizing map (fz_som.h) -------------------------------------
// Every array may live in host or device memory; host arrays are staged through the context's buffers (StageWhole, fz_stage.h).
extern "C" int fz_som_train(fz_ctx* c, const double* models, const double* models_err, const double* models_mask, int64_t M, int32_t B,
                            double* nodes, const int32_t* nodes_pos, int32_t NNODE, int32_t NPROJ, const int64_t* draws,
                            const double* learn_rate, const double* sigma, int64_t T, int32_t neighbor_kind, int32_t use_wt,
                            double wt_thresh, double cdf_thresh, const fz_like_opts* opts, int32_t track_scale, int64_t s0, int64_t s1,
                            int32_t* bmus) {
    if (!c || !models || !models_err || !models_mask || !nodes || !nodes_pos || !draws || !learn_rate || !sigma || !opts || !bmus)
        return fail(-1, "fz_som_train: NULL argument");
    if (B <= 0 || B > 32) return fail(-5, "fz_som_train: %d bands unsupported (1..32)", (int)B);
    if (NPROJ <= 0 || NPROJ > SOM_MAXPROJ) return fail(-5, "fz_som_train: %d grid dimensions unsupported (1..%d)", (int)NPROJ, SOM_MAXPROJ);
    if (NNODE <= 0 || NNODE > (1 << 22))
        return fail(-5, "fz_som_train: %d nodes unsupported (1..4194304: every node is owned by one thread of ONE workgroup)", (int)NNODE);
    if (M <= 0) return fail(-4, "fz_som_train: no models");
    if (neighbor_kind != 0 && neighbor_kind != 1) return fail(-4, "fz_som_train: unknown neighbour kind %d (0 Gaussian, 1 Lorentzian)", (int)neighbor_kind);
    if (s0 < 0 || s1 > T || s0 > s1) return fail(-4, "fz_som_train: step range [%lld, %lld) outside [0, %lld)", (long long)s0, (long long)s1, (long long)T);
    if (track_scale && !opts->free_scale) return fail(-4, "fz_som_train: track_scale needs a free scale (free_scale=True)");
    if (s0 == s1) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {models, models_err, models_mask, nodes, nodes_pos, draws, learn_rate, sigma, bmus}));
    // host-side checks that keep every device access in bounds: the drawn rows, and the squared-distance range (CDF histogram)
    FZCHK(check_draws("fz_som_train", draws, s0, s1, M));
    std::vector<int32_t> pos((size_t)NNODE * NPROJ);
    FZCHK(host_read(pos.data(), nodes_pos, pos.size() * 4));
    double dmax = 0.0;
    for (int p = 0; p < NPROJ; ++p) {
        int32_t lo = pos[p], hi = pos[p];
        for (int32_t n = 0; n < NNODE; ++n) { const int32_t v = pos[(size_t)n * NPROJ + p]; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        dmax += ((double)hi - lo) * ((double)hi - lo);
    }
    size_t lds_max;
    FZCHK(train_lds_max(c, &lds_max));
    const size_t fixed = 8 * (size_t)fz::som_fixed_lds_doubles(B);
    const size_t hist = use_wt ? 0 : 4 * ((size_t)dmax + 1);
    if (fixed + hist > lds_max)
        return fail(-5, "fz_som_train: the CDF rule keeps a histogram of the %.0f squared grid distances in LDS; at most %zu fit", dmax + 1,
                    (lds_max - fixed) / 4);
    const size_t resident = 8 * (size_t)NNODE * B + 8 * (((size_t)NNODE * NPROJ + 1) / 2);
    const bool lds_nodes = fixed + hist + resident <= lds_max;
    const size_t lds = fixed + hist + (lds_nodes ? resident : 0);

    StageWhole st{c};
    const void *d_x, *d_xe, *d_xm, *d_pos, *d_dr, *d_lr, *d_sig; void *d_nodes, *d_bmus;
    FZCHK(st.in(models, (size_t)M * B * 8, &d_x)); FZCHK(st.in(models_err, (size_t)M * B * 8, &d_xe));
    FZCHK(st.in(models_mask, (size_t)M * B * 8, &d_xm)); FZCHK(st.in(nodes_pos, pos.size() * 4, &d_pos));
    FZCHK(st.in(draws, (size_t)T * 8, &d_dr)); FZCHK(st.in(learn_rate, (size_t)T * 8, &d_lr)); FZCHK(st.in(sigma, (size_t)T * 8, &d_sig));
    FZCHK(st.inout(nodes, (size_t)NNODE * B * 8, &d_nodes));
    FZCHK(st.inout(bmus, (size_t)T * 4, &d_bmus));                                              // steps outside [s0, s1) keep their values

    fz::SomArgs a;
    a.x = (const double*)d_x; a.xe = (const double*)d_xe; a.xm = (const double*)d_xm; a.nodes = (double*)d_nodes;
    a.pos = (const int32_t*)d_pos; a.draws = (const int64_t*)d_dr; a.lr = (const double*)d_lr; a.sig = (const double*)d_sig;
    a.bmus = (int32_t*)d_bmus; a.s0 = s0; a.s1 = s1; a.nnode = NNODE; a.nproj = NPROJ; a.B = B; a.kind = neighbor_kind;
    a.use_wt = use_wt ? 1 : 0; a.wt_thresh = wt_thresh; a.cdf_thresh = cdf_thresh;
    a.free_scale = opts->free_scale ? 1 : 0; a.dim_prior = opts->dim_prior ? 1 : 0;
    a.modec = (opts->free_scale && !opts->ignore_model_err) ? 1 : 0; a.track_scale = track_scale ? 1 : 0; a.dmax = (int)dmax;
    return lds_nodes ? train_run(c, st, fz::k_som_train<true>, a, M, NNODE, lds) : train_run(c, st, fz::k_som_train<false>, a, M, NNODE, lds);
}
