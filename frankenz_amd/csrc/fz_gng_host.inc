// ---- networks.py ABI: training of a growing neural gas (fz_gng.h) ---------------------------------------
// Every array may live in host or device memory; host arrays are staged through the context's buffers (StageWhole, fz_stage.h).
namespace {
// the sizes of the two state arrays (include/frankenz_hip.h gives the layout; networks._gng_state_sizes is the Python twin)
int64_t gng_state_doubles(int32_t cap, int32_t B) { return 2 * (int64_t)cap * B + cap + 2 * (int64_t)B; }
int64_t gng_state_ints(int32_t cap, int32_t max_degree, int32_t prune_cap, int32_t edge_cap) {
    return GNG_NCNT + 2 * (int64_t)cap + 4 * (int64_t)cap * max_degree + 3 * (int64_t)prune_cap + edge_cap;
}
}  // namespace

extern "C" int fz_gng_train(fz_ctx* c, const double* models, const double* models_err, const double* models_mask, int64_t M, int32_t B,
                            const int64_t* draws, int64_t T, double* fstate, int32_t* istate, int64_t* ids, int32_t cap,
                            int32_t max_degree, int32_t prune_cap, int32_t edge_cap, int32_t nbatch, int32_t max_age, int32_t max_nodes,
                            int64_t nnode_init, double learn_best, double learn_neighbor, double new_err_keep, double all_err_keep,
                            const fz_like_opts* opts, int32_t track_scale, int64_t alias0, int64_t alias1, int64_t s0, int64_t s1,
                            int64_t* bmus, int32_t* batch) {
    if (!c || !models || !models_err || !models_mask || !draws || !fstate || !istate || !ids || !opts || !bmus || !batch)
        return fail(-1, "fz_gng_train: NULL argument");
    if (B <= 0 || B > 32) return fail(-5, "fz_gng_train: %d bands unsupported (1..32)", (int)B);
    if (cap < 2 || cap > FZ_GNG_MAX_NODES)
        return fail(-5, "fz_gng_train: %d node slots unsupported (2..%d: every slot is owned by one thread of ONE workgroup)", (int)cap,
                    FZ_GNG_MAX_NODES);
    if (max_degree < 2 || max_degree > 64)
        return fail(-5, "fz_gng_train: a degree limit of %d is unsupported (2..64: one lane per neighbour)", (int)max_degree);
    if (max_nodes > cap) return fail(-4, "fz_gng_train: max_nodes %d exceeds the %d node slots", (int)max_nodes, (int)cap);
    if (nbatch <= 0 || prune_cap <= 0 || edge_cap <= 0) return fail(-4, "fz_gng_train: nbatch and the list capacities must be positive");
    if (M <= 0) return fail(-4, "fz_gng_train: no models");
    if (T <= 0 || T >= ((int64_t)1 << 30)) return fail(-5, "fz_gng_train: %lld steps unsupported (1..2^30 - 1)", (long long)T);
    if (s0 < 0 || s1 > T || s0 > s1) return fail(-4, "fz_gng_train: step range [%lld, %lld) outside [0, %lld)", (long long)s0, (long long)s1, (long long)T);
    if (alias0 < -1 || alias0 >= M || alias1 < -1 || alias1 >= M) return fail(-3, "fz_gng_train: aliased row outside [-1, %lld)", (long long)M);
    if (track_scale && !opts->free_scale) return fail(-4, "fz_gng_train: track_scale needs a free scale (free_scale=True)");
    if (s0 == s1) return 0;
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {models, models_err, models_mask, draws, fstate, istate, ids, bmus, batch}));
    // host-side checks that keep every device access in bounds: the drawn rows and the counters of the state
    FZCHK(check_draws("fz_gng_train", draws, s0, s1, M));
    int32_t cnt[GNG_NCNT];
    FZCHK(host_read(cnt, istate, sizeof(cnt)));
    if (cnt[fz::GNG_NN] < 2 || cnt[fz::GNG_NN] > cap || cnt[fz::GNG_NP] < 0 || cnt[fz::GNG_NP] > prune_cap || cnt[fz::GNG_EC] < 0 ||
        cnt[fz::GNG_EC] > edge_cap || cnt[fz::GNG_STATUS] != 0 || cnt[fz::GNG_AL0] < -1 || cnt[fz::GNG_AL0] >= cap || cnt[fz::GNG_AL1] < -1 ||
        cnt[fz::GNG_AL1] >= cap || (cnt[fz::GNG_CUR] & ~1))
        return fail(-4, "fz_gng_train: the state's counters are inconsistent (nodes %d of 2..%d, prune entries %d, edges %d, status %d)",
                    cnt[fz::GNG_NN], (int)cap, cnt[fz::GNG_NP], cnt[fz::GNG_EC], cnt[fz::GNG_STATUS]);
    size_t lds_max;
    FZCHK(train_lds_max(c, &lds_max));
    const size_t fixed = 8 * (size_t)fz::gng_fixed_lds_doubles(B);
    const size_t resident = 8 * ((size_t)cap * B + cap + 2 * (((size_t)cap + 1) / 2));
    const bool lds_nodes = fixed + resident <= lds_max;
    const size_t lds = fixed + (lds_nodes ? resident : 0);
    const int64_t nb = (T - 1) / nbatch + 1;
    const size_t nf = (size_t)gng_state_doubles(cap, B) * 8, ni = (size_t)gng_state_ints(cap, max_degree, prune_cap, edge_cap) * 4;

    StageWhole st{c};
    const void *d_x, *d_xe, *d_xm, *d_dr; void *d_f, *d_i, *d_ids, *d_bmus, *d_batch;
    FZCHK(st.in(models, (size_t)M * B * 8, &d_x)); FZCHK(st.in(models_err, (size_t)M * B * 8, &d_xe));
    FZCHK(st.in(models_mask, (size_t)M * B * 8, &d_xm)); FZCHK(st.in(draws, (size_t)T * 8, &d_dr));
    FZCHK(st.inout(fstate, nf, &d_f)); FZCHK(st.inout(istate, ni, &d_i)); FZCHK(st.inout(ids, (size_t)cap * 8, &d_ids));
    FZCHK(st.inout(bmus, (size_t)T * 8, &d_bmus)); FZCHK(st.inout(batch, (size_t)nb * 2 * 4, &d_batch));   // steps outside [s0, s1) keep their values

    fz::GngArgs a;
    a.x = (const double*)d_x; a.xe = (const double*)d_xe; a.xm = (const double*)d_xm; a.draws = (const int64_t*)d_dr;
    a.fstate = (double*)d_f; a.istate = (int32_t*)d_i; a.ids = (int64_t*)d_ids; a.bmus = (int64_t*)d_bmus; a.batch = (int32_t*)d_batch;
    a.s0 = s0; a.s1 = s1; a.nnode_init = nnode_init; a.alias0 = alias0; a.alias1 = alias1;
    a.B = B; a.cap = cap; a.md = max_degree; a.pcap = prune_cap; a.ecap = edge_cap;
    a.nbatch = nbatch; a.max_age = max_age; a.max_nodes = max_nodes;
    a.learn_best = learn_best; a.learn_nbr = learn_neighbor; a.f_new = new_err_keep; a.f_all = all_err_keep;
    a.free_scale = opts->free_scale ? 1 : 0; a.dim_prior = opts->dim_prior ? 1 : 0;
    a.modec = (opts->free_scale && !opts->ignore_model_err) ? 1 : 0; a.track_scale = track_scale ? 1 : 0;
    FZCHK(lds_nodes ? train_run(c, st, fz::k_gng_train<true>, a, M, cap, lds) : train_run(c, st, fz::k_gng_train<false>, a, M, cap, lds));
    HIPCHK(hipMemcpy(cnt, d_i, sizeof(cnt), hipMemcpyDeviceToHost));
    switch (cnt[fz::GNG_STATUS]) {
        case fz::GNG_OK: return 0;
        case fz::GNG_E_DEGREE:
            return fail(-7, "fz_gng_train: step %d would give a node more than %d neighbours (the degree limit of the adjacency lists)",
                        cnt[fz::GNG_STEP], (int)max_degree);
        case fz::GNG_E_PRUNE:
            return fail(-7, "fz_gng_train: step %d overflows the prune list (%d entries)", cnt[fz::GNG_STEP], (int)prune_cap);
        case fz::GNG_E_NODES:
            return fail(-4, "fz_gng_train: at step %d the network has fewer than two connected nodes left", cnt[fz::GNG_STEP]);
        default:
            return fail(-7, "fz_gng_train: step %d ran out of edge ids (%d)", cnt[fz::GNG_STEP], (int)edge_cap);
    }
}
