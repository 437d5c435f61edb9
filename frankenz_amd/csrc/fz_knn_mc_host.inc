// Host side of the k-NN fitter's Monte-Carlo draws (fz_knn_mc.h; docs/knn.md): fz_knn_draw_features, fz_knn_draw_trees.
// Included by frankenz_hip.hip after fz_knn_host.inc (knn_trees_shape, knn_install_trees).

namespace {
// the map's per-band constants out of the ABI struct (pdf.magnitude / pdf.luptitude of this package, value half)
int knn_mc_map_consts(const char* who, const fz_knn_map* m, int F, fz::KnnMcMap& mp) {
    if (F < 1 || F > FZ_KNN_MC_FMAX) return fail(-5, "%s: %d bands, 1..%d are supported", who, F, FZ_KNN_MC_FMAX);
    if (m->kind < FZ_KNN_MAP_IDENTITY || m->kind > FZ_KNN_MAP_LUPTITUDE) return fail(-4, "%s: feature map kind %d is not 0 (identity), 1 (magnitude) or 2 (luptitude)", who, (int)m->kind);
    for (int b = 0; b < FZ_KNN_MC_FMAX; ++b) {
        const double sky = b < F ? m->skynoise[b] : 1.0, zp = b < F ? m->zeropoints[b] : 1.0;
        if (m->kind == FZ_KNN_MAP_LUPTITUDE) { mp.a[b] = 2.0 * sky; mp.b[b] = std::log(sky / zp); }
        else { mp.a[b] = zp; mp.b[b] = 0.0; }
    }
    return 0;
}
// the error words of a call: d_mw[0] -- flags[0] zeroed, the 64-bit row word at flags + 2 all ones (the kernels take its minimum)
int knn_mc_flags_begin(fz_ctx* c, int** d_flags) {
    FZCHK(c->d_mw[0].ensure(64));
    HIPCHK(hipMemsetAsync(c->d_mw[0].p, 0, 64, c->stream));
    HIPCHK(hipMemsetAsync((char*)c->d_mw[0].p + 8, 0xFF, 8, c->stream));
    *d_flags = c->d_mw[0].as<int>();
    return 0;
}
int knn_mc_flags_check(fz_ctx* c, const char* who, const char* what, int64_t first) {
    int32_t w[4] = {0, 0, 0, 0};
    HIPCHK(hipGetLastError());
    FZCHK(copy_out(c, w, c->d_mw[0].p, sizeof w));
    if (w[0] & FZ_KNN_MC_ERR_SCALE) {
        int64_t row; memcpy(&row, w + 2, 8);
        return fail(-4, "%s: scale < 0 (or nan) in the errors of %s %lld", who, what, (long long)(first + row));
    }
    return 0;
}
template <int MAP>
void knn_mc_launch_features(fz_ctx* c, const double* x, const double* xe, int64_t n, int F, const fz::KnnMcMap& mp, uint32_t k0, uint32_t k1,
                            int64_t first, double* q, int* d_flags) {
    const int64_t nt = n * ((F + 1) >> 1);
    hipLaunchKernelGGL((fz::k_knn_mc_features<MAP>), dim3((unsigned)((nt + FZ_KNN_MC_NT - 1) / FZ_KNN_MC_NT)), dim3(FZ_KNN_MC_NT), 0, c->stream,
                       x, xe, n, F, mp, k0, k1, first, q, d_flags);
}
template <int MAP>
void knn_mc_launch_sets(fz_ctx* c, const double* y, const double* ye, int K, int64_t M, int F, const fz::KnnMcMap& mp, uint32_t k0, uint32_t k1,
                        float* out, int* d_flags) {
    const int64_t nt = M * ((F + 1) >> 1);
    hipLaunchKernelGGL((fz::k_knn_mc_sets<MAP>), dim3((unsigned)((nt + FZ_KNN_MC_NT - 1) / FZ_KNN_MC_NT), (unsigned)K), dim3(FZ_KNN_MC_NT), 0,
                       c->stream, y, ye, M, F, mp, k0, k1, out, d_flags);
}
}  // namespace

// knn.py:830-832 for N objects: q = map(x + xe z), z of (key, object first + i, band, set 0).  Rows as given (not cleaned).
extern "C" int fz_knn_draw_features(fz_ctx* c, const double* x, const double* xe, int64_t N, int32_t F, const fz_knn_map* map, uint32_t key0,
                                    uint32_t key1, int64_t first, double* q) {
    if (!c || !map) return fail(-1, "fz_knn_draw_features: NULL argument");
    fz::KnnMcMap mp;
    FZCHK(knn_mc_map_consts("fz_knn_draw_features", map, F, mp));
    if (N < 0 || first < 0) return fail(-4, "fz_knn_draw_features: %lld objects from row %lld", (long long)N, (long long)first);
    if (N == 0) return 0;
    if (!x || !xe || !q) return fail(-1, "fz_knn_draw_features: NULL argument");
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {x, xe, q}));
    const size_t row = (size_t)F * 8;
    // staging of host rows: the objects in d_pl[1] / d_pl[2], the features in d_q (where the searches stage theirs)
    const StageRows xv(c, x, row, c->d_pl[1], STAGE_IN), ev(c, xe, row, c->d_pl[2], STAGE_IN), qv(c, q, row, c->d_q, STAGE_OUT);
    int* d_flags;
    FZCHK(knn_mc_flags_begin(c, &d_flags));
    const int64_t nc = std::min<int64_t>(N, 1 << 20);
    for (int64_t i0 = 0; i0 < N; i0 += nc) {
        const int64_t n = std::min(nc, N - i0);
        const double *dx, *de; double* dq;
        FZCHK(xv.at(i0, n, &dx)); FZCHK(ev.at(i0, n, &de)); FZCHK(qv.at(i0, n, &dq));
        {
            Timer t(c, &c->tm.ms_other, &c->tm.n_other);
            // (the counter's row is first + i0 + i; the row word of the flags counts from the chunk's start)
            if (map->kind == FZ_KNN_MAP_LUPTITUDE) knn_mc_launch_features<FZ_KNN_MAP_LUPTITUDE>(c, dx, de, n, F, mp, key0, key1, first + i0, dq, d_flags);
            else if (map->kind == FZ_KNN_MAP_MAGNITUDE) knn_mc_launch_features<FZ_KNN_MAP_MAGNITUDE>(c, dx, de, n, F, mp, key0, key1, first + i0, dq, d_flags);
            else knn_mc_launch_features<FZ_KNN_MAP_IDENTITY>(c, dx, de, n, F, mp, key0, key1, first + i0, dq, d_flags);
        }
        // a chunk's bad row is reported before the next chunk is drawn: the smallest row of the call is in the first chunk that has one
        FZCHK(knn_mc_flags_check(c, "fz_knn_draw_features", "object", i0));
        FZCHK(qv.back(i0, n));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// knn.py:158-188 for the K feature sets: out[t][j] = float32(map(float32(y + ye z))), z of (key, model j, band, set 1 + t), installed as
// the resident sets exactly as fz_knn_upload_trees installs the same floats; feats_out (K,M,F) float32, host or device, or NULL.
extern "C" int fz_knn_draw_trees(fz_ctx* c, const double* models, const double* models_err, int32_t K, int64_t M, int32_t F,
                                 const fz_knn_map* map, uint32_t key0, uint32_t key1, float* feats_out) {
    if (!c || !models || !models_err || !map) return fail(-1, "fz_knn_draw_trees: NULL argument");
    FZCHK(knn_trees_shape(c, "fz_knn_draw_trees", K, M, F));
    if (K > 65535) return fail(-5, "fz_knn_draw_trees: K = %d feature sets, at most 65535", (int)K);
    fz::KnnMcMap mp;
    FZCHK(knn_mc_map_consts("fz_knn_draw_trees", map, F, mp));
    HIPCHK(hipSetDevice(c->device));
    FZCHK(wait_for_producers(c, {models, models_err, feats_out}));
    const size_t row = (size_t)F * 8, raw = (size_t)K * M * F * 4;
    // staging of host rows: the user's models (as given: the resident copies are the cleaned ones) in d_pl[1] / d_pl[2]
    const StageRows yv(c, models, row, c->d_pl[1], STAGE_IN), ev(c, models_err, row, c->d_pl[2], STAGE_IN);
    const double *dy, *de;
    FZCHK(yv.at(0, M, &dy)); FZCHK(ev.at(0, M, &de));
    FZCHK(c->d_pl[0].ensure(raw));
    int* d_flags;
    FZCHK(knn_mc_flags_begin(c, &d_flags));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        if (map->kind == FZ_KNN_MAP_LUPTITUDE) knn_mc_launch_sets<FZ_KNN_MAP_LUPTITUDE>(c, dy, de, K, M, F, mp, key0, key1, c->d_pl[0].as<float>(), d_flags);
        else if (map->kind == FZ_KNN_MAP_MAGNITUDE) knn_mc_launch_sets<FZ_KNN_MAP_MAGNITUDE>(c, dy, de, K, M, F, mp, key0, key1, c->d_pl[0].as<float>(), d_flags);
        else knn_mc_launch_sets<FZ_KNN_MAP_IDENTITY>(c, dy, de, K, M, F, mp, key0, key1, c->d_pl[0].as<float>(), d_flags);
    }
    FZCHK(knn_mc_flags_check(c, "fz_knn_draw_trees", "model", 0));
    if (feats_out) FZCHK(copy_out(c, feats_out, c->d_pl[0].p, raw));
    FZCHK(knn_install_trees(c, K, M, F));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
