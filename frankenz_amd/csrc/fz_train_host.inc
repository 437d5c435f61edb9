// ---- what fz_som_train and fz_gng_train share on the host (fz_train.h; StageWhole: fz_stage.h) ----------------------------
namespace {
// the rows drawn at the steps [s0, s1) must exist: this keeps every model-row access of the kernel in bounds
int check_draws(const char* name, const int64_t* draws, int64_t s0, int64_t s1, int64_t M) {
    std::vector<int64_t> dr((size_t)(s1 - s0));
    FZCHK(host_read(dr.data(), draws + s0, dr.size() * 8));
    for (int64_t j : dr)
        if (j < 0 || j >= M) return fail(-3, "%s: drawn row %lld outside [0, %lld)", name, (long long)j, (long long)M);
    return 0;
}

int train_lds_max(fz_ctx* c, size_t* lds_max) {
    int v = 0;
    HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    *lds_max = (size_t)v;
    return 0;
}

// a.rowk: the per-row terms (k_train_rowk) in staging slot 9; slots 0..8 are the entry point's own arrays
template <class Args>
int train_rowk(fz_ctx* c, Args& a, int64_t M) {
    FZCHK(c->d_net[9].ensure((size_t)M * 4 * 8));
    double* rowk = (double*)c->d_net[9].p;
    hipLaunchKernelGGL(fz::k_train_rowk, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, a.xe, a.xm, M, a.B, a.free_scale, rowk);
    a.rowk = rowk;
    return 0;
}

// The row kernel, the ONE persistent workgroup of the trainer (a thread per node up to TRAIN_NT, in whole waves) and the staged
// outputs back to the host.  `a` is complete except for rowk.
template <class Args>
int train_run(fz_ctx* c, StageWhole& st, void (*kernel)(Args), Args& a, int64_t M, int nodes, size_t lds) {
    FZCHK(train_rowk(c, a, M));
    const int nt = nodes >= TRAIN_NT ? TRAIN_NT : ((nodes + 63) / 64) * 64;
    HIPCHK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        Timer t(c, &c->tm.ms_other, &c->tm.n_other);
        hipLaunchKernelGGL(kernel, dim3(1), dim3((unsigned)nt), lds, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    FZCHK(st.finish());
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}
}  // namespace
