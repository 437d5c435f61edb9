// development only (tools/devbuild.sh): every band count except 5 answers "not compiled", so that the experimental
// library is small and quick to build.  Never part of a release build.
// One weak stub table per band count of FZ_BT_LIST: the table of a unit that IS linked (fz_inst.hip, a strong symbol) takes its place.
#include "../frankenz_amd/csrc/fz_ctx.h"
template <class... A> static int stub(A...) { return fail(-1, "dev build: 5 bands only"); }
#define FZ_STUB_BT(N) __attribute__((weak)) const fz_bt_table* fz_bt_unit_##N() { static const fz_bt_table t = {N, stub, stub, stub, stub, stub}; return &t; }
FZ_BT_LIST(FZ_STUB_BT)
