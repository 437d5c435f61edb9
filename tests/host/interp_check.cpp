// interp1 (frankenz_amd/csrc/fz_interp.h) on the host, over heap arrays of exactly n doubles so that a sanitizer build sees a read one
// element off either end.  tests/test_interp_host.py compiles this with -fsanitize=address,undefined, runs it and compares what it
// prints with numpy.interp.
//
// One line per evaluation:  <case> <n> <x bits> <result bits>   (bit patterns as 16 hex digits; the test rebuilds xp / fp itself
// by the same rules).  Cases, for every n in {1, 2, 5, 50}:
//   finite   xp[k] = 0.25 + 0.5 k
//   plateau  xp[k] = 0.25 + 0.5 (k - (k + 1) / 3): nodes 1 and 2, 4 and 5, ... coincide
//   tail     the finite nodes up to m = n / 2 (at least one), NaN from there on
//   allnan   every node NaN
//   nan0     NaN at node 0, finite nodes after it
// fp[k] = 1 + k^2 / 8 (strictly increasing: no two neighbours equal, so a NaN slope stays NaN as in numpy).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "fz_interp.h"

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const char* names[5] = {"finite", "plateau", "tail", "allnan", "nan0"};
    const int ns[4] = {1, 2, 5, 50};
    for (int c = 0; c < 5; ++c)
        for (int n : ns) {
            std::unique_ptr<double[]> xp(new double[n]), fp(new double[n]);       // exactly n doubles each
            for (int k = 0; k < n; ++k) {
                xp[k] = 0.25 + 0.5 * (c == 1 ? k - (k + 1) / 3 : k);
                fp[k] = 1.0 + 0.125 * k * k;
            }
            const int m = n / 2 > 1 ? n / 2 : 1;
            if (c == 2) for (int k = m; k < n; ++k) xp[k] = nan;
            if (c == 3) for (int k = 0; k < n; ++k) xp[k] = nan;
            if (c == 4) xp[0] = nan;
            // below, on and between the nodes, above the last one, NaN
            std::vector<double> xs = {-1.0, 0.0, 0.25, 0.3, 0.5, 0.75, 1.0, 1.25, 1.7, 2.25, 3.0, 12.75, 13.0, 24.75, 24.9, 1e3, nan};
            for (int k = 0; k < n; ++k)
                if (xp[k] == xp[k]) { xs.push_back(xp[k]); xs.push_back(std::nextafter(xp[k], 1e9)); xs.push_back(std::nextafter(xp[k], -1e9)); }
            const double* px = xp.get();
            const double* pf = fp.get();
            auto XP = [px](int k) { return px[k]; };
            auto FP = [pf](int k) { return pf[k]; };
            for (double x : xs) {
                const double r = fz::interp1(x, XP, FP, n);
                std::printf("%s %d %016llx %016llx\n", names[c], n, (unsigned long long)bits(x), (unsigned long long)bits(r));
            }
        }
    return 0;
}
