// The pure launch arithmetic of frankenz_amd/csrc/fz_grid.h over a fixed list of inputs, one line per answer
// (tests/test_grid_host.py compiles this with the sanitizers and compares the lines with its own statement of the rules).
#include <cstdio>

#include "fz_grid.h"

int main() {
    // grid cus need bpc fit -> rc blocks
    for (int cus : {256, 8}) {
        const long long needs[] = {cus - 1, cus, cus + 1, 3LL * cus + 5};
        const long long fits[] = {0, cus / 2 - 1, cus / 2, cus - 1, cus, 2LL * cus + 1, 5LL * cus + 1};
        for (long long need : needs)
            for (long long fit : fits)
                for (int bpc : {1, 2}) {
                    int64_t blocks = -1;
                    const int rc = fz_grid_resident(need, bpc, fit, cus, blocks);
                    printf("grid %d %lld %d %lld %d %lld\n", cus, need, bpc, fit, rc, rc == 0 ? (long long)blocks : -1LL);
                }
    }
    // cap M forced value -> entries
    for (long long M : {1LL, 131072LL, 131073LL, 1048576LL, 2000000LL}) {
        printf("cap %lld 0 0 %lld\n", M, (long long)fz_amb_cap(M, false, 0));
        for (long long v : {1LL, 3LL}) printf("cap %lld 1 %lld %lld\n", M, v, (long long)fz_amb_cap(M, true, v));
    }
    // kde acc_stride -> objects per wave, waves per block (thresholds: 53 KiB / 8, 160 KiB / 4, 160 KiB / 2 bytes of 8-byte entries)
    for (int st : {1, 848, 849, 5120, 5121, 10240, 10241, 20480}) {
        const fz_kde_geom g = fz_kde_geometry(st);
        printf("kde %d %d %d\n", st, g.tw, g.wpb);
    }
    // rows M G w2 acc_stride -> waves, register pairs (0 0: refused)
    for (long long M : {4095LL, 4096LL, 5120LL, 5121LL, 8191LL, 8192LL, 10240LL, 10241LL, 16383LL, 16384LL, 20480LL, 20481LL}) {
        const fz_rows_shape s = fz_plane_rows_shape(M, 701, 100, 801);
        printf("rows %lld 701 100 801 %d %d\n", M, s.nw, s.e2);
    }
    const long long refused[][3] = {{701, 128, 829}, {701, 100, 800}, {1025, 100, 1125}, {1024, 126, 1150}, {65500, 100, 65600}};
    for (const auto& q : refused) {
        const fz_rows_shape s = fz_plane_rows_shape(5000, q[0], q[1], q[2]);
        printf("rows 5000 %lld %lld %lld %d %d\n", q[0], q[1], q[2], s.nw, s.e2);
    }
    return 0;
}
