// span_host -- the host-only pieces of rmx_region_span (remixt_amd/csrc/rmx_host.h) as a stand-alone program for
// gcc -fsanitize=address,undefined (tests/test_span_host_cpu.py):
//   span_host window <wl> <wr>              "ok 0|1": the window rule with the cap of 16 384 entries
//   span_host spread <seed> <nr> <nq> <per> a seeded [nr][nq][per] table with NaN sown into some queries of some restarts, every
//                                           restart of r0 .. r0 + nr - 1 and two outside it listed: "filled <n>", then one line
//                                           per (restart, query): the number of NaN entries
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../remixt_amd/csrc/rmx_host.h"

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "window")) {
        printf("ok %d\n", rmxh::span_window_ok((int32_t)atoll(argv[2]), (int32_t)atoll(argv[3]), 16384) ? 1 : 0);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "spread")) {
        const unsigned seed = (unsigned)atoi(argv[2]);
        const int32_t nr = atoi(argv[3]), nq = atoi(argv[4]);
        const size_t per = (size_t)atoll(argv[5]);
        const int32_t r0 = 3;
        std::vector<double> out((size_t)nr * nq * per);      // (exactly the table: an index past it is a heap overflow)
        unsigned s = seed * 2654435761u + 1u;
        auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
        for (double &v : out) v = -(double)(next() % 1000) / 7.;
        for (int32_t ri = 0; ri < nr; ri++)
            for (int32_t i = 0; i < nq; i++)
                if (next() % 3 == 0) out[((size_t)ri * nq + i) * per + next() % per] = std::nan("");
        std::vector<int32_t> restarts = {r0 - 1, r0 + nr};      // (outside the call's range: skipped)
        for (int32_t ri = 0; ri < nr; ri += 2) restarts.push_back(r0 + ri);      // (every other restart was flagged)
        const long long filled = rmxh::span_spread_nan(out.data(), r0, nr, nq, per, restarts.data(), (int32_t)restarts.size());
        printf("filled %lld\n", filled);
        for (int32_t ri = 0; ri < nr; ri++)
            for (int32_t i = 0; i < nq; i++) {
                size_t n = 0;
                for (size_t e = 0; e < per; e++) n += std::isnan(out[((size_t)ri * nq + i) * per + e]);
                printf("%d %d %zu\n", ri, i, n);
            }
        printf("null %lld\n", (long long)rmxh::span_spread_nan(nullptr, r0, nr, nq, per, restarts.data(), (int32_t)restarts.size()));
        return 0;
    }
    fprintf(stderr, "usage: span_host window <wl> <wr> | spread <seed> <nr> <nq> <per>\n");
    return 2;
}
