// extremes_host -- the host-only pieces of rmx_region_extremes (rmxh::extremes_ncol_ok and check_levels in
// remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined (tests/test_extremes_host_cpu.py):
//   extremes_host ncol <ncol>                       prints "ok" or "bad"
//   extremes_host levels <C> <nlevel> <S> <entries> entries: integers, comma separated (- for an empty list); the array handed
//                                                   over holds exactly what was given: an index past it is a heap overflow.
//                                                   Prints "ok", "bad <index of the first negative entry>" or "refused"
//                                                   (exit status 2 if the entries are not C * nlevel * S many)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../remixt_amd/csrc/rmx_host.h"

static std::vector<int16_t> parse(const char *s) {
    std::vector<int16_t> v;
    if (!strcmp(s, "-")) return v;
    for (const char *p = s; *p;) {
        char *e;
        v.push_back((int16_t)strtoll(p, &e, 10));
        p = *e ? e + 1 : e;
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "ncol")) {
        const int32_t ncol = (int32_t)strtoll(argv[2], nullptr, 10);
        if (rmxh::extremes_ncol_ok(ncol) != (ncol >= 1 && ncol <= 16)) return 3;
        printf("%s\n", rmxh::extremes_ncol_ok(ncol) ? "ok" : "bad");
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "levels")) {
        const long long C = strtoll(argv[2], nullptr, 10), nlevel = strtoll(argv[3], nullptr, 10), S = strtoll(argv[4], nullptr, 10);
        const std::vector<int16_t> levels = parse(argv[5]);
        const bool shaped = C >= 0 && nlevel >= 0 && S >= 0;
        if (shaped && (unsigned long long)C * nlevel * S != levels.size()) return 2;
        const long long bad = rmxh::check_levels(C, nlevel, S, levels.empty() ? nullptr : levels.data());
        if (bad == -1) printf("ok\n");
        else if (bad == -2) printf("refused\n");
        else printf("bad %lld\n", bad);
        // entries without a pointer describe no table
        if (shaped && !levels.empty() && rmxh::check_levels(C, nlevel, S, nullptr) != -2) return 3;
        return 0;
    }
    fprintf(stderr, "usage: extremes_host ncol <ncol> | extremes_host levels <C> <nlevel> <S> <entries>\n");
    return 2;
}
