// locus_host -- the host-only pieces of rmx_locus_joint (rmxh::locus_shape_ok and check_locus_lengths in
// remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined (tests/test_locus_host_cpu.py):
//   locus_host shape <nrow> <ncol> <nslot>     prints "ok" or "bad"
//   locus_host lengths <nslot> <entries>       entries: the [nq][4] queries as integers, comma separated (- for an empty list); the
//                                              array handed over holds exactly what was given: an index past it is a heap
//                                              overflow.  Prints "ok" or "bad <query>: <reason>" (exit status 2 if the entries
//                                              are no multiple of four)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../remixt_amd/csrc/rmx_host.h"

static std::vector<int32_t> parse(const char *s) {
    std::vector<int32_t> v;
    if (!strcmp(s, "-")) return v;
    for (const char *p = s; *p;) {
        char *e;
        v.push_back((int32_t)strtoll(p, &e, 10));
        p = *e ? e + 1 : e;
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "shape")) {
        const long long nrow = strtoll(argv[2], nullptr, 10), ncol = strtoll(argv[3], nullptr, 10), nslot = strtoll(argv[4], nullptr, 10);
        const bool want = nrow >= 1 && nrow <= 16 && ncol >= 1 && ncol <= 16 && nslot >= 0 && nslot <= 4096 &&
                          (nslot > 1 ? nslot : 1) * nrow * ncol <= (1ll << 20);
        const bool got = rmxh::locus_shape_ok((int32_t)nrow, (int32_t)ncol, (int32_t)nslot);
        if (got != want) return 3;
        printf("%s\n", got ? "ok" : "bad");
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "lengths")) {
        const int32_t nslot = (int32_t)strtoll(argv[2], nullptr, 10);
        const std::vector<int32_t> q = parse(argv[3]);
        if (q.size() % 4) return 2;
        const char *why = nullptr;
        const long long bad = rmxh::check_locus_lengths((int32_t)(q.size() / 4), q.empty() ? nullptr : q.data(), nslot, &why);
        if ((bad >= 0) != (why != nullptr)) return 3;
        if (bad < 0) printf("ok\n");
        else printf("bad %lld: %s\n", bad, why);
        // queries without a pointer describe no list
        if (!q.empty() && rmxh::check_locus_lengths((int32_t)(q.size() / 4), nullptr, nslot, nullptr) != 0) return 3;
        return 0;
    }
    fprintf(stderr, "usage: locus_host shape <nrow> <ncol> <nslot> | locus_host lengths <nslot> <entries>\n");
    return 2;
}
