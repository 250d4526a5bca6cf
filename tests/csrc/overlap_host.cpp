// overlap_host -- the host-only checks of rmx_restart_overlap (rmxh::check_pairs and check_permutations in
// remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined (tests/test_overlap_host_cpu.py):
//   overlap_host pairs <RA> <RB> <entries>       entries: integers, comma separated (- for an empty list), two per pair; prints
//                                                "ok", "bad <index of the first pair outside>" or "refused"
//   overlap_host perms <nperm> <C> <S> <entries> prints "ok", "bad <index p * C + c of the first row that is no bijection>" or
//                                                "refused" (exit status 2 if the entries are not nperm * C * S many)
//   overlap_host shift <nperm> <C> <S> <row> <at> <value>   the tables of the cyclic shifts s -> (s + row index) mod S, built here,
//                                                with entry <at> of row <row> set to <value> (row -1: unchanged)
// The arrays handed over hold exactly the entries given: an index past them is a heap overflow.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../remixt_amd/csrc/rmx_host.h"

template <typename T> static std::vector<T> parse(const char *s) {
    std::vector<T> v;
    if (!strcmp(s, "-")) return v;
    for (const char *p = s; *p;) {
        char *e;
        v.push_back((T)strtoll(p, &e, 10));
        p = *e ? e + 1 : e;
    }
    return v;
}

static void report(long long bad) {
    if (bad == -1) printf("ok\n");
    else if (bad == -2) printf("refused\n");
    else printf("bad %lld\n", bad);
}

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "pairs")) {
        const long long RA = strtoll(argv[2], nullptr, 10), RB = strtoll(argv[3], nullptr, 10);
        const std::vector<int32_t> pairs = parse<int32_t>(argv[4]);
        if (pairs.size() % 2) return 2;
        report(rmxh::check_pairs((int64_t)(pairs.size() / 2), pairs.empty() ? nullptr : pairs.data(), RA, RB));
        // pairs without a pointer describe no list
        if (!pairs.empty() && rmxh::check_pairs((int64_t)(pairs.size() / 2), nullptr, RA, RB) != -2) return 3;
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "perms")) {
        const long long nperm = strtoll(argv[2], nullptr, 10), C = strtoll(argv[3], nullptr, 10), S = strtoll(argv[4], nullptr, 10);
        const std::vector<int16_t> perms = parse<int16_t>(argv[5]);
        const bool shaped = nperm >= 0 && C >= 0 && S >= 0;
        if (shaped && (unsigned long long)nperm * C * S != perms.size()) return 2;
        report(rmxh::check_permutations(nperm, C, S, perms.empty() ? nullptr : perms.data()));
        if (shaped && !perms.empty() && rmxh::check_permutations(nperm, C, S, nullptr) != -2) return 3;
        return 0;
    }
    if (argc == 8 && !strcmp(argv[1], "shift")) {
        const long long nperm = strtoll(argv[2], nullptr, 10), C = strtoll(argv[3], nullptr, 10), S = strtoll(argv[4], nullptr, 10);
        const long long row = strtoll(argv[5], nullptr, 10), at = strtoll(argv[6], nullptr, 10), value = strtoll(argv[7], nullptr, 10);
        if (nperm < 1 || C < 1 || S < 1 || row >= nperm * C || at < 0 || at >= S) return 2;
        std::vector<int16_t> perms((size_t)(nperm * C * S));
        for (long long r = 0; r < nperm * C; r++)
            for (long long s = 0; s < S; s++) perms[(size_t)(r * S + s)] = (int16_t)((s + r) % S);
        if (row >= 0) perms[(size_t)(row * S + at)] = (int16_t)value;
        report(rmxh::check_permutations(nperm, C, S, perms.data()));
        return 0;
    }
    fprintf(stderr, "usage: overlap_host pairs <RA> <RB> <entries> | perms <nperm> <C> <S> <entries> | shift <nperm> <C> <S> <row> <at> <value>\n");
    return 2;
}
