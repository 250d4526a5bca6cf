// conditional_host -- the host-only pieces of rmx_region_conditional (rmxh::check_conditional, conditional_q_ok and
// conditional_pairs in remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined
// (tests/test_conditional_host_cpu.py):
//   conditional_host <N> <nmask> <nlabel> <nslot> <chain ends, comma separated or -> <queries> <windows>
// queries are lists of integers, four per entry, windows two per entry, comma separated (- for an empty list).  The arrays
// handed to check_conditional hold exactly what was given: an index past them is a heap overflow.  Prints
// "bad <query> <reason>" or "ok".
//   conditional_host pairs <per> <strip>      prints conditional_pairs(per, strip)
//   conditional_host q <Q>                    prints conditional_q_ok(Q) as 0 / 1
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
    if (argc == 4 && !strcmp(argv[1], "pairs")) {
        printf("%zu\n", rmxh::conditional_pairs((size_t)strtoull(argv[2], nullptr, 10), (size_t)strtoull(argv[3], nullptr, 10)));
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "q")) {
        printf("%d\n", rmxh::conditional_q_ok(atoi(argv[2])) ? 1 : 0);
        return 0;
    }
    if (argc != 8) {
        fprintf(stderr, "usage: conditional_host <N> <nmask> <nlabel> <nslot> <chain ends> <queries> <windows>\n");
        return 2;
    }
    const int32_t N = atoi(argv[1]), nmask = atoi(argv[2]), nlabel = atoi(argv[3]), nslot = atoi(argv[4]);
    const std::vector<int32_t> ends = parse(argv[5]), queries = parse(argv[6]), windows = parse(argv[7]);
    if (queries.size() % 4 || windows.size() % 2 || queries.size() / 4 != windows.size() / 2) return 2;
    std::vector<int32_t> chain((size_t)N);
    int32_t c = 0;
    for (int32_t n = 0; n < N; n++) {
        chain[(size_t)n] = c;
        for (int32_t e : ends) if (e == n) c++;
    }
    const int32_t nq = (int32_t)(queries.size() / 4);
    const char *why = "unset";
    const long long bad = rmxh::check_conditional(nq, queries.data(), windows.data(), nslot, N, chain.data(), nmask, nlabel, &why);
    if (bad >= 0) printf("bad %lld %s\n", bad, why);
    else printf("ok%s\n", why ? " with a reason" : "");
    // without a place for the reason
    if (rmxh::check_conditional(nq, queries.data(), windows.data(), nslot, N, chain.data(), nmask, nlabel, nullptr) != bad) return 3;
    return 0;
}
