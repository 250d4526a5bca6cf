// sums_host -- the host-only pieces of rmx_region_sums (rmxh::sums_max_bins, sums_lds_bytes, sum_increment, check_weights and
// check_sum_spans in remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined
// (tests/test_sums_host_cpu.py):
//   sums_host bins <S>                         prints sums_max_bins(S)
//   sums_host lds <S> <nbins>                  prints sums_lds_bytes(S, nbins)
//   sums_host increment <w> <level> <nbins>    prints sum_increment(w, level, nbins)
//   sums_host weights <nwt> <entries>          the [nwt] weights as integers, comma separated (- for a missing pointer); prints the
//                                              rule's answer: -1, -2 or the index of the first negative entry
//   sums_host spans <nq> <nwt> <entries>       the [nq][4] queries; prints the rule's answer: -1, -2 or the first query whose
//                                              weights leave the pool
// The arrays handed over hold exactly what was given: an index past them is a heap overflow.  Exit status 2 where the entries
// given do not match the extents (the rule would read past them by the caller's fault).
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

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "bins")) {
        printf("%d\n", (int)rmxh::sums_max_bins((int32_t)strtoll(argv[2], nullptr, 10)));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "lds")) {
        printf("%lld\n", (long long)rmxh::sums_lds_bytes((int32_t)strtoll(argv[2], nullptr, 10), (int32_t)strtoll(argv[3], nullptr, 10)));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "increment")) {
        printf("%d\n", (int)rmxh::sum_increment((int32_t)strtoll(argv[2], nullptr, 10), (int32_t)strtoll(argv[3], nullptr, 10), (int32_t)strtoll(argv[4], nullptr, 10)));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "weights")) {
        const long long nwt = strtoll(argv[2], nullptr, 10);
        const std::vector<int32_t> w = parse<int32_t>(argv[3]);
        if (nwt >= 0 && !w.empty() && w.size() != (size_t)nwt) return 2;
        printf("%lld\n", (long long)rmxh::check_weights(nwt, w.empty() ? nullptr : w.data()));
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "spans")) {
        const int32_t nq = (int32_t)strtoll(argv[2], nullptr, 10);
        const long long nwt = strtoll(argv[3], nullptr, 10);
        const std::vector<int32_t> q = parse<int32_t>(argv[4]);
        if (nq >= 0 && !q.empty() && q.size() != (size_t)nq * 4) return 2;
        printf("%lld\n", (long long)rmxh::check_sum_spans(nq, q.empty() ? nullptr : q.data(), nwt));
        return 0;
    }
    fprintf(stderr, "usage: sums_host bins <S> | lds <S> <nbins> | increment <w> <level> <nbins> | weights <nwt> <entries> | spans <nq> <nwt> <entries>\n");
    return 2;
}
