// decode_host -- the host-only pieces of rmx_region_decode (rmxh::decode_max_len_ok, check_decode_lengths and decode_plan in
// remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined (tests/test_decode_host_cpu.py):
//   decode_host check <max_len> <queries>      queries: integers, four per entry, comma separated (- for an empty list); the
//                                              array handed over holds exactly what was given: an index past it is a heap
//                                              overflow.  Prints "bad <query> <reason>" or "ok"
//   decode_host plan <nr> <nq> <S> <max_len>   prints "plan nrc qc strip_elems bp_elems states_at queries_at out_doubles", or
//                                              "refused <code>", after checking the plan's own invariants (exit status 3 if
//                                              one fails): at least one restart and one query, both budgets kept, the three
//                                              parts of the staging buffer in order and not overlapping, no overflow
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
    if (argc == 4 && !strcmp(argv[1], "check")) {
        const int32_t max_len = (int32_t)strtoll(argv[2], nullptr, 10);
        const std::vector<int32_t> queries = parse(argv[3]);
        if (queries.size() % 4) return 2;
        const char *why = "unset";
        const long long bad = rmxh::check_decode_lengths((int32_t)(queries.size() / 4), queries.data(), max_len, &why);
        if (bad >= 0) printf("bad %lld %s\n", bad, why);
        else printf("ok%s\n", why ? " with a reason" : "");
        // without a place for the reason
        if (rmxh::check_decode_lengths((int32_t)(queries.size() / 4), queries.data(), max_len, nullptr) != bad) return 3;
        if (rmxh::decode_max_len_ok(max_len) != (max_len >= 1 && max_len <= 16384)) return 3;
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "plan")) {
        const int32_t nr = (int32_t)strtoll(argv[2], nullptr, 10), nq = (int32_t)strtoll(argv[3], nullptr, 10);
        const int32_t S = (int32_t)strtoll(argv[4], nullptr, 10), max_len = (int32_t)strtoll(argv[5], nullptr, 10);
        rmxh::DecodePlan p;
        memset(&p, 0xff, sizeof p);
        const int rc = rmxh::decode_plan(nr, nq, S, max_len, &p);
        if (rmxh::decode_plan(nr, nq, S, max_len, nullptr) != 5) return 3;
        if (rc) { printf("refused %d\n", rc); return 0; }
        const unsigned long long nrc = (unsigned long long)p.nrc, qc = (unsigned long long)p.qc, L = (unsigned long long)max_len;
        bool ok = p.nrc >= 1 && p.qc >= 1 && p.nrc <= nr && p.qc <= nq && p.nrc <= 65535;
        ok = ok && p.strip_elems == L * (unsigned long long)S && p.bp_elems == nrc * qc * p.strip_elems;
        ok = ok && (p.bp_elems * 2 <= rmxh::DECODE_BP_BUDGET);
        ok = ok && p.states_at == nrc * qc && p.queries_at * 8 >= p.states_at * 8 + nrc * qc * L * 2 && p.queries_at * 8 < p.states_at * 8 + nrc * qc * L * 2 + 8;
        ok = ok && p.out_doubles == p.queries_at + 2 * qc && p.out_doubles * 8 <= rmxh::DECODE_OUT_BUDGET;
        printf("plan %d %d %zu %zu %zu %zu %zu\n", p.nrc, p.qc, p.strip_elems, p.bp_elems, p.states_at, p.queries_at, p.out_doubles);
        return ok ? 0 : 3;
    }
    fprintf(stderr, "usage: decode_host check <max_len> <queries> | decode_host plan <nr> <nq> <S> <max_len>\n");
    return 2;
}
