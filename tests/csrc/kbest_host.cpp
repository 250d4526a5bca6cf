// kbest_host -- the host-only pieces of rmx_region_kbest (rmxh::kbest_k_ok and kbest_plan in remixt_amd/csrc/rmx_host.h) as a
// stand-alone program for gcc -fsanitize=address,undefined (tests/test_kbest_host_cpu.py):
//   kbest_host k <K>                              prints "ok" or "refused"
//   kbest_host plan <nr> <nq> <S> <K> <max_len>   prints "plan nrc qc strip_elems bp_elems states_at queries_at out_doubles", or
//                                                 "refused <code>", after checking the plan's own invariants (exit status 3 if
//                                                 one fails): at least one restart and one query, both budgets kept, the three
//                                                 parts of the staging buffer in order and not overlapping, no overflow
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../remixt_amd/csrc/rmx_host.h"

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "k")) {
        const int32_t K = (int32_t)strtoll(argv[2], nullptr, 10);
        if (rmxh::kbest_k_ok(K) != (K >= 1 && K <= 8)) return 3;
        printf("%s\n", rmxh::kbest_k_ok(K) ? "ok" : "refused");
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "plan")) {
        const int32_t nr = (int32_t)strtoll(argv[2], nullptr, 10), nq = (int32_t)strtoll(argv[3], nullptr, 10);
        const int32_t S = (int32_t)strtoll(argv[4], nullptr, 10), K = (int32_t)strtoll(argv[5], nullptr, 10), max_len = (int32_t)strtoll(argv[6], nullptr, 10);
        rmxh::KbestPlan p;
        memset(&p, 0xff, sizeof p);
        const int rc = rmxh::kbest_plan(nr, nq, S, K, max_len, &p);
        if (rmxh::kbest_plan(nr, nq, S, K, max_len, nullptr) != 5) return 3;
        if (rc) { printf("refused %d\n", rc); return 0; }
        const unsigned long long nrc = (unsigned long long)p.nrc, qc = (unsigned long long)p.qc, L = (unsigned long long)max_len, k = (unsigned long long)K;
        bool ok = p.nrc >= 1 && p.qc >= 1 && p.nrc <= nr && p.qc <= nq && p.nrc <= 65535;
        ok = ok && p.strip_elems == L * k * (unsigned long long)S && p.bp_elems == nrc * qc * p.strip_elems;
        ok = ok && (p.bp_elems * 2 <= rmxh::DECODE_BP_BUDGET);
        ok = ok && p.states_at == nrc * qc * k && p.queries_at * 8 >= p.states_at * 8 + nrc * qc * k * L * 2 && p.queries_at * 8 < p.states_at * 8 + nrc * qc * k * L * 2 + 8;
        ok = ok && p.out_doubles == p.queries_at + 2 * qc && p.out_doubles * 8 <= rmxh::DECODE_OUT_BUDGET;
        printf("plan %d %d %zu %zu %zu %zu %zu\n", p.nrc, p.qc, p.strip_elems, p.bp_elems, p.states_at, p.queries_at, p.out_doubles);
        return ok ? 0 : 3;
    }
    fprintf(stderr, "usage: kbest_host k <K> | kbest_host plan <nr> <nq> <S> <K> <max_len>\n");
    return 2;
}
