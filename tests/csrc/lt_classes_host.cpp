// CPU sanitizer harness for rmxh::lt_classes (remixt_amd/csrc/rmx_host.h): the total-copy classes of a state table.  Built by
// tests/test_lt_classes_cpu.py with g++ -fsanitize=address,undefined -fno-sanitize-recover=all and run as a child process.
//   lt_classes_host <file>   <file>: int64 C, S, M, then the class tables cn_classes[C][S][M][2] as int64
// prints "rc <rc> NT <NT>", then per state-table class "count <n>", "ltcls <S values>", "ltrep <S values>", and last the
// answers to bad arguments "args <rc> <rc>".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../remixt_amd/csrc/rmx_host.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t head[3];
    if (fread(head, 8, 3, f) != 3) { fclose(f); return 2; }
    const int32_t C = (int32_t)head[0], S = (int32_t)head[1], M = (int32_t)head[2];
    std::vector<int64_t> cn((size_t)C * S * M * 2);
    const size_t got = fread(cn.data(), 8, cn.size(), f);
    fclose(f);
    if (got != cn.size()) return 2;
    std::vector<int32_t> ltcls, ltrep, count;
    int32_t NT = -1;
    const int rc = rmxh::lt_classes(cn.data(), C, S, M, ltcls, ltrep, count, &NT);
    printf("rc %d NT %d\n", rc, (int)NT);
    if (rc == 0) {
        if (ltcls.size() != (size_t)C * S || ltrep.size() != (size_t)C * S || count.size() != (size_t)C) return 3;
        for (int c = 0; c < C; c++) {
            printf("count %d\n", (int)count[(size_t)c]);
            printf("ltcls");
            for (int s = 0; s < S; s++) printf(" %d", (int)ltcls[(size_t)c * S + s]);
            printf("\nltrep");
            for (int s = 0; s < S; s++) printf(" %d", (int)ltrep[(size_t)c * S + s]);
            printf("\n");
        }
    }
    int32_t nt2 = 0;
    printf("args %d %d\n", rmxh::lt_classes(nullptr, C, S, M, ltcls, ltrep, count, &nt2), rmxh::lt_classes(cn.data(), C, 0, M, ltcls, ltrep, count, &nt2));
    return 0;
}
