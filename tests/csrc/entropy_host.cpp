// entropy_host -- the host-only pieces of rmx_path_entropy (rmxh::entropy_range_ok, entropy_tiles and entropy_chunk in
// remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined (tests/test_entropy_host_cpu.py):
//   entropy_host range <N> <n0> <n1>                          prints "ok" or "bad"
//   entropy_host tiles <n0> <n1> <TC> <tclass> <brk_slot>     the two tables as integers, comma separated (- for a missing
//                                                             pointer), exactly n1 entries each.  Counts first with null
//                                                             outputs, then fills buffers of exactly the counted sizes, and
//                                                             prints "<tiles> <singles>", then one line per tile "class:
//                                                             indices", then the line of the singles ("-" for none)
//   entropy_host chunk <nr> <nseg> <budget_bytes>             prints the segments per chunk
// The arrays handed over hold exactly what was given: an index past them is a heap overflow.
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
    if (argc == 5 && !strcmp(argv[1], "range")) {
        const long long N = strtoll(argv[2], nullptr, 10), n0 = strtoll(argv[3], nullptr, 10), n1 = strtoll(argv[4], nullptr, 10);
        const bool want = 0 <= n0 && n0 < n1 && n1 <= N;
        const bool got = rmxh::entropy_range_ok(N, n0, n1);
        if (got != want) return 3;
        printf("%s\n", got ? "ok" : "bad");
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "tiles")) {
        const int32_t n0 = (int32_t)strtoll(argv[2], nullptr, 10), n1 = (int32_t)strtoll(argv[3], nullptr, 10), TC = (int32_t)strtoll(argv[4], nullptr, 10);
        const std::vector<int32_t> tclass = parse<int32_t>(argv[5]), brk = parse<int32_t>(argv[6]);
        if (n1 >= 0 && ((!tclass.empty() && tclass.size() != (size_t)n1) || (!brk.empty() && brk.size() != (size_t)n1))) return 2;
        const int32_t *tp = tclass.empty() ? nullptr : tclass.data(), *bp = brk.empty() ? nullptr : brk.data();
        const rmxh::EntropyCounts cnt = rmxh::entropy_tiles(n0, n1, tp, bp, TC, nullptr, nullptr);
        printf("%lld %lld\n", (long long)cnt.tiles, (long long)cnt.singles);
        if (cnt.tiles < 0) return 0;
        std::vector<int32_t> tiles((size_t)cnt.tiles * (1 + rmxh::ENTROPY_TILE), 12345), singles((size_t)cnt.singles, 12345);
        const rmxh::EntropyCounts again = rmxh::entropy_tiles(n0, n1, tp, bp, TC, tiles.data(), singles.data());
        if (again.tiles != cnt.tiles || again.singles != cnt.singles) return 3;
        // one list alone fills the same entries
        std::vector<int32_t> tiles2(tiles.size(), 12345), singles2(singles.size(), 12345);
        rmxh::entropy_tiles(n0, n1, tp, bp, TC, tiles2.data(), nullptr);
        rmxh::entropy_tiles(n0, n1, tp, bp, TC, nullptr, singles2.data());
        if (tiles2 != tiles || singles2 != singles) return 3;
        for (int64_t t = 0; t < cnt.tiles; t++) {
            const int32_t *row = tiles.data() + t * (1 + rmxh::ENTROPY_TILE);
            printf("%d:", row[0]);
            for (int i = 0; i < rmxh::ENTROPY_TILE; i++) printf("%s%d", i ? "," : "", row[1 + i]);
            printf("\n");
        }
        if (singles.empty()) printf("-");
        for (size_t i = 0; i < singles.size(); i++) printf("%s%d", i ? "," : "", singles[i]);
        printf("\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "chunk")) {
        const long long nr = strtoll(argv[2], nullptr, 10), nseg = strtoll(argv[3], nullptr, 10), budget = strtoll(argv[4], nullptr, 10);
        const long long c = (long long)rmxh::entropy_chunk(nr, nseg, budget);
        if (c < 1) return 3;
        if (nr >= 1 && nseg >= 1 && (c > nseg || (c > 1 && (__int128)c * nr * 16 > budget))) return 3;      // inside the budget, unless one segment alone is not
        printf("%lld\n", c);
        return 0;
    }
    fprintf(stderr, "usage: entropy_host range <N> <n0> <n1> | tiles <n0> <n1> <TC> <tclass> <brk_slot> | chunk <nr> <nseg> <budget_bytes>\n");
    return 2;
}
