// automaton_host -- the host-only pieces of rmx_region_automaton (rmxh::automaton_shape_ok, check_automata and check_symbols in
// remixt_amd/csrc/rmx_host.h) as a stand-alone program for gcc -fsanitize=address,undefined (tests/test_automaton_host_cpu.py):
//   automaton_host shape <nauto> <Q> <A>                        prints "ok" or "bad"
//   automaton_host automata <nauto> <Q> <A> <delta> <start>     delta: the [nauto][Q][A] entries, start: the [nauto] entries, as
//                                                               integers, comma separated (- for a missing pointer).  Prints
//                                                               the rule's answer: -1, -2 or the index of the first bad entry
//   automaton_host symbols <C> <nsym> <S> <A> <entries>         the [C][nsym][S] symbols; prints the rule's answer
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
    if (argc == 5 && !strcmp(argv[1], "shape")) {
        const long long nauto = strtoll(argv[2], nullptr, 10), Q = strtoll(argv[3], nullptr, 10), A = strtoll(argv[4], nullptr, 10);
        const bool want = nauto >= 1 && nauto <= 64 && Q >= 1 && Q <= 16 && A >= 1 && A <= 16;
        const bool got = rmxh::automaton_shape_ok((int32_t)nauto, (int32_t)Q, (int32_t)A);
        if (got != want) return 3;
        printf("%s\n", got ? "ok" : "bad");
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "automata")) {
        const int32_t nauto = (int32_t)strtoll(argv[2], nullptr, 10), Q = (int32_t)strtoll(argv[3], nullptr, 10), A = (int32_t)strtoll(argv[4], nullptr, 10);
        const std::vector<uint8_t> delta = parse<uint8_t>(argv[5]);
        const std::vector<int32_t> start = parse<int32_t>(argv[6]);
        if (rmxh::automaton_shape_ok(nauto, Q, A)) {
            if (!delta.empty() && delta.size() != (size_t)nauto * Q * A) return 2;
            if (!start.empty() && start.size() != (size_t)nauto) return 2;
        }
        printf("%lld\n", (long long)rmxh::check_automata(nauto, Q, A, delta.empty() ? nullptr : delta.data(), start.empty() ? nullptr : start.data()));
        return 0;
    }
    if (argc == 7 && !strcmp(argv[1], "symbols")) {
        const long long C = strtoll(argv[2], nullptr, 10), nsym = strtoll(argv[3], nullptr, 10), S = strtoll(argv[4], nullptr, 10);
        const int32_t A = (int32_t)strtoll(argv[5], nullptr, 10);
        const std::vector<int16_t> sym = parse<int16_t>(argv[6]);
        if (C >= 0 && nsym >= 0 && S >= 0 && A >= 1 && !sym.empty() && sym.size() != (size_t)(C * nsym * S)) return 2;
        printf("%lld\n", (long long)rmxh::check_symbols(C, nsym, S, A, sym.empty() ? nullptr : sym.data()));
        return 0;
    }
    fprintf(stderr, "usage: automaton_host shape <nauto> <Q> <A> | automata <nauto> <Q> <A> <delta> <start> | symbols <C> <nsym> <S> <A> <entries>\n");
    return 2;
}
