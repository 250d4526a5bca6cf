// rmx_host.h -- the pieces of the C ABI that never touch the device, as plain C++ (no HIP types), so that the CPU test
// suite can compile them with gcc -fsanitize=address,undefined (tests/csrc/host_sanitize.cpp, tests/test_sanitizers_cpu.py):
//   compress_cn_states   rmx_compress_cn_states: dense (N,S,M,2) int64 state array -> class tables + class id per segment
//   lt_classes           the total-copy classes of the state tables (compact read-depth planes of the cell cache)
//   span_window_ok, span_spread_nan  rmx_region_span: the window rule of a table, and NaN in every entry of a failed query
//   check_patterns       rmx_region_pattern: the rules of the piece lists of its queries
//   check_conditional, conditional_q_ok, conditional_pairs  rmx_region_conditional: the run and window rules, and the chunks of a call
//   decode_max_len_ok, check_decode_lengths, decode_plan  rmx_region_decode: the length rules and the chunks of a call
//   kbest_k_ok, kbest_plan                                rmx_region_kbest: the rank rule and the chunks of a call
//   extremes_ncol_ok, check_levels  rmx_region_extremes: the column rule, and that no level entry is negative
//   locus_shape_ok, check_locus_lengths  rmx_locus_joint: the table and slot rule, and that a profile query fits its slots
//   automaton_shape_ok, check_automata, check_symbols  rmx_region_automaton: the shape rule, and that every transition, start state and symbol is in range
//   sums_max_bins, sums_lds_bytes, sum_increment, check_weights, check_sum_spans  rmx_region_sums: the bins the LDS plan holds, the saturating increment, the weight pool's rules
//   entropy_range_ok, entropy_tiles, entropy_chunk  rmx_path_entropy: the range rule, the work lists of a range and the chunks of a call
//   check_pairs, check_permutations  rmx_restart_overlap: the restart pairs lie inside the two batches, every permutation row is a bijection
//   weighted_search      rmx_weighted_search: numpy's cumsum / searchsorted(side='right') for the weighted M-step samples
//                        (reference remixt/cn_model.py:475-480)
//   weighted_sample_round  rmx_weighted_sample_round: a whole round of that sampling from a strided weight column
//   Nm1                  scipy.optimize.fmin (Nelder-Mead, one variable) as a resumable state machine: the polish stage
//                        of scipy.optimize.brute in BreakpointModel.update_param (reference remixt/cn_model.py:553-561)
// Status codes: 0 ok, 4 = RMX_EUNSUPPORTED, 5 = RMX_EARG (include/remixt_amd.h).
#ifndef RMX_HOST_H
#define RMX_HOST_H
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

// (Nm1 also runs inside a kernel: k_param_search_nm)
#if defined(__HIPCC__)
#define RMX_HD __host__ __device__
#else
#define RMX_HD
#endif

namespace rmxh {

// rmx_region_span's window rule: wl, wr >= 0 and a table of (wl + 1) (wr + 1) <= max_entries entries (no overflow for any int32 pair)
inline bool span_window_ok(int32_t wl, int32_t wr, int64_t max_entries) {
    return wl >= 0 && wr >= 0 && ((int64_t)wl + 1) * ((int64_t)wr + 1) <= max_entries;
}
// rmx_region_span after a failed call: out is [nr][nq][per]; in every restart of `restarts` (absolute indices; the ones outside
// [r0, r0 + nr) are skipped) a query with a NaN in any entry becomes NaN in every entry -- a workgroup that fails leaves NaN in the
// columns of its own group only.  Returns the number of queries it filled.
inline int64_t span_spread_nan(double *out, int32_t r0, int32_t nr, int32_t nq, size_t per, const int32_t *restarts, int32_t nrestarts) {
    int64_t filled = 0;
    if (!out || !restarts) return filled;
    for (int32_t k = 0; k < nrestarts; k++) {
        const int64_t ri = (int64_t)restarts[k] - r0;
        if (ri < 0 || ri >= nr) continue;
        for (int32_t i = 0; i < nq; i++) {
            double *t = out + ((size_t)ri * nq + i) * per;
            bool bad = false;
            for (size_t e = 0; e < per && !bad; e++) bad = std::isnan(t[e]);
            if (bad) { std::fill(t, t + per, std::nan("")); filled++; }
        }
    }
    return filled;
}

// rmx_region_pattern's rules for its queries [nq][4] = (first piece p0, piece count np, 0, 0) over pieces [npieces][4] =
// (a, b, mask index or -1, label index or -1): np >= 1, p0 .. p0 + np - 1 inside the array, fields 2 and 3 zero; every piece of
// the query with 0 <= a <= b < N and table indices in [-1, nmask) / [-1, nlabel); the pieces ascending and disjoint
// (b_j < a_j+1; touching is allowed) and all in one chain (chain[n]: the chain of segment n, [N]).  Only pieces a query
// names are looked at; queries may share pieces.  Returns the index of the first query that breaks a rule, with *reason
// (a string literal), or -1.
inline int64_t check_patterns(int32_t nq, const int32_t *queries, int32_t npieces, const int32_t *pieces, int32_t N, const int32_t *chain,
                              int32_t nmask, int32_t nlabel, const char **reason) {
    const char *why = nullptr;
    int64_t bad = -1;
    if (nq < 0 || npieces < 0 || N < 0 || (nq > 0 && !queries) || (npieces > 0 && !pieces) || (N > 0 && !chain)) { why = "bad arguments"; bad = 0; }
    for (int32_t i = 0; i < nq && !why; i++) {
        const int32_t *qq = queries + 4 * (size_t)i;
        const int64_t p0 = qq[0], np = qq[1];
        if (np < 1) why = "a query needs at least one piece";
        else if (p0 < 0 || p0 + np > (int64_t)npieces) why = "a query's pieces lie outside the piece array";
        else if (qq[2] != 0 || qq[3] != 0) why = "the third and fourth fields of a query must be 0";
        for (int64_t k = 0; k < np && !why; k++) {
            const int32_t *pp = pieces + 4 * (size_t)(p0 + k);
            if (pp[0] < 0 || pp[1] >= N || pp[0] > pp[1]) why = "a piece needs 0 <= first <= last < num_segments";
            else if (pp[2] < -1 || pp[2] >= nmask) why = "mask index out of range";
            else if (pp[3] < -1 || pp[3] >= nlabel) why = "label index out of range";
            else if (k > 0 && pp[-3] >= pp[0]) why = "the pieces of a query must be ascending and disjoint";
            else if (chain[pp[0]] != chain[pp[1]] || (k > 0 && chain[pp[-4]] != chain[pp[0]])) why = "the pieces of a query must lie in one chain";
        }
        if (why) bad = i;
    }
    if (reason) *reason = why;
    return bad;
}

// rmx_region_conditional.  Its queries [nq][4] = (a, b, mask index or -1, label index or -1) are evidence runs, its windows
// [nq][2] = (lo, hi) the segments whose conditional marginals come back, nslot slots per query.  The rules: 1 <= nslot <=
// COND_MAX_SLOTS; 0 <= lo <= a <= b <= hi < N, lo and hi in one chain (chain[n]: the chain of segment n, [N]; a and b lie between
// them); hi - lo + 1 <= nslot; b - a + 1 <= COND_MAX_RUN; table indices in [-1, nmask) / [-1, nlabel).  Returns the index of the
// first query that breaks a rule, with *reason (a string literal), or -1.
constexpr int32_t COND_MAX_SLOTS = 16384;
constexpr int32_t COND_MAX_RUN = 4096;
constexpr int32_t COND_MAX_Q = 64;
constexpr size_t COND_OUT_BUDGET = (size_t)64 << 20;       // outputs and queries of a chunk, bytes
constexpr size_t COND_WS_BUDGET = (size_t)256 << 20;       // U rows of a chunk, bytes
inline bool conditional_q_ok(int32_t Q) { return Q >= 1 && Q <= COND_MAX_Q; }
inline int64_t check_conditional(int32_t nq, const int32_t *queries, const int32_t *windows, int32_t nslot, int32_t N, const int32_t *chain,
                                 int32_t nmask, int32_t nlabel, const char **reason) {
    const char *why = nullptr;
    int64_t bad = -1;
    if (nq < 0 || N < 0 || (nq > 0 && (!queries || !windows)) || (N > 0 && !chain)) { why = "bad arguments"; bad = 0; }
    else if (nslot < 1 || nslot > COND_MAX_SLOTS) { why = "nslot must be in [1, 16384]"; bad = 0; }
    for (int32_t i = 0; i < nq && !why; i++) {
        const int32_t *qq = queries + 4 * (size_t)i;
        const int64_t a = qq[0], b = qq[1], lo = windows[2 * (size_t)i], hi = windows[2 * (size_t)i + 1];
        if (a < 0 || b >= N || a > b) why = "a query needs 0 <= first <= last < num_segments";
        else if (lo < 0 || hi >= N || lo > a || hi < b) why = "a window needs 0 <= lo <= first and last <= hi < num_segments";
        else if (chain[lo] != chain[hi]) why = "a window crosses a chain end";
        else if (hi - lo + 1 > (int64_t)nslot) why = "a window is longer than nslot";
        else if (b - a + 1 > (int64_t)COND_MAX_RUN) why = "an evidence run is longer than 4096 segments";
        else if (qq[2] < -1 || qq[2] >= nmask) why = "mask index out of range";
        else if (qq[3] < -1 || qq[3] >= nlabel) why = "label index out of range";
        if (why) bad = i;
    }
    if (reason) *reason = why;
    return bad;
}
// the most (restart, query) pairs of a chunk: a pair has `per` doubles of output (and 16 bytes of staged query) and `strip`
// doubles of U rows; the outputs stay within COND_OUT_BUDGET and the strips within COND_WS_BUDGET, and a chunk never holds less
// than one pair
inline size_t conditional_pairs(size_t per, size_t strip) {
    const size_t by_out = COND_OUT_BUDGET / (per * 8 + 16), by_ws = COND_WS_BUDGET / (std::max<size_t>(strip, 1) * 8);
    return std::max<size_t>(1, std::min(by_out, by_ws));
}

// rmx_region_decode.  Its max_len rule: 1 <= max_len <= DECODE_MAX_LEN
constexpr int32_t DECODE_MAX_LEN = 16384;
constexpr int32_t DECODE_MAX_STATES = 1024;
constexpr size_t DECODE_OUT_BUDGET = (size_t)64 << 20;      // outputs and queries of a chunk, bytes
constexpr size_t DECODE_BP_BUDGET = (size_t)1 << 30;        // back-pointer strips of a chunk, bytes (1 GiB: 1280 arm-sized strips at 355 states, five workgroups per CU)
inline bool decode_max_len_ok(int32_t max_len) { return max_len >= 1 && max_len <= DECODE_MAX_LEN; }
// every query [nq][4] = (a, b, .., ..) has a <= b and b - a + 1 <= max_len (no overflow for any int32 pair).  Returns the
// index of the first query that breaks a rule, with *reason (a string literal), or -1
inline int64_t check_decode_lengths(int32_t nq, const int32_t *queries, int32_t max_len, const char **reason) {
    const char *why = nullptr;
    int64_t bad = -1;
    if (nq < 0 || (nq > 0 && !queries)) { why = "bad arguments"; bad = 0; }
    else if (!decode_max_len_ok(max_len)) { why = "max_len must be in [1, 16384]"; bad = 0; }
    for (int32_t i = 0; i < nq && !why; i++) {
        const int64_t a = queries[4 * (size_t)i], b = queries[4 * (size_t)i + 1];
        if (a > b) why = "a query needs first <= last";
        else if (b - a + 1 > (int64_t)max_len) why = "a query is longer than max_len";
        if (why) bad = i;
    }
    if (reason) *reason = why;
    return bad;
}
// The chunks of a call over nr restarts and nq queries at S states: blocks of nrc restarts, chunks of qc queries.  A chunk
// holds, per (restart, query), a back-pointer strip of max_len * S int16, a log-probability (double) and max_len states
// (int16), and per query 16 bytes of staged query.  nrc and qc are the largest with
//   nrc * qc * strip_bytes <= DECODE_BP_BUDGET   and   qc * (nrc * (8 + 2 max_len) + 16) + 8 <= DECODE_OUT_BUDGET (8: alignment),
// nrc <= 65535 (a grid dimension) taken first, and never below one restart and one query: the largest strip, 16384 * 1024 * 2
// bytes = 32 MiB, and the largest single output, 8 + 32768 + 16 bytes, fit their budgets.  The staging buffer, in doubles:
// logp [nrc][qc] at 0, states int16 [nrc][qc][max_len] at states_at, queries int32 [qc][4] at queries_at, out_doubles in all
struct DecodePlan {
    int32_t nrc, qc;
    size_t strip_elems;       // int16 per (restart, query) strip
    size_t bp_elems;          // int16 of back-pointer scratch: nrc * qc * strip_elems
    size_t states_at, queries_at, out_doubles;
};
inline int decode_plan(int32_t nr, int32_t nq, int32_t S, int32_t max_len, DecodePlan *p) {
    if (!p || nr < 1 || nq < 1 || S < 1 || S > DECODE_MAX_STATES || !decode_max_len_ok(max_len)) return 5;
    const size_t strip = (size_t)max_len * (size_t)S, strip_bytes = strip * 2, per_out = 8 + 2 * (size_t)max_len;
    const size_t strips = std::max<size_t>(1, DECODE_BP_BUDGET / strip_bytes);
    const size_t nrc = std::min<size_t>(std::min<size_t>((size_t)nr, 65535), std::min<size_t>(strips, std::max<size_t>(1, (DECODE_OUT_BUDGET - 24) / per_out)));
    const size_t qc = std::max<size_t>(1, std::min<size_t>((size_t)nq, std::min<size_t>(strips / nrc, (DECODE_OUT_BUDGET - 8) / (nrc * per_out + 16))));
    p->nrc = (int32_t)nrc; p->qc = (int32_t)qc;
    p->strip_elems = strip;
    p->bp_elems = nrc * qc * strip;
    p->states_at = nrc * qc;
    p->queries_at = p->states_at + (nrc * qc * (size_t)max_len * 2 + 7) / 8;
    p->out_doubles = p->queries_at + 2 * qc;
    return 0;
}

// rmx_region_kbest.  Its rank rule: 1 <= K <= KBEST_MAX_K (a packed back-pointer keeps the rank in three bits)
constexpr int32_t KBEST_MAX_K = 8;
inline bool kbest_k_ok(int32_t K) { return K >= 1 && K <= KBEST_MAX_K; }
// The chunks of a call, as decode_plan's with a rank axis: per (restart, query) a strip of max_len * K * S int16 pointers, K
// log-probabilities (doubles) and K * max_len states (int16), and per query 16 bytes of staged query, under the same two budgets
// (the buffers are the ones rmx_region_decode grows).  The length rules are check_decode_lengths.  nrc and qc are the largest with
//   nrc * qc * strip_bytes <= DECODE_BP_BUDGET   and   qc * (nrc * K * (8 + 2 max_len) + 16) + 8 <= DECODE_OUT_BUDGET,
// nrc <= 65535 taken first, and never below one restart and one query: the largest strip, 16384 * 8 * 1024 * 2 bytes = 256 MiB,
// and the largest single output, 8 * (8 + 32768) + 16 bytes, fit their budgets.  The staging buffer, in doubles: logp [nrc][qc][K]
// at 0, states int16 [nrc][qc][K][max_len] at states_at, queries int32 [qc][4] at queries_at, out_doubles in all
struct KbestPlan {
    int32_t nrc, qc;
    size_t strip_elems;       // int16 per (restart, query) strip
    size_t bp_elems;          // int16 of back-pointer scratch: nrc * qc * strip_elems
    size_t states_at, queries_at, out_doubles;
};
inline int kbest_plan(int32_t nr, int32_t nq, int32_t S, int32_t K, int32_t max_len, KbestPlan *p) {
    if (!p || nr < 1 || nq < 1 || S < 1 || S > DECODE_MAX_STATES || !kbest_k_ok(K) || !decode_max_len_ok(max_len)) return 5;
    const size_t strip = (size_t)max_len * (size_t)K * (size_t)S, strip_bytes = strip * 2, per_out = (size_t)K * (8 + 2 * (size_t)max_len);
    const size_t strips = std::max<size_t>(1, DECODE_BP_BUDGET / strip_bytes);
    const size_t nrc = std::min<size_t>(std::min<size_t>((size_t)nr, 65535), std::min<size_t>(strips, std::max<size_t>(1, (DECODE_OUT_BUDGET - 24) / per_out)));
    const size_t qc = std::max<size_t>(1, std::min<size_t>((size_t)nq, std::min<size_t>(strips / nrc, (DECODE_OUT_BUDGET - 8) / (nrc * per_out + 16))));
    p->nrc = (int32_t)nrc; p->qc = (int32_t)qc;
    p->strip_elems = strip;
    p->bp_elems = nrc * qc * strip;
    p->states_at = nrc * qc * (size_t)K;
    p->queries_at = p->states_at + (nrc * qc * (size_t)K * (size_t)max_len * 2 + 7) / 8;
    p->out_doubles = p->queries_at + 2 * qc;
    return 0;
}

// rmx_region_extremes.  Its column rule: 1 <= ncol <= EXTREMES_MAX_COL (the columns of the matrix instruction's B operand)
constexpr int32_t EXTREMES_MAX_COL = 16;
inline bool extremes_ncol_ok(int32_t ncol) { return ncol >= 1 && ncol <= EXTREMES_MAX_COL; }
// the level tables [C][nlevel][S] of a call hold no negative entry.  Returns the index of the first entry that does, -1 if
// there is none, or -2 for arguments that describe no table (a negative extent, or entries without a pointer)
inline int64_t check_levels(int64_t C, int64_t nlevel, int64_t S, const int16_t *levels) {
    if (C < 0 || nlevel < 0 || S < 0) return -2;
    const uint64_t n = (uint64_t)C * (uint64_t)nlevel * (uint64_t)S;      // (each extent is below 2^31 in a batch; the caller's are int32)
    if (n > 0 && !levels) return -2;
    for (uint64_t i = 0; i < n; i++) if (levels[i] < 0) return (int64_t)i;
    return -1;
}

// rmx_locus_joint.  Its shape rule: 1 <= nrow, ncol <= LOCUS_MAX_LEVELS (the 16 x 16 threads of an emission, the columns of the
// matrix instruction's B operand), 0 <= nslot <= LOCUS_MAX_SLOTS (0: the pair form), and a (restart, query) output of
// max(nslot, 1) nrow ncol <= LOCUS_MAX_ENTRIES doubles (no overflow for any int32 triple)
constexpr int32_t LOCUS_MAX_LEVELS = 16;
constexpr int32_t LOCUS_MAX_SLOTS = 4096;
constexpr int64_t LOCUS_MAX_ENTRIES = (int64_t)1 << 20;
inline bool locus_shape_ok(int32_t nrow, int32_t ncol, int32_t nslot) {
    if (nrow < 1 || nrow > LOCUS_MAX_LEVELS || ncol < 1 || ncol > LOCUS_MAX_LEVELS || nslot < 0 || nslot > LOCUS_MAX_SLOTS) return false;
    return (int64_t)std::max<int32_t>(nslot, 1) * nrow * ncol <= LOCUS_MAX_ENTRIES;
}
// every query [nq][4] = (a, t, .., ..) has a <= t, and in the profile form (nslot >= 1) t - a + 1 <= nslot: slot t - a is
// the last one the kernel writes (no overflow for any int32 pair).  Returns the index of the first query that breaks a rule,
// with *reason (a string literal), or -1
inline int64_t check_locus_lengths(int32_t nq, const int32_t *queries, int32_t nslot, const char **reason) {
    const char *why = nullptr;
    int64_t bad = -1;
    if (nq < 0 || (nq > 0 && !queries)) { why = "bad arguments"; bad = 0; }
    else if (nslot < 0 || nslot > LOCUS_MAX_SLOTS) { why = "nslot must be in [0, 4096]"; bad = 0; }
    for (int32_t i = 0; i < nq && !why; i++) {
        const int64_t a = queries[4 * (size_t)i], t = queries[4 * (size_t)i + 1];
        if (a > t) why = "a query needs first <= last";
        else if (nslot >= 1 && t - a + 1 > (int64_t)nslot) why = "a profile query is longer than nslot";
        if (why) bad = i;
    }
    if (reason) *reason = why;
    return bad;
}

// rmx_region_automaton.  Its shape rule: 1 <= Q <= AUTOMATON_MAX_STATES (the columns of the matrix instruction's B operand),
// 1 <= A <= AUTOMATON_MAX_SYMBOLS (the rows of the kernel's predecessor table), 1 <= nauto <= AUTOMATON_MAX_AUTOMATA
constexpr int32_t AUTOMATON_MAX_STATES = 16;
constexpr int32_t AUTOMATON_MAX_SYMBOLS = 16;
constexpr int32_t AUTOMATON_MAX_AUTOMATA = 64;
inline bool automaton_shape_ok(int32_t nauto, int32_t Q, int32_t A) {
    return nauto >= 1 && nauto <= AUTOMATON_MAX_AUTOMATA && Q >= 1 && Q <= AUTOMATON_MAX_STATES && A >= 1 && A <= AUTOMATON_MAX_SYMBOLS;
}
// the transition tables delta [nauto][Q][A] hold states in [0, Q) and start [nauto] does.  Returns the index of the first bad
// entry -- of delta as a flat index, of start[i] as nauto Q A + i -- -1 if there is none, or -2 for arguments that describe no
// tables (a shape outside the rule, or a missing pointer)
inline int64_t check_automata(int32_t nauto, int32_t Q, int32_t A, const uint8_t *delta, const int32_t *start) {
    if (!automaton_shape_ok(nauto, Q, A) || !delta || !start) return -2;
    const int64_t n = (int64_t)nauto * Q * A;      // (at most 64 x 16 x 16)
    for (int64_t i = 0; i < n; i++) if ((int32_t)delta[i] >= Q) return i;
    for (int32_t i = 0; i < nauto; i++) if (start[i] < 0 || start[i] >= Q) return n + i;
    return -1;
}
// the symbol tables [C][nsym][S] of a call hold symbols in [0, A).  Returns the index of the first entry outside, -1 if there
// is none, or -2 for arguments that describe no table (a negative extent, A < 1, or entries without a pointer)
inline int64_t check_symbols(int64_t C, int64_t nsym, int64_t S, int32_t A, const int16_t *symbols) {
    if (C < 0 || nsym < 0 || S < 0 || A < 1) return -2;
    const uint64_t n = (uint64_t)C * (uint64_t)nsym * (uint64_t)S;      // (each extent is below 2^31 in a batch; the caller's are int32)
    if (n > 0 && !symbols) return -2;
    for (uint64_t i = 0; i < n; i++) if (symbols[i] < 0 || (int32_t)symbols[i] >= A) return (int64_t)i;
    return -1;
}

// rmx_region_sums.  The kernel keeps G [S rounded up to 16][16 CT] doubles in LDS, CT = 1, 2 or 4 column tiles
// of 16 bins, beside a row of doubles, one int16 level row and the compacted int16 index: SR (128 CT + 12) bytes, which must
// fit the 160 KiB of a workgroup together with the kernel's static LDS (SUMS_STATIC_LDS bytes at the most).  So the most
// bins a call may ask for is 64 up to 304 states, 32 up to 608 and 16 up to SUMS_MAX_STATES; 0 beyond (unsupported)
constexpr int32_t SUMS_MAX_BINS = 64;
constexpr int32_t SUMS_MAX_STATES = 1024;
constexpr int64_t SUMS_LDS_LIMIT = 160 * 1024;
constexpr int64_t SUMS_STATIC_LDS = 64;
// the column tiles of 16 that hold nbins bins: 1, 2 or 4 (0 for nbins outside [1, SUMS_MAX_BINS])
inline int32_t sums_column_tiles(int32_t nbins) {
    if (nbins < 1 || nbins > SUMS_MAX_BINS) return 0;
    return nbins <= 16 ? 1 : (nbins <= 32 ? 2 : 4);
}
// the dynamic LDS of a call with nbins bins at S states, in bytes (0 for arguments outside the rules above)
inline int64_t sums_lds_bytes(int32_t S, int32_t nbins) {
    const int32_t ct = sums_column_tiles(nbins);
    if (S < 1 || S > SUMS_MAX_STATES || !ct) return 0;
    const int64_t SR = ((int64_t)S + 15) / 16 * 16;
    return SR * (128 * (int64_t)ct + 12);
}
inline int32_t sums_max_bins(int32_t S) {
    for (int32_t nbins = SUMS_MAX_BINS; nbins >= 16; nbins /= 2) {
        const int64_t lds = sums_lds_bytes(S, nbins);
        if (lds > 0 && lds + SUMS_STATIC_LDS <= SUMS_LDS_LIMIT) return nbins;
    }
    return 0;
}
// the increment of a state of level `level` on a segment of weight w: min(w level, nbins - 1) with a 64-bit product (w up to
// 2^31 - 1 times a level up to 32767 overflows 32 bits).  w, level >= 0 and nbins >= 1 are the caller's to check
inline int32_t sum_increment(int32_t w, int32_t level, int32_t nbins) {
    const int64_t p = (int64_t)w * (int64_t)level;
    return p < (int64_t)nbins - 1 ? (int32_t)p : nbins - 1;
}
// the weight pool [nwt] holds no negative entry.  Returns the index of the first entry that does, -1 if there is none, or -2
// for arguments that describe no pool
inline int64_t check_weights(int64_t nwt, const int32_t *weights) {
    if (nwt < 0 || (nwt > 0 && !weights)) return -2;
    for (int64_t i = 0; i < nwt; i++) if (weights[i] < 0) return i;
    return -1;
}
// every query [nq][4] = (a, b, .., o) with a <= b keeps its weights o .. o + (b - a) inside the pool: 0 <= o and
// o + (b - a) < nwt (no overflow for any int32 triple).  Returns the index of the first query that does not (a > b is one),
// -1 if there is none, or -2 for arguments that describe no queries
inline int64_t check_sum_spans(int32_t nq, const int32_t *queries, int64_t nwt) {
    if (nq < 0 || (nq > 0 && !queries) || nwt < 0) return -2;
    for (int32_t i = 0; i < nq; i++) {
        const int64_t a = queries[4 * (size_t)i], b = queries[4 * (size_t)i + 1], o = queries[4 * (size_t)i + 3];
        if (a > b || o < 0 || o + (b - a) >= nwt) return i;
    }
    return -1;
}

// rmx_path_entropy.  Its segment range [n0, n1) of a model of N segments: 0 <= n0 < n1 <= N
inline bool entropy_range_ok(int64_t N, int64_t n0, int64_t n1) { return n0 >= 0 && n0 < n1 && n1 <= N; }
// the work lists of the range [n0, n1): the plain adjacencies n -> n + 1 (tclass[n] in [0, TC), brk_slot[n] < 0) bucketed by
// transition class, classes ascending and n ascending inside a class, into tiles of ENTROPY_TILE indices -- tiles_out
// [tiles][1 + ENTROPY_TILE] = class, then the indices, the last tile of a class padded with -1; the breakend adjacencies
// (tclass[n] >= 0, brk_slot[n] >= 0) in ascending n -> singles_out [singles].  Chain ends (tclass[n] < 0) go into neither.
// Returns the two counts; with a null output pointer that list is only counted.  {-1, -1} for arguments that describe no range
// (a negative n0, n1 < n0, missing tables, TC < 0) or a class at or beyond TC
constexpr int32_t ENTROPY_TILE = 16;
struct EntropyCounts { int64_t tiles, singles; };
inline EntropyCounts entropy_tiles(int32_t n0, int32_t n1, const int32_t *tclass, const int32_t *brk_slot, int32_t TC, int32_t *tiles_out, int32_t *singles_out) {
    if (n0 < 0 || n1 < n0 || !tclass || !brk_slot || TC < 0) return {-1, -1};
    std::vector<int64_t> cnt((size_t)TC, 0);
    int64_t singles = 0;
    for (int32_t n = n0; n < n1; n++) {
        if (tclass[n] < 0) continue;
        if (tclass[n] >= TC) return {-1, -1};
        if (brk_slot[n] >= 0) { if (singles_out) singles_out[singles] = n; singles++; }
        else cnt[(size_t)tclass[n]]++;
    }
    // first tile of a class, then the number of indices placed in it so far
    std::vector<int64_t> first((size_t)TC, 0);
    int64_t tiles = 0;
    for (int32_t c = 0; c < TC; c++) { first[(size_t)c] = tiles; tiles += (cnt[(size_t)c] + ENTROPY_TILE - 1) / ENTROPY_TILE; }
    if (tiles_out) {
        for (int32_t c = 0; c < TC; c++)
            for (int64_t t = first[(size_t)c]; t < (c + 1 < TC ? first[(size_t)c + 1] : tiles); t++) {
                int32_t *row = tiles_out + t * (1 + ENTROPY_TILE);
                row[0] = c;
                std::fill(row + 1, row + 1 + ENTROPY_TILE, (int32_t)-1);
            }
        std::fill(cnt.begin(), cnt.end(), (int64_t)0);
        for (int32_t n = n0; n < n1; n++) {
            if (tclass[n] < 0 || brk_slot[n] >= 0) continue;
            const size_t c = (size_t)tclass[n];
            const int64_t k = cnt[c]++;
            tiles_out[(first[c] + k / ENTROPY_TILE) * (1 + ENTROPY_TILE) + 1 + k % ENTROPY_TILE] = n;
        }
    }
    return {tiles, singles};
}
// segments per staging chunk of a call over nr restarts and nseg segments: the two output planes of a chunk, nr x chunk doubles
// each, stay inside budget_bytes; at least 1 (a budget below one segment still makes progress), at most nseg
inline int64_t entropy_chunk(int64_t nr, int64_t nseg, int64_t budget_bytes) {
    if (nr < 1 || nseg < 1) return 1;
    const int64_t per_seg = nr > INT64_MAX / 16 ? INT64_MAX : nr * 16;
    return std::max<int64_t>(1, std::min<int64_t>(nseg, budget_bytes / per_seg));
}

// rmx_restart_overlap.  Its pairs [npairs][2]: a restart of batch A in [0, RA) and one of batch B in [0, RB).  Returns the index
// of the first pair outside, -1 if there is none, or -2 for arguments that describe no list (no pair, or pairs without a pointer)
inline int64_t check_pairs(int64_t npairs, const int32_t *pairs, int64_t RA, int64_t RB) {
    if (npairs < 1 || !pairs || RA < 0 || RB < 0) return -2;
    for (int64_t i = 0; i < npairs; i++)
        if (pairs[2 * i] < 0 || pairs[2 * i] >= RA || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= RB) return i;
    return -1;
}
// its state permutations [nperm][C][S]: every row is a bijection of [0, S).  Returns the index (p * C + c) of the first row that
// is not -- an entry outside [0, S) or a repeated one --, -1 if there is none, or -2 for arguments that describe no table
inline int64_t check_permutations(int64_t nperm, int64_t C, int64_t S, const int16_t *perms) {
    if (nperm < 1 || C < 1 || S < 1 || S > 32767 || !perms) return -2;
    std::vector<uint8_t> seen((size_t)S);
    for (int64_t row = 0; row < nperm * C; row++) {
        std::fill(seen.begin(), seen.end(), (uint8_t)0);
        const int16_t *p = perms + (size_t)row * (size_t)S;
        for (int64_t s = 0; s < S; s++) {
            if (p[s] < 0 || p[s] >= S || seen[(size_t)p[s]]) return row;
            seen[(size_t)p[s]] = 1;
        }
    }
    return -1;
}

inline int compress_cn_states(const int64_t *cn_states, int32_t N, int32_t S, int32_t M, int32_t max_classes,
                              int32_t *seg_class_out, int64_t *classes_out, int32_t *num_classes) {
    if (!cn_states || !seg_class_out || !classes_out || !num_classes) return 5;
    const size_t tsz = (size_t)S * M * 2;
    int C = 0;
    for (int n = 0; n < N; n++) {
        const int64_t *t = cn_states + (size_t)n * tsz;
        int found = -1;
        if (n > 0 && memcmp(t, classes_out + (size_t)seg_class_out[n - 1] * tsz, tsz * 8) == 0) found = seg_class_out[n - 1];
        for (int c = 0; c < C && found < 0; c++) if (memcmp(t, classes_out + (size_t)c * tsz, tsz * 8) == 0) found = c;
        if (found < 0) {
            if (C >= max_classes) return 4;
            memcpy(classes_out + (size_t)C * tsz, t, tsz * 8);
            found = C++;
        }
        seg_class_out[n] = found;
    }
    *num_classes = C;
    return 0;
}

// Total-copy classes of the state tables.  The read-depth likelihood of a (segment, state) cell depends on the state only
// through its expected depth sum_m h[m] * tot[m] and the hdel branch, so the states of one table that share the tuple
// tot[0..M) and the hdel bit share the value to the bit.  Per state-table class c: ltcls[c * S + s] is the total-copy class
// of state s, numbered in order of first appearance; ltrep[c * S + k] the first state of class k (-1 past the table's
// count); count[c] the number of classes of table c; *NT the largest count.
inline int lt_classes(const int64_t *cn_classes, int32_t C, int32_t S, int32_t M,
                      std::vector<int32_t> &ltcls, std::vector<int32_t> &ltrep, std::vector<int32_t> &count, int32_t *NT) {
    if (!cn_classes || !NT || C < 1 || S < 1 || M < 1) return 5;
    ltcls.assign((size_t)C * S, -1); ltrep.assign((size_t)C * S, -1); count.assign((size_t)C, 0);
    std::vector<int64_t> keys((size_t)S * (M + 1)), key((size_t)M + 1);
    int32_t nt = 0;
    for (int c = 0; c < C; c++) {
        int k = 0;
        for (int s = 0; s < S; s++) {
            const int64_t *t = cn_classes + ((size_t)c * S + s) * M * 2;
            bool hdel = true;
            for (int m = 0; m < M; m++) { key[(size_t)m] = t[m * 2] + t[m * 2 + 1]; if (t[m * 2] != 0 || t[m * 2 + 1] != 0) hdel = false; }
            key[(size_t)M] = hdel ? 1 : 0;
            int found = -1;
            for (int j = 0; j < k && found < 0; j++) if (std::equal(key.begin(), key.end(), keys.begin() + (size_t)j * (M + 1))) found = j;
            if (found < 0) { std::copy(key.begin(), key.end(), keys.begin() + (size_t)k * (M + 1)); ltrep[(size_t)c * S + k] = s; found = k++; }
            ltcls[(size_t)c * S + s] = found;
        }
        count[(size_t)c] = k;
        nt = std::max(nt, (int32_t)k);
    }
    *NT = nt;
    return 0;
}

inline int weighted_search(const double *p, int64_t n, const double *u, int32_t k, int64_t *out, int64_t *positive) {
    if (!p || n < 1 || (k > 0 && (!u || !out))) return 5;
    std::vector<double> cdf((size_t)n);
    double acc = 0.;
    int64_t pos = 0;
    for (int64_t i = 0; i < n; i++) { acc += p[i]; cdf[(size_t)i] = acc; pos += p[i] > 0.; }
    const double last = cdf[(size_t)n - 1];
    for (int64_t i = 0; i < n; i++) cdf[(size_t)i] /= last;
    for (int32_t j = 0; j < k; j++) {
        const int64_t idx = (int64_t)(std::upper_bound(cdf.begin(), cdf.end(), u[j]) - cdf.begin());
        out[j] = std::min<int64_t>(idx, n - 1);
    }
    if (positive) *positive = pos;
    return 0;
}

// One round of the weighted M-step sampling (remixt_amd/cn_model.py _sample_without_replacement: `size` distinct indices, successively
// with probability proportional to the weights = numpy's choice(replace=False, p=...), reference remixt/cn_model.py:475-480): the
// weights are w[i * stride] / norm (a column of an (N, 2) indicator array, normalised like numpy's `weights / weights.sum()`), the
// k uniform draws u select indices from their cumulative sum exactly as weighted_search does, and the indices not seen before are
// appended to found[0 .. *nfound) in the order of the draws (numpy: unique(concatenate(found, new)) by first occurrence), up to cap.
inline int weighted_sample_round(const double *w, int64_t n, int64_t stride, double norm, const double *u, int32_t k,
                                 int64_t *found, int32_t *nfound, int32_t cap, int64_t *positive) {
    if (!w || n < 1 || stride < 1 || !(norm > 0.) || (k > 0 && !u) || !found || !nfound || *nfound < 0 || *nfound > cap) return 5;
    std::vector<double> cdf((size_t)n);
    double acc = 0.;
    int64_t pos = 0;
    for (int64_t i = 0; i < n; i++) { const double p = w[(size_t)(i * stride)] / norm; acc += p; cdf[(size_t)i] = acc; pos += p > 0.; }
    const double last = cdf[(size_t)n - 1];
    for (int64_t i = 0; i < n; i++) cdf[(size_t)i] /= last;
    if (positive) *positive = pos;
    std::vector<int64_t> seen(found, found + *nfound);
    std::sort(seen.begin(), seen.end());
    int32_t nf = *nfound;
    for (int32_t j = 0; j < k && nf < cap; j++) {
        int64_t idx = (int64_t)(std::upper_bound(cdf.begin(), cdf.end(), u[j]) - cdf.begin());
        idx = std::min<int64_t>(idx, n - 1);
        auto it = std::lower_bound(seen.begin(), seen.end(), idx);
        if (it != seen.end() && *it == idx) continue;
        seen.insert(it, idx);
        found[nf++] = idx;
    }
    *nfound = nf;
    return 0;
}

// scipy.optimize.fmin (Nelder-Mead, one variable, xatol = fatol = 1e-4, maxiter = maxfun = 200) as a
// resumable state machine: same floating-point operations in the same order as scipy's
// _minimize_neldermead (python twin: remixt_amd/lockstep.py fmin_1d; tests compare the two).
struct Nm1 {
    enum { START, W_INIT0, W_INIT1, W_XR, W_XE, W_XC, W_XCC, W_SHRINK, DONE };
    double s0 = 0, s1 = 0, f0 = INFINITY, f1 = INFINITY, xbar = 0, xr = 0, fxr = 0, xe = 0, xc = 0, xcc = 0, req = 0, last = 0;
    int fcalls = 0, iters = 0, state = START;
    static constexpr int maxfun = 200, maxiter = 200;
    static constexpr double xatol = 1e-4, fatol = 1e-4;
    RMX_HD bool request(double x, int next) { if (fcalls >= maxfun) return false; fcalls++; req = x; last = x; state = next; return true; }
    RMX_HD void sort() { if (f1 < f0) { double t_ = f0; f0 = f1; f1 = t_; t_ = s0; s0 = s1; s1 = t_; } }
    // feed the value of the last request (ignored on the first call); true = `req` holds the next point
    RMX_HD bool advance(double x0, double f) {
#pragma clang fp contract(off)
        switch (state) {
        case START:
            s0 = x0; s1 = x0 != 0. ? (1 + 0.05) * x0 : 0.00025;
            if (request(s0, W_INIT0)) return true;
            goto init_done;
        case W_INIT0:
            f0 = f;
            if (request(s1, W_INIT1)) return true;
            goto init_done;
        case W_INIT1:
            f1 = f;
            goto init_done;
        case W_XR:
            fxr = f;
            if (fxr < f0) {
                xe = 3. * xbar - 2. * s1;
                if (request(xe, W_XE)) return true;
                goto maxfun_exit;
            }
            // N = 1: fsim[-2] is fsim[0], so "fxr < fsim[-2]" cannot hold here
            if (fxr < f1) {
                xc = 1.5 * xbar - 0.5 * s1;
                if (request(xc, W_XC)) return true;
                goto maxfun_exit;
            }
            xcc = 0.5 * xbar + 0.5 * s1;
            if (request(xcc, W_XCC)) return true;
            goto maxfun_exit;
        case W_XE:
            if (f < fxr) { s1 = xe; f1 = f; } else { s1 = xr; f1 = fxr; }
            goto iter_done;
        case W_XC:
            if (f <= fxr) { s1 = xc; f1 = f; goto iter_done; }
            goto shrink;
        case W_XCC:
            if (f < f1) { s1 = xcc; f1 = f; goto iter_done; }
            goto shrink;
        case W_SHRINK:
            f1 = f;
            goto iter_done;
        default:
            return false;
        }
    shrink:
        s1 = s0 + 0.5 * (s1 - s0);
        if (request(s1, W_SHRINK)) return true;
        goto maxfun_exit;
    init_done:
        sort();
        iters = 1;
        goto loop_top;
    iter_done:
        iters++;
    maxfun_exit:
        sort();
    loop_top:
        if (fcalls < maxfun && iters < maxiter) {
            if (!(fabs(s1 - s0) <= xatol && fabs(f0 - f1) <= fatol)) {
                xbar = s0 / 1;
                xr = 2. * xbar - 1. * s1;
                if (request(xr, W_XR)) return true;
                goto maxfun_exit;      // cannot happen (fcalls < maxfun was just checked); mirrors the python flow
            }
        }
        state = DONE;
        return false;
    }
    RMX_HD double xopt() const { return s0; }
};

}  // namespace rmxh
#endif
