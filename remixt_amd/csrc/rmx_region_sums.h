// rmx_region_sums.h -- k_region_sums, included from rmx_api.hip behind rmx_kernels.h: it uses the pieces the region
// query kernels share (RgnArgs, rgn_adj, rgn_compact, rgn_D_exp, rgn_take_sum, rgn_block_sum, rga_symbol_row, group_sum).
#ifndef RMX_REGION_SUMS_H
#define RMX_REGION_SUMS_H

// =============================================================================
// Region sums: for a query (a, b, level table, weight offset o) over the model segments [a, b] of one chain and
// B <= 64 bins, the exact distribution of the additive functional sum_n w_n level_n(c_n), w_n = weights[o + n - a] >= 0,
// level_n(s) >= 0 the level of state s under the state class of segment n, with the last bin absorbing: bin B - 1 is ">= B - 1".
// The pair (copy-number state, running sum) is a Markov chain under the structured posterior; with the increment
// d_n(s) = min((int64) w_n level_n(s), B - 1) and H(s', k) = G_n+1(s', k) / D_n(s'),
//   G_b(s, k)     = post_b(s) [k = d_b(s)]
//   X(s, k)       = fa_n(s) sum_s' W_n(s, s') H(s', k)
//   G_n(s, k)     = X(s, k - d_n(s))                          for d_n(s) <= k < B - 1   (0 for k < d_n(s))
//   G_n(s, B - 1) = sum_{k' = B-1-d_n(s)}^{B-1} X(s, k')      (ascending k')
//   out(k)        = log sum_s G_a(s, k).
// It is k_region_automaton's walk with a wider column axis and a shift in place of pred.  Nothing binds: in real arithmetic
// the total over (s, k) is 1 at every step.  G is still divided by its total after every step, the start included, and the
// logarithms are added up.  ONE scale carries all columns, because columns mix under the shift: a bin more than about 1e-308
// below the total comes out -inf.  Nothing of the model is written.
// One workgroup of 256 threads per (restart, query).  CT = 1, 2 or 4 column tiles of 16; W = 16 CT columns, the columns >= B
// hold +0.  G lives in LDS as [S rounded up to 16][W]; a step is
//   1. the states s' with mass in any of the W columns (the set does not depend on B), compacted in state order by a ballot;
//   2. one D(s') for those, as in k_region_automaton; lane j divides columns j, j + 16, .. in place;
//   3. X on v_mfma_f64_16x16x4_f64 with k_region_automaton's lane map: the A operand W(s0 + i, s'_k), selected to 0 where
//      fa = 0 or s >= S, is loaded ONCE per (row tile, four s') and issued against the CT B operands H(s'_k, 16 c + j) into
//      CT accumulators per row tile;
//   4. the epilogue through LDS: fa X goes from the accumulators to G once every wave has finished reading H; thread (s, k)
//      then reads X(s, k - d_n(s)), or the ascending tail sum for k = B - 1, and writes G_n(s, k) -- an operand is selected,
//      never multiplied by 0.  A row's W <= 64 columns belong to lanes of one wave in one round (RGN_NT is a multiple of W, and
//      W divides 64): the row is read before any lane writes it.  The tail loop does not diverge: every lane of the wave walks
//      the longest tail of the wave's rows and selects its operands, so every store follows every load.  On a segment of weight 0 the epilogue is the identity and no level row is loaded;
//   5. the total in a fixed order, and G divided by it in place.
// q.labels / q.nlabel carry the level tables (every entry >= 0, the host checked); fields 2 and 3 of a query are the level
// table and the offset of the run's weights in wts (the host checked the span and that no weight is negative).  Every sum has
// one order, fixed by S and CT alone: a (restart, query) result depends on neither the restart range, the other queries, the
// launch, nor on where its weights lie in the pool.  Only columns s < S of fa / post are read (clamped address and select).
// A D(s') that is 0 or not finite under mass, or a total that is not a finite number >= 0, sets RGN_ERR_DENOM in flags[r] and
// gives NaN in all B entries; a bin that cannot be reached gives -inf.
// grid (queries, restarts), block RGN_NT, dynamic LDS rgs_lds_bytes(S, CT); out[(ri * nq + query) * B + k].
// =============================================================================
static inline size_t rgs_lds_bytes(int S, int CT) { const size_t SR = ((size_t)S + 15) & ~(size_t)15; return SR * ((size_t)CT * RGN_KB * 8 + 8 + 2 * 2); }
// the increment of a state of level lv on a segment of weight w: the 64-bit product, saturated at the last bin
__device__ __forceinline__ int rgs_increment(int w, int lv, int B) {
    const long long p = (long long)w * (long long)lv;
    return p < (long long)(B - 1) ? (int)p : B - 1;
}
// the sums over s < S of the first nc <= W columns of G [S][W], W = 16 CT: thread t takes column t % W of the rows
// t / W, t / W + RGN_NT / W, ..; the RGN_NT / W partial sums of a column then go through the first rows of G itself (the
// barriers make sure that every thread has read G before), and thread t < nc adds them in ascending order (the others get 0)
template <int CT>
__device__ __forceinline__ double rgs_column_sums(double *G, int S, int nc) {
    constexpr int W = CT * RGN_KB, NG = RGN_NT / W;
    const int tid = threadIdx.x, k = tid % W, g = tid / W;
    double p = 0.;
    for (int s = g; s < S; s += NG) p += G[s * W + k];
    __syncthreads();
    G[g * W + k] = p;         // (NG W = RGN_NT doubles: G has at least 16 W >= NG W of them)
    __syncthreads();
    double t = 0.;
    if (tid < nc) {
#pragma unroll
        for (int i = 0; i < NG; i++) t += G[i * W + tid];
    }
    return t;
}
template <int TPW, int CT>
__global__ __launch_bounds__(RGN_NT) void k_region_sums(Dev d, int r0, int use_wb, RgnArgs q, const int32_t *wts, int B, double *out, uint32_t *flags) {
    constexpr int W = CT * RGN_KB;                      // columns of a row of G
    extern __shared__ double rgs_lds[];                 // G [SR][W], fas [SR], lev [SR] (int16), idx [SR] (int16)
    __shared__ double red[RGN_NW];
    __shared__ int nact, s_bad;
    const int qi = blockIdx.x, ri = blockIdx.y, r = r0 + ri, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform, and known to be: the matrix instructions sit under conditions on it)
    const int grp = tid / RGN_GL, gl = tid % RGN_GL;
    const int ai = lane & 15, kk = lane >> 4;
    const int col = tid % W;                            // (the thread's column in every pass over e = tid, tid + RGN_NT, ..)
    const int S = d.S, SR = (S + 15) & ~15;
    double *G = rgs_lds, *fas = G + (size_t)SR * W;
    int16_t *lev = (int16_t *)(fas + SR), *idx = lev + SR;
    const int a = q.queries[4 * qi], b = q.queries[4 * qi + 1], li = q.queries[4 * qi + 2];
    const int32_t *wq = wts + q.queries[4 * qi + 3];    // w_n = wq[n - a]
    if (tid == 0) s_bad = 0;
    double logp = 0.;
    bool failed = false;
    // ---- start: G_b(s, k) = post_b(s) [k = d_b(s)] ----------------------------------------------------------------------
    {
        const double *post = d.post + rs_off(d, r, b);
        const int w = wq[b - a];
        if (w != 0) rga_symbol_row(d, q, b, li, S, SR, lev);
        __syncthreads();
        double part = 0.;
        for (int e = tid; e < SR * W; e += RGN_NT) {      // (e % W == col: RGN_NT is a multiple of W)
            const int s = e / W, sc = s < S ? s : S - 1;
            const double pv = post[sc];
            const int dn = w != 0 ? rgs_increment(w, lev[s], B) : 0;
            const double v = (s < S && col == dn) ? pv : 0.;
            G[e] = v;
            part += v;
        }
        const double Z = rgn_block_sum(part, red);
        const bool okz = rgn_take_sum(Z, false, logp, failed);
        for (int e = tid; e < SR * W; e += RGN_NT) G[e] = okz ? G[e] / Z : 0.;
    }
    for (int n = b - 1; n >= a && !failed && logp > -INFINITY; n--) {
        const auto [wb, Wt, pd] = rgn_adj(d, r, n, use_wb);
        const double *fa = d.fa + rs_off(d, r, n);
        const int w = wq[n - a];
        for (int s = tid; s < SR; s += RGN_NT) {
            const int sc = s < S ? s : S - 1;
            const double fv = fa[sc];
            fas[s] = s < S ? fv : 0.;
        }
        // ---- 1. the states s' with mass in any column, in state order ------------------------------------------
        __syncthreads();      // (G of the step before, or of the start, is complete, and its level row has been read)
        if (w != 0) rga_symbol_row(d, q, n, li, S, SR, lev);
        const int na = __builtin_amdgcn_readfirstlane(rgn_compact(S, idx, nact, [&](int s) {
            bool act = false;
            for (int k = 0; k < W; k++) act = act || G[s * W + ((k + lane) & (W - 1))] > 0.;      // (rotated by the lane: the lanes' rows are W doubles apart)
            return act;
        }));
        // ---- 2. D(s') and H = G / D in place ---------------------------------------------------------------------
        if (wb) {
            for (int j0 = 0; j0 < na; j0 += RGN_NT / RGN_GL) {
                const int j = j0 + grp;
                const bool ok = j < na;
                const int sp = ok ? idx[j] : 0;
                double p = 0.;
                if (ok) {
                    const double *wr = Wt + (size_t)sp * S;
                    for (int s = gl; s < S; s += RGN_GL) p = fma(fas[s], wr[s], p);
                }
                const double D = group_sum(p, RGN_GL);
                if (ok) {
                    if (gl == 0 && !(D > 0. && D < INFINITY)) s_bad = 1;
#pragma unroll
                    for (int c = 0; c < CT; c++) G[sp * W + c * RGN_KB + gl] = G[sp * W + c * RGN_KB + gl] / D;
                }
            }
        } else {
            for (int j = tid; j < na; j += RGN_NT) {
                const int sp = idx[j];
                const double D = rgn_D_exp(d, n, sp, fas, pd);
                if (!(D > 0. && D < INFINITY)) s_bad = 1;
                for (int k = 0; k < W; k++) G[sp * W + k] = G[sp * W + k] / D;
            }
        }
        __syncthreads();
        // ---- 3. X on the matrix cores: one A operand per (row tile, four s') against the CT column tiles ---------
        psm_d4 acc[TPW][CT];
        bool rowlive[TPW];    // the lane's A row of tile u is a state the walk can pass
#pragma unroll
        for (int u = 0; u < TPW; u++) {
#pragma unroll
            for (int c = 0; c < CT; c++) acc[u][c] = psm_d4{0., 0., 0., 0.};
            const int s = (wave + RGN_NW * u) * 16 + ai;
            rowlive[u] = s < S && fas[s < SR ? s : 0] != 0.;
        }
        for (int j0 = 0; j0 < na; j0 += 4) {
            const int j = j0 + kk;
            const bool ok = j < na;
            const int sp = idx[ok ? j : 0];
            double bv[CT];
#pragma unroll
            for (int c = 0; c < CT; c++) {
                const double hv = G[sp * W + c * RGN_KB + ai];
                bv[c] = ok ? hv : 0.;
            }
#pragma unroll
            for (int u = 0; u < TPW; u++) {
                const int s0 = (wave + RGN_NW * u) * 16;
                if (s0 < S) {         // (uniform over the wave)
                    const int s = s0 + ai, sc = s < S ? s : S - 1;
                    const bool live = ok && rowlive[u];
                    double wv;
                    if (wb) wv = Wt[(size_t)sp * S + sc];
                    else wv = live ? exp(trans_value(d, n, sc, sp, pd)) : 0.;
                    const double av = live ? wv : 0.;
#pragma unroll
                    for (int c = 0; c < CT; c++) acc[u][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[c], acc[u][c], 0, 0, 0);
                }
            }
        }
        // ---- 4. fa X to LDS once every wave has finished reading H, then G_n(s, k) from the row of X ------------------
        __syncthreads();
#pragma unroll
        for (int u = 0; u < TPW; u++) {
            const int s0 = (wave + RGN_NW * u) * 16;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int s = s0 + kk + 4 * g;
                if (s < SR) {
                    const double fv = fas[s];
#pragma unroll
                    for (int c = 0; c < CT; c++) G[s * W + c * RGN_KB + ai] = fv != 0. ? fv * acc[u][c][g] : 0.;
                }
            }
        }
        __syncthreads();
        // (a row's W columns belong to W lanes of one wave in one round: every lane has read the row before any lane of the wave
        // writes it)
        double part = 0.;
        if (w != 0) {
#pragma unroll 1
            for (int e = tid; e < SR * W; e += RGN_NT) {         // (column e % W == col)
                const int s = e / W;
                const int dn = rgs_increment(w, lev[s], B);
                const double *xr = G + s * W;
                const int from = col - dn;
                const double x1 = xr[from > 0 ? from : 0];
                // the tail sum of column B - 1, ascending k' = B - 1 - dn .. B - 1: EVERY lane of the wave walks the longest tail
                // of the wave's 64 / W rows and selects its operands (a lane outside column B - 1, or past its row's tail, adds
                // +0), so the loop does not diverge and every store below follows every load of the wave in program order
                int dmax = dn;
#pragma unroll
                for (int off = W; off < 64; off <<= 1) {
                    const int o = __shfl_xor(dmax, off, 64);
                    dmax = o > dmax ? o : dmax;
                }
                dmax = __builtin_amdgcn_readfirstlane(dmax);
                const bool last = col == B - 1;
                double t = 0.;
                for (int p = 0; p <= dmax; p++) {
                    const bool take = last && p <= dn;
                    const double x = xr[take ? B - 1 - dn + p : 0];
                    t += take ? x : 0.;
                }
                const double v = last ? t : ((col < B - 1 && from >= 0) ? x1 : 0.);
                G[e] = v;
                part += v;
            }
        } else {
            for (int e = tid; e < SR * W; e += RGN_NT) part += G[e];
        }
        // ---- 5. the total in a fixed order (its barriers also publish G), and G divided by it ------------------------------
        const double Z = rgn_block_sum(part, red);
        const bool okz = rgn_take_sum(Z, s_bad != 0, logp, failed);
        for (int e = tid; e < SR * W; e += RGN_NT) G[e] = okz ? G[e] / Z : 0.;
    }
    // ---- out(k) = log sum_s G_a(s, k) -------------------------------------------------------------------------------
    __syncthreads();
    {
        const double t = rgs_column_sums<CT>(G, S, B);
        if (tid < B) {
            double v;
            if (failed) v = __builtin_nan("");
            else if (!(logp > -INFINITY) || t == 0.) v = -INFINITY;
            else v = logp + log(t);
            out[((size_t)ri * q.nq + qi) * B + tid] = v;
        }
    }
    if (tid == 0 && failed) atomicOr(&flags[r], RGN_ERR_DENOM);
}
#endif
