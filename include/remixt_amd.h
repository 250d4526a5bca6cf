/*
 * remixt_amd.h -- C ABI of the MI355X-native ReMixT variational-HMM kernel.
 *
 * This is the drop-in boundary below the reference's Python object protocol.
 * The reference has no FFI on this path: `remixt/cn_model.py` talks to the
 * Cython class `remixt.bpmodel.RemixtModel` (reference remixt/bpmodel.pyx:397).
 * Every entry point below replaces one method / attribute of that class (cited
 * per function, paths relative to the reference root).  remixt_amd/bpmodel.py is
 * the ctypes binding that re-creates the `RemixtModel` protocol on top of it;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C: pointers + sizes, no C++/torch types.  All host arrays are
 *     C-contiguous float64 / int64 exactly as the reference passes them.
 *   - a `rmx_batch` holds ONE dataset (segments, state tables, topology) and R
 *     independent "restarts" (the reference's one-process-per-init_id fan-out,
 *     remixt/workflow.py:329-340).  The reference's RemixtModel == batch of 1.
 *   - every function returns an int status: 0 ok; RMX_E* otherwise, with a
 *     message retrievable through rmx_last_error().  RMX_EVALUE / RMX_EASSERT
 *     mirror the reference's ValueError / AssertionError sites.
 *   - restart ranges are [r0, r1).  All work is queued on the batch's HIP
 *     stream; functions that return host values synchronise that stream.
 *   - nothing is computed on the CPU: if no HIP device is usable the create
 *     call fails with RMX_EDEVICE (there is no fallback path).
 */
#ifndef REMIXT_AMD_H
#define REMIXT_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RMX_OK 0
#define RMX_EVALUE 1     /* reference: ValueError (bad shapes, nan ll, invalid p, x<=0 in digamma) */
#define RMX_EASSERT 2    /* reference: AssertionError (nan in alphas/betas/marginals, bpmodel.pyx:936-962) */
#define RMX_EDEVICE 3    /* HIP runtime failure / no device */
#define RMX_EUNSUPPORTED 4 /* outside the supported envelope (documented in DESIGN.md) */
#define RMX_EARG 5       /* bad argument to this C API */

#define RMX_MAX_CLONES 4

typedef struct rmx_batch rmx_batch;

/* Read-only problem description == positional arguments of
 * RemixtModel.__cinit__ (bpmodel.pyx:461-476), with the (N,S,M,2) state array
 * given in class-compressed form: segment n uses table cn_classes[seg_class[n]].
 * (cn_model.py:359-364 builds at most a handful of distinct tables: they differ
 * only in the normal-clone row.)  rmx_compress_cn_states() converts the dense
 * reference array. */
typedef struct rmx_problem {
    int32_t num_clones;            /* M (<= RMX_MAX_CLONES) */
    int32_t num_segments;          /* N */
    int32_t num_breakpoints;       /* K */
    int32_t num_cn_states;         /* S */
    int32_t num_brk_states;        /* B */
    int32_t num_classes;           /* C */
    int32_t normal_contamination;  /* bool */
    int32_t reserved;
    const int64_t *cn_classes;     /* [C][S][M][2] */
    const int32_t *seg_class;      /* [N] */
    const int64_t *brk_states;     /* [B][M] */
    const double *l;               /* [N] segment lengths */
    const double *x;               /* [N] total read counts */
    const double *y;               /* [N][2] allele read counts */
    const int64_t *is_telomere;    /* [N] */
    const int64_t *breakpoint_idx; /* [N] (-1 = none) */
    const int64_t *breakpoint_orient; /* [N] */
    double transition_penalty;     /* fabs() taken, bpmodel.pyx:534 */
} rmx_problem;

/* ids for rmx_set_param / rmx_get_param: the `cdef public` float attributes of
 * RemixtModel (bpmodel.pyx:433-454, 417-418, 422) */
enum rmx_param_id {
    RMX_P_NEGBIN_R_0 = 0, RMX_P_NEGBIN_R_1, RMX_P_NEGBIN_HDEL_MU, RMX_P_NEGBIN_HDEL_R_0, RMX_P_NEGBIN_HDEL_R_1,
    RMX_P_BETABIN_M_0, RMX_P_BETABIN_M_1, RMX_P_BETABIN_LOH_P, RMX_P_BETABIN_LOH_M_0, RMX_P_BETABIN_LOH_M_1,
    RMX_P_PRIOR_OUTLIER_TOTAL, RMX_P_PRIOR_OUTLIER_ALLELE, RMX_P_DIVERGENCE_WEIGHT,
    RMX_P_HMM_LOG_NORM_CONST /* read-only */, RMX_P_COUNT
};

/* ids for rmx_get_array / rmx_set_array: array attributes of RemixtModel
 * (bpmodel.pyx:405-442).  Shapes in the reference's layout. */
enum rmx_array_id {
    RMX_A_H = 0,                   /* f64 [M]            rw */
    RMX_A_P_BREAKPOINT,            /* f64 [K][B]         rw */
    RMX_A_P_ALLELE_SWAP,           /* f64 [N][2]         rw */
    RMX_A_P_OUTLIER_TOTAL,         /* f64 [N][2]         rw */
    RMX_A_P_OUTLIER_ALLELE,        /* f64 [N][2]         rw */
    RMX_A_POSTERIOR_MARGINALS,     /* f64 [N][S]         rw */
    RMX_A_FRAMELOGPROB,            /* f64 [N][S]         r  */
    RMX_A_TOTAL_LIKELIHOOD_MASK,   /* i64 [N]            rw (shared by the batch) */
    RMX_A_ALLELE_LIKELIHOOD_MASK,  /* i64 [N]            rw (shared by the batch) */
    RMX_A_LOG_TRANSMAT,            /* f64 [N-1][S][S]    r  materialised on request only */
    RMX_A_CACHED_LOG_TRANSMAT,     /* f64 [N-1][S][S]    r  materialised on request only */
    RMX_A_JOINT_POSTERIOR_MARGINALS, /* f64 [N-1][S][S]  r  materialised on request only */
    RMX_A_STATE_SEQUENCE,          /* i64 [N]            r  last Viterbi path */
    RMX_A_COUNT
};

/* -- lifetime ------------------------------------------------------------- */
/* RemixtModel.__cinit__ (bpmodel.pyx:461-604) for R restarts at once.
 * h_init: [R][M]; divergence_weight: [R] (fabs taken, :535). */
int rmx_batch_create(const rmx_problem *problem, int32_t num_restarts, const double *h_init,
                     const double *divergence_weight, int32_t device, rmx_batch **out);
int rmx_batch_destroy(rmx_batch *b);
/* Dense (N,S,M,2) int64 -> class-compressed form.  seg_class_out: [N];
 * classes_out: caller buffer for up to max_classes tables of S*M*2 int64.
 * Returns the number of classes through *num_classes (RMX_EUNSUPPORTED when
 * more than max_classes distinct tables occur). */
int rmx_compress_cn_states(const int64_t *cn_states, int32_t N, int32_t S, int32_t M,
                           int32_t max_classes, int32_t *seg_class_out, int64_t *classes_out,
                           int32_t *num_classes);
const char *rmx_last_error(void);
/* The restarts whose device-side checks (the reference's ValueError / AssertionError sites) fired in the calling thread's last
 * failing call: up to `cap` indices into out (out may be NULL with cap 0), returns their number.  Every flagged restart's
 * error state is cleared when the call reports, and rmx_last_error() describes the lowest one; a batched caller fails exactly
 * the listed restarts.  A failing call that flagged no restart (bad argument, device failure, unsupported shape) leaves the
 * list empty: it never describes an earlier call. */
int rmx_last_error_restarts(int32_t *out, int32_t cap);
/* use an externally owned HIP stream (e.g. torch's current stream); NULL = own */
int rmx_set_stream(rmx_batch *b, void *hip_stream);
int rmx_synchronize(rmx_batch *b);
/* derived sizes: 0 cn_max (bpmodel.pyx:489), 1 num chains, 2 num transition classes,
 * 3 num breakend segments, 4 padded row stride of [N][S] device arrays; 10 / 11 chains on the register-resident
 * forward-backward kernels / on the general one; 12 the forward-backward kernel the last update_p_cn launched for the
 * former (1 k_fbm: FP64 matrix cores at 4 restarts per workgroup, vector FMA at 2 / 1; 2 k_fbv: two-phase vector FMA, 3 k_fbk: weights from packed copy numbers, 4 k_fbq: matrix cores with
 * weights from 8-bit codes; 0: general kernel k_fb<0> only), 13 restarts per workgroup of that launch, 14 the lattice kernel of
 * the last decode (1 k_viterbi_reg, 2 k_viterbi_code, 3 k_viterbi, 4 k_viterbi_max, 5 k_viterbi_code_max, 6 k_viterbi_sad_max: above ~380 states); 18 workgroups per restart of that lattice, 19 the trace-back (1 parallel, 0 the sequential walk), 54 decodes repeated after a lattice cluster's watchdog ran out; 15 the largest number of restarts per workgroup of that launch (13 is the
 * smallest: k_fbm gives long chains fewer restarts per workgroup than short ones); 64 the largest number of total-copy classes of a state table,
 * 65 whether the cell cache keeps its read-depth planes per class (1) or per state (0; also without a cell cache) */
int rmx_info(rmx_batch *b, int32_t what, int64_t *out);
/* -- tuning options ------------------------------------------------------- */
/* Not part of the reference protocol: which of this library's equivalent kernels / launch shapes run.  Results do not
 * depend on them beyond rounding (tests/test_hip_*.py compare the alternatives); they exist so that tests can put a
 * small problem on the launch shape a large one gets, and for A/B measurements.  rmx_set_default_option applies to
 * batches created afterwards (process-wide); rmx_set_option to one batch (creation-time options: RMX_EARG). */
enum rmx_option_id {
    RMX_OPT_FB_KERNEL = 0,      /* forward-backward: 0 auto, 1 general single-vector kernel for every chain, 2 tabulated weights
                                   instead of on-the-fly weights for grids beyond the register-resident kernel (S > 176), 3 the two-phase
                                   vector kernels (k_fbv up to 176 states, k_fbk above) instead of k_fbm / k_fbq */
    RMX_OPT_FB_NV,              /* restarts advanced by one forward-backward workgroup: 0 auto (k_fbm: 4 on the matrix cores, or 2 / 1 on the
                                   vector ALU while that many workgroups fit the chip's 256 CUs at once), 1, 2, 4 (the shapes that exist) */
    RMX_OPT_FB_BREAKEND_CODES,  /* 1 (default): breakend steps from pair codes + clone-product tables; 0: per-clone distance tables */
    RMX_OPT_FUSE_SWEEPS,        /* 1 (default): marginals + indicator updates + next frame pass as one kernel between sweeps */
    RMX_OPT_TWO_STREAMS,        /* 1 (default): breakend branch of a sweep on a second stream next to the marginal pass */
    RMX_OPT_VITERBI_PLAIN,      /* decode: 0 (default) the reference's own formulation -- maxima forward, the lattice rows kept, arg-maxima recomputed in the
                                   trace-back (k_viterbi_max / k_viterbi_code_max + k_backtrace_max, k_viterbi_sad_max + k_backtrace_sad above ~380 states; round 5); 1 the table-reading lattice kernel with
                                   back-pointers (k_viterbi); 2 round 4's register / code-table lattices with back-pointers */
    RMX_OPT_SEARCH_MODE,        /* parameter searches: 5 (default since round 5) the four standard searches together in rounds the device drives: optimiser
                                   state on the device, a kernel pair per round, queued back to back (half the latency of the host-driven rounds);
                                   0 the same shared rounds driven from the host (the default until round 4);
                                   1 one parameter at a time, table-free (what the caller falls back to when rmx_param_search_multi answers RMX_EUNSUPPORTED);
                                   2 one parameter at a time with table rebuilds per candidate (the path of every non-standard parameter).
                                   No other value is accepted: 3, 4, 6 and 7 were experiments that lost their measurements and were taken out again */
    RMX_OPT_ELL_DENSE,          /* 1: sampled objectives over all states instead of the lists of states with posterior mass */
    RMX_OPT_STRIP,              /* 1 (default): strip kernels for the (segment x state) passes when 32 < S <= 384 */
    RMX_OPT_CELL_CACHE,         /* creation time, 1 (default): cache the six likelihood values of every cell */
    RMX_OPT_SPARSE_TRIAL,       /* creation time, 1 (default): keep per-segment lists of states with posterior mass */
    RMX_OPT_FB_DEBUG,           /* creation time, 1: cycle counters of the forward-backward kernel through rmx_info(20..) */
    RMX_OPT_PAIRWISE_KERNEL,    /* breakend pairwise reductions: 0 auto (above 200 states k_pairwise_sp: the state pairs above the posterior threshold; else k_pairwise_be2), 1 general kernel
                                   (k_pairwise), 2 the dense pair-code kernel (k_pairwise_be2), 3 k_pairwise_sp, 4 k_pairwise_sp with a block of one wave per adjacency */
    RMX_OPT_PACE_SWEEPS,        /* 1: rmx_variational_update reaches each sweep's forward-backward point only after the previous sweep's
                                   forward-backward launch has finished on the device, instead of queueing all its sweeps at once; for restart groups that share a GPU -- at 355 states two paced groups of 8
                                   make 144 EM iterations/s, free-running ones 118 */
    RMX_OPT_FB_WG_BUDGET,       /* workgroups a forward-backward launch may have side by side when the shapes of its chains are chosen (0: 256, one per CU
                                   of an MI355X): tests set a small number to put a small problem on the mixed shapes a genome gets */
    RMX_OPT_TRIAL_KERNEL,       /* M-step trial passes over the lists of states with posterior mass: 0 (default) cells laid out flat over the threads
                                   (k_trial_flat: a segmented sum in list order), 1 a quarter wave per segment (k_trial_sparse) */
    RMX_OPT_GRAD_KERNEL,        /* h M-step rounds (objective + gradient on the samples): 0 (default) the lane chains laid out flat over the threads
                                   (k_gradflat_round; the same per-segment sums to the bit), 1 half a wave per sampled segment with the final sums
                                   folded in (round 4's form), 2 half a wave per segment and the final sums as a kernel of their own */
    RMX_OPT_STREAM_POOL,        /* 1 (default): a batch's two streams come from a process-wide pool per device and return to it when the batch is destroyed
                                   (streams are never destroyed: which hardware queue a role gets is decided once per process); 0: created and destroyed per batch */
    RMX_OPT_VITERBI_CLUSTER,    /* lattice above 176 states (k_viterbi_sad_max, default transition model): 0 (default) 4 workgroups per restart up to 300 states, 8
                                   above, each a share of the target states, the rows exchanged through memory step by step (halved while restarts x
                                   workgroups > 64; one where the device already holds 192 such workgroups); 1 one workgroup per restart (up to ~380
                                   states that is round 5's code-table lattice k_viterbi_code_max); 2 / 4 / 8 that many; 102 / 104 / 108: a test of the clusters' watchdog (one member never
                                   publishes its first row: the waits run out and the decode is repeated with one workgroup per restart) */
    RMX_OPT_TRACEBACK,          /* trace-back of the kept lattice rows (default transition model): 0 (default) in parallel -- the first arg-maximum of every target
                                   state of every row on the whole chip (k_bp_all), then the walk as a composition of maps (k_chase_compose / _ends / _fill);
                                   1 the sequential walk on one wave per restart (k_backtrace_max / k_backtrace_sad) */
    RMX_OPT_LT_CLASSES,         /* creation time, 1 (default): the cell cache keeps the two read-depth planes per (segment, total-copy class) instead of per
                                   (segment, state) -- states of a table with the same total copy numbers share the value to the bit -- where a table has at
                                   most 128 such classes; 0: six planes per (segment, state).  Results are the same bits either way */
    RMX_OPT_COUNT
};
int rmx_set_default_option(int32_t option_id, int32_t value);
int rmx_set_option(rmx_batch *b, int32_t option_id, int32_t value);
int rmx_get_option(rmx_batch *b, int32_t option_id, int32_t *value);

/* -- attributes ----------------------------------------------------------- */
int rmx_set_param(rmx_batch *b, int32_t r, int32_t param_id, double value);
int rmx_get_param(rmx_batch *b, int32_t r, int32_t param_id, double *value);
int rmx_set_transition_model(rmx_batch *b, int32_t model);  /* bpmodel.pyx:456, 606-616 */
int rmx_set_array(rmx_batch *b, int32_t r, int32_t array_id, const void *host_src);
int rmx_get_array(rmx_batch *b, int32_t r, int32_t array_id, void *host_dst);
/* The attributes p_outlier_total / p_outlier_allele (bpmodel.pyx:419-421) of restarts [r0, r1) in one transfer into registered
 * host memory the batch owns: *total / *allele point to [r1 - r0][N][2] float64, valid until the next call.  The two copies are
 * queued IN ORDER on the batch's stream (behind everything already queued there) and the call returns when they have landed.  What BreakpointModel.get_param_sample_weight (cn_model.py:323-352) reads at the start of every M-step. */
int rmx_fetch_indicators(rmx_batch *b, int32_t r0, int32_t r1, const double **total, const double **allele);
/* read-only derived state tables, (N,S[,M]) int64 like the reference attributes
 * cn_states_total / num_alleles_subclonal / is_hdel / is_loh (bpmodel.pyx:497-507):
 * which = 0..3 in that order */
/* calculate_log_transmat(out) (bpmodel.pyx:639-684): dense (N-1) x S x S log transition array for the CURRENT
 * p_breakpoint of restart r into a host array of 8 (N-1) S^2 bytes; no model state changes. */
int rmx_calculate_log_transmat(rmx_batch *b, int32_t r, double *dst);
/* Host-only helper of the weighted M-step sampling (cn_model.py:475-480 with p = weights): the index every
 * uniform draw u[j] selects from cumsum(p) / sum -- numpy's cumsum / searchsorted(side='right') with the same
 * accumulation order; *positive = count_nonzero(p > 0).  Runs without the GIL, no device involved. */
int rmx_weighted_search(const double *p, int64_t n, const double *u, int32_t k, int64_t *out, int64_t *positive);
/* One round of that sampling without a normalised copy of the weights (host only, no GIL, no device): weights w[i * stride] / norm
 * (a column of the (N, 2) outlier indicators the sample of negbin_r_* / betabin_M_* is weighted with, cn_model.py:323-352); the k
 * uniform draws u pick indices from the cumulative sum as rmx_weighted_search does; indices not yet in found[0 .. *nfound) are
 * appended in the order of the draws, up to cap (numpy's unique-by-first-occurrence of the concatenation).  *positive = number of
 * positive weights (fewer than the sample size: numpy's "Fewer non-zero entries in p than size"). */
int rmx_weighted_sample_round(const double *w, int64_t n, int64_t stride, double norm, const double *u, int32_t k,
                              int64_t *found, int32_t *nfound, int32_t cap, int64_t *positive);
int rmx_get_state_table(rmx_batch *b, int32_t which, int64_t *host_dst);

/* -- coordinate updates (bpmodel.pyx cpdef methods), restarts [r0,r1) ------ */
int rmx_update_framelogprob(rmx_batch *b, int32_t r0, int32_t r1);      /* :898-919 */
int rmx_update_p_cn(rmx_batch *b, int32_t r0, int32_t r1);              /* :921-962 */
int rmx_update_p_breakpoint(rmx_batch *b, int32_t r0, int32_t r1);      /* :964-985 */
int rmx_update_p_outlier_total(rmx_batch *b, int32_t r0, int32_t r1);   /* :987-1003 */
int rmx_update_p_outlier_allele(rmx_batch *b, int32_t r0, int32_t r1);  /* :1005-1023 */
int rmx_update_p_allele_swap(rmx_batch *b, int32_t r0, int32_t r1);     /* :1025-1042 */
/* the five updates in BreakpointModel.variational_update order (cn_model.py:444-460),
 * `iters` times, without host round trips */
int rmx_variational_update(rmx_batch *b, int32_t r0, int32_t r1, int32_t iters);

/* -- objectives ----------------------------------------------------------- */
/* out: [r1-r0] */
int rmx_calculate_elbo(rmx_batch *b, int32_t r0, int32_t r1, double *elbo_out);       /* :1119-1123 */
/* calculate_elbo in two halves (round 5): _begin queues the ELBO of restarts [r0, r1) on the batch's stream -- kernels and the copy of the
 * results -- and returns without waiting; _end waits for it and returns the values (and raises what rmx_calculate_elbo would have).  The
 * batched EM driver queues the next iteration's sweeps in between: the value is only recorded (cn_model.py:420-428), nothing waits for it. */
int rmx_calculate_elbo_begin(rmx_batch *b, int32_t r0, int32_t r1);
int rmx_calculate_elbo_end(rmx_batch *b, double *elbo_out);
int rmx_calculate_variational_energy(rmx_batch *b, int32_t r0, int32_t r1, double *out);  /* :1060-1117 */
int rmx_calculate_variational_entropy(rmx_batch *b, int32_t r0, int32_t r1, double *out); /* :1044-1058 */
/* sample: int64 [N] 0/1 mask as in the reference (:1125, :1159); partial_h_out may be
 * NULL; when given it receives [M] (:1159-1195). */
int rmx_expected_log_likelihood(rmx_batch *b, int32_t r, const int64_t *sample, double *ell_out,
                                double *partial_h_out);
/* The M-steps of BreakpointModel (cn_model.py:482-569) evaluate the objective hundreds of times on
 * one fixed sample: rmx_set_sample uploads the mask once; rmx_expected_log_likelihood with
 * sample == NULL then re-uses it. */
int rmx_set_sample(rmx_batch *b, int32_t r, const int64_t *sample);
/* E[ll] on the current sample for G values of one likelihood parameter (the grid stage of
 * scipy.optimize.brute, cn_model.py:553-558) with one host round trip; G <= 64.  Leaves the
 * parameter at values[G-1], as G sequential evaluations would. */
int rmx_expected_ll_param_grid(rmx_batch *b, int32_t r, int32_t param_id, const double *values, int32_t G, double *out);
/* Lock-step M-steps over several restarts (remixt_amd/restarts.py): one candidate value of one
 * likelihood parameter per listed restart (distinct restarts), each evaluated on its own current
 * sample; out[i] belongs to restarts[i].  One host round trip for the whole list. */
int rmx_expected_ll_batch(rmx_batch *b, int32_t nreq, const int32_t *restarts, int32_t param_id, const double *values, double *out);
/* The whole scipy.optimize.brute search of BreakpointModel.update_param (cn_model.py:553-561) for one
 * likelihood parameter of every listed restart, in lock step: G grid values (np.mgrid[lo:hi:G*1j]),
 * first arg-min, then scipy.optimize.fmin (Nelder-Mead) restated as a host state machine; every
 * round of objective evaluations is one rmx_expected_ll_batch.  nll is +inf outside [lo, hi]
 * (cn_model.py:542-543).  xopt[i] = the optimiser's result for restarts[i]; the parameter is left at
 * the value of the restart's last evaluation, as the sequential scipy run leaves it. */
int rmx_param_search(rmx_batch *b, int32_t nreq, const int32_t *restarts, int32_t param_id, double lo, double hi,
                     const double *grid, int32_t G, double *xopt);
/* The four standard searches of every listed restart in the same evaluation rounds (they move disjoint
 * likelihood components and do not write to the model while searching, cn_model.py:533-561 x 4):
 * param_ids [nparams] a subset of negbin_r_0/1, betabin_M_0/1; slot j = position in param_ids, its
 * samples given by rmx_set_sample_slot; lo / hi [nparams]; grids [nparams][G]; xopt / lastval
 * [nparams][nreq] = optimiser result and last evaluated point (the state the acceptance test of
 * cn_model.py:563-569 looks at).  The model is not modified.  RMX_EUNSUPPORTED: use rmx_param_search. */
int rmx_set_sample_slot(rmx_batch *b, int32_t r, int32_t slot, const int64_t *sample);
/* The M-step samples (cn_model.py:475-480) of several restarts in one call and one device transfer: list i
 * is the ascending segment indices indices[offsets[i] .. offsets[i+1]) of restart restarts[i]; slots[i] = -1:
 * the restart's current sample (as rmx_set_sample), 0..3: its parameter slot (as rmx_set_sample_slot). */
int rmx_set_sample_lists(rmx_batch *b, int32_t nlists, const int32_t *restarts, const int32_t *slots,
                         const int32_t *offsets, const int32_t *indices);
int rmx_param_search_multi(rmx_batch *b, int32_t nreq, const int32_t *restarts, int32_t nparams,
                           const int32_t *param_ids, const double *lo, const double *hi,
                           const double *grids, int32_t G, double *xopt, double *lastval);
/* Lock-step h M-step (BreakpointModel.update_h, cn_model.py:482-531): one candidate haploid-depth
 * vector h[i][0..M) per listed restart; out[i][0] = E[ll] (calculate_expected_log_likelihood,
 * bpmodel.pyx:1125-1157) and out[i][1..M] = dE[ll]/dh (calculate_expected_log_likelihood_partial_h,
 * bpmodel.pyx:1159-1195) on restart i's current sample; out is [nreq][1 + RMX_MAX_CLONES].  Leaves
 * h[i] set on the restart, as `model.h = h` followed by the two calls would. */
int rmx_expected_ll_h_batch(rmx_batch *b, int32_t nreq, const int32_t *restarts, const double *h, double *out);
/* E[ll] over ALL segments (the reference passes a mask of ones, cn_model.py:497, :524, :549, :563)
 * for restarts [r0, r1); out: [r1-r0]. */
int rmx_expected_ll_full(rmx_batch *b, int32_t r0, int32_t r1, double *out);
/* The M-step's accept test (`ell_after < ell_before`, cn_model.py:497-505, 563-569) without committing the
 * tried values: full-data E[ll] at the current (changed) h / parameters, evaluated into scratch
 * per-segment expectations -- same numbers as rmx_expected_ll_full -- leaving the restart's own
 * expectations, cell cache and staleness flags untouched.  rmx_trial_rollback then puts the previous
 * value back (param_id >= 0: likelihood parameter, values[0]; param_id < 0: h, values[0..M)) and declares
 * the untouched expectations current again, so a rejected update costs no second pass over the cells.
 * Valid only in the sequence rmx_expected_ll_full -> sampled evaluations -> rmx_expected_ll_full_trial ->
 * accept (set the new value) | rmx_trial_rollback. */
int rmx_expected_ll_full_trial(rmx_batch *b, int32_t r0, int32_t r1, double *out);
int rmx_trial_rollback(rmx_batch *b, int32_t r, int32_t param_id, const double *values);
/* The full-data E[ll] split into the four likelihood components that negbin_r_0, negbin_r_1, betabin_M_0 and
 * betabin_M_1 move (out [r1-r0][4]; their sum is rmx_expected_ll_full up to rounding): trial = 0 at the committed values,
 * trial = 1 with the changed parameters on trial (as rmx_expected_ll_full_trial).  The accept tests of the four
 * parameters (cn_model.py:563-569, one update_param after the other) then take ONE pass over the cells: E[ll] with
 * parameter j on trial and the earlier ones decided is a sum of component values of the two calls.  Afterwards, per
 * parameter: rmx_set_param (accept) or rmx_trial_rollback (reject; only that parameter's components become current again).
 * trial = 2: the component sums of the expectations the LAST trial pass over this range left in scratch (rmx_expected_ll_full_trial or
 * trial = 1), without another pass: right after the h M-step's accept test they are E[ll] at (accepted h, committed parameters),
 * i.e. the "before" of the parameter accept tests, for every restart whose h was accepted (restarts whose h was rolled back: trial = 0,
 * which costs no pass either).  A restart's own expectations then stay stale until the next ELBO / sweep: ONE full refresh per EM
 * iteration instead of one after the h M-step and one after the parameter M-steps.
 * trial = 3: the same per restart, for a range the last rmx_expected_ll_full_trial covered: the scratch sums for the restarts whose own
 * expectations are stale (h kept), the sums of their own expectations for the others (rolled back, or untouched) -- the mixed outcome
 * of a batch's h accept tests without a refresh pass; RMX_EUNSUPPORTED if that trial pass is not the last one over the range. */
int rmx_expected_ll_components(rmx_batch *b, int32_t r0, int32_t r1, int32_t trial, double *out);
/* per-cell values, for tests (:751-776, :809-853): u/v/w in {0,1} */
int rmx_log_likelihood_total(rmx_batch *b, int32_t r, int32_t n, int32_t s, int32_t u, double *out);
int rmx_log_likelihood_allele(rmx_batch *b, int32_t r, int32_t n, int32_t s, int32_t v, int32_t w, double *out);

/* The other per-cell cpdef methods of RemixtModel for segment n, state s (no caller in cn_model.py; part of the protocol):
 * which = 0 calculate_expected_total_reads (bpmodel.pyx:686-698) -> out[0]
 *         1 calculate_expected_total_reads_partial_h (:700-708) -> out[0..M)
 *         2 calculate_expected_allele_ratio (:710-725) -> out[0]     (RMX_EVALUE: total_depth <= 0)
 *         3 calculate_expected_allele_ratio_partial_h (:727-745) -> out[0..M)
 *         4 calculate_log_prior_cn (:747-750) -> out[0]
 *         5 calculate_log_likelihood_total_partial_h (:778-807), outlier state u -> out[0..M)
 *         6 calculate_log_likelihood_allele_partial_h (:855-896), outlier state v, allele w -> out[0..M)
 * out must hold RMX_MAX_CLONES doubles. */
int rmx_cell_quantity(rmx_batch *b, int32_t r, int32_t n, int32_t s, int32_t which, int32_t u, int32_t v, int32_t w, double *out);

/* -- decoding ------------------------------------------------------------- */
/* infer_cn (:1197-1210): Viterbi over the framelogprob / log_transmat of the last
 * update_p_cn; cn_out int64 [N][M][2]; logprob_out may be NULL */
int rmx_infer_cn(rmx_batch *b, int32_t r, int64_t *cn_out, double *logprob_out);
/* the same for restarts r0 .. r0+nr-1 with their lattices running side by side: cn_out int64
 * [nr][N][M][2], logprob_out [nr] or NULL (the per-restart decode of analysis/pipeline.py:196-206) */
int rmx_infer_cn_batch(rmx_batch *b, int32_t r0, int32_t nr, int64_t *cn_out, double *logprob_out);

/* -- posterior sampling (no reference counterpart) -------------------------- */
/* num_samples whole copy-number paths per restart r0 .. r0+nr-1 from the structured posterior q(c) of the last
 * update_p_cn: the chain HMM of its framelogprob / log_transmat snapshot, the one infer_cn decodes and whose marginals
 * are posterior_marginals.  states_out int16 [nr][num_samples][N]: indices into the segment's state table.  seeds
 * [nr]: the stream of restart r0+i; a (seed, sample index) pair gives the same path in any call.  The model is not
 * modified.  RMX_EVALUE (flagged restarts) before a restart's first update_p_cn; RMX_EASSERT (flagged) when a step
 * has no finite positive weight. */
int rmx_sample_cn(rmx_batch *b, int32_t r0, int32_t nr, int32_t num_samples, const uint64_t *seeds, int16_t *states_out);

/* -- posterior summaries (no reference counterpart) -------------------------- */
/* Linear functionals and row statistics of the attribute posterior_marginals of restarts r0 .. r0+nr-1, exactly as
 * rmx_get_array would return it for each of them (whatever the last sweep or an rmx_set_array left there: there is no
 * validity state), computed on the device in one read of it.  The model is not modified.
 *   weights   [C][S][Q] one table per state class (C = num_classes of the problem), 1 <= Q <= 256; or NULL with Q = 0
 *   states    int16 [nr][N] a state per segment (e.g. a decoded path), each in [0, S); or NULL
 *   proj_out  [nr][N][Q]: sum over s < S of post[n][s] * weights[seg_class[n]][s][q]; or NULL
 *   stats_out [nr][N][3]: the row maximum, the entropy -sum_{post > 0} post log(post), post[n][states[n]] (0 without
 *             states); or NULL
 *   argmax_out int16 [nr][N]: the first index of the row maximum (numpy.argmax); or NULL
 * A restart's outputs are bit-identical in any [r0, r0+nr) range that holds it.  RMX_EARG, with nothing launched: a bad
 * range, all outputs NULL, proj_out without weights, Q out of range, a states entry outside [0, S). */
int rmx_posterior_summary(rmx_batch *b, int32_t r0, int32_t nr, int32_t Q, const double *weights, const int16_t *states,
                          double *proj_out, double *stats_out, int16_t *argmax_out);

/* -- region event probabilities (no reference counterpart) ------------------- */
/* log-probabilities, under the structured posterior of the last update_p_cn, of path events over runs of model segments
 * of restarts r0 .. r0+nr-1.  Query i = queries[i][0..3] = (first segment a, last segment b, mask index or
 * -1, label index or -1) asks for log P(c_n in mask at every n in [a, b] with constrain[n] != 0, and
 * label(c_n) == label(c_n+1) at every adjacency inside [a, b]).  The model is not modified.
 *   queries   int32 [nq][4]; a <= b, both in [0, N) and in the same chain
 *   masks     uint8 [C][nmask][S], non-zero = allowed state, one table per state class; NULL with nmask = 0
 *   labels    int16 [C][nlabel][S], one table per state class; NULL with nlabel = 0
 *   constrain uint8 [N]: whether a mask binds at the segment; NULL = everywhere
 *   logp_out  [nr][nq]; -inf for an impossible event
 * A (restart, query) result is bit-identical in any restart range and any batch of queries.  RMX_EARG, with nothing
 * launched: a bad range, a query with a > b, an end outside [0, N), ends in different chains, a mask or label index out
 * of range.  RMX_EVALUE with the restarts listed by rmx_last_error_restarts: a restart has had no update_p_cn.
 * RMX_EASSERT with the restarts listed: a backward step met a zero or non-finite normaliser under positive mass (that
 * query's result is NaN).  RMX_EUNSUPPORTED: more than 1024 states. */
int rmx_region_prob(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, const uint8_t *masks,
                    int32_t nlabel, const int16_t *labels, const uint8_t *constrain, double *logp_out);

/* -- region change counts (no reference counterpart) -------------------------- */
/* log-probabilities of the number of label changes over runs of model segments.  Queries, tables and
 * constrain are those of rmx_region_prob, but every query names a label (index >= 0).  With C = the number of adjacencies
 * n in [a, b-1] with label(c_n) != label(c_n+1), bin k of query i is
 *   log P(c_n in mask at every n in [a, b] with constrain[n] != 0, and C == k),   k = 0 .. nbins-1,
 * the last bin meaning C >= nbins-1.  Changes are counted between consecutive MODEL segments: a zero-length segment
 * inserted at a shared boundary that takes a third state contributes two.  The model is not modified.
 *   nbins     1 .. 16
 *   logp_out  [nr][nq][nbins]; -inf for a bin that cannot happen, and for a bin below about 1e-308 of the query's total
 *             (one scale carries all bins of a step)
 * A (restart, query) result is bit-identical in any restart range and any batch of queries.  Errors as rmx_region_prob,
 * and RMX_EARG with nothing launched for nbins outside [1, 16] or a query whose label index is negative.
 * RMX_EASSERT: every bin of the failing query is NaN.  RMX_EUNSUPPORTED: more than 1024 states (the bound of the
 * kernel's LDS plan: 142 bytes per state rounded up to 16 states). */
int rmx_region_counts(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, const uint8_t *masks,
                      int32_t nlabel, const int16_t *labels, const uint8_t *constrain, int32_t nbins, double *logp_out);

/* -- region extremes (no reference counterpart) -------------------------------- */
/* log-probabilities that a per-state integer level stays at or below each of ncol nested thresholds over runs of model
 * segments: the CDF of a region's peak copy number, or, with a reflected level table, of its lowest.
 * Queries, masks and constrain are those of rmx_region_prob, but field 3 of a query is a level index (>= 0) and there is no
 * label constraint.  Column j of query i is
 *   log P(c_n in mask and level(c_n) <= j at every n in [a, b] with constrain[n] != 0),   j = 0 .. ncol-1;
 * a state whose level is ncol or more is in no column, and neither mask nor level binds where constrain[n] is 0.  In
 * real arithmetic the columns do not decrease in j.  One walk of the run serves every column.  The model is not modified.
 *   levels    int16 [C][nlevel][S], every entry >= 0, one table per state class
 *   ncol      1 .. 16
 *   logp_out  [nr][nq][ncol]; -inf for a column that cannot happen.  Every column carries its own scale: a column is
 *             not lost below 1e-308 of another (rmx_region_counts' bins are)
 * A (restart, query) result is bit-identical in any restart range and any batch of queries.  Errors as rmx_region_prob,
 * and RMX_EARG with nothing launched for ncol outside [1, 16], a level index outside [0, nlevel) or a negative level
 * entry.  RMX_EASSERT: every column of the failing query is NaN.  RMX_EUNSUPPORTED: more than 1024 states (the bound of
 * the kernel's LDS plan: 140 bytes per state rounded up to 16 states). */
int rmx_region_extremes(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, const uint8_t *masks,
                        int32_t nlevel, const int16_t *levels, const uint8_t *constrain, int32_t ncol, double *logp_out);

/* -- restart overlap (no reference counterpart) -------------------------------- */
/* The exact overlap of two restarts' structured posteriors q_A, q_B of their last update_p_cn over runs of model segments
 * (DESIGN 4.19).  Both are the Markov chains the reference's forward-backward pass defines (remixt/bpmodel.pyx:1213-1246:
 * alphas, betas and the pairwise posterior of neighbouring segments), so for a run [first, last] of one chain
 *   Z = sum_x q_A(x_first .. x_last)^lam * q_B(pi x_first .. pi x_last)^mu
 * is one backward recursion over the run.  mode 0: (lam, mu) = (1/2, 1/2), Z is the Bhattacharyya coefficient BC <= 1
 * (squared Hellinger distance 1 - BC, Bhattacharyya distance -log BC); mode 1: (1, 1), Z is the probability that independent
 * draws of the two posteriors coincide on the run (A = B: the collision probability; 1 / Z its effective number of
 * configurations).  pi maps a state index of A to the state index of B it is compared with, per state class.
 *   batch_a, batch_b  the batches of the A and the B side; batch_b may be batch_a.  Two batches must describe the same problem
 *             on the same device (segments, states, classes, clones, transition classes, breakend slots, penalty and current
 *             transition model); the call runs on batch_a's stream behind what batch_b's stream holds when it is made, and
 *             neither batch may be updated while it runs
 *   pairs     int32 [npairs][2]: restart of batch_a, restart of batch_b
 *   queries   int32 [nq][4]: first segment, last segment (of one chain), permutation index, 0
 *   perms     int16 [nperm][C][S]: every row a bijection of [0, S)
 *   logz_out  [npairs][nq]: log Z; -inf where the two posteriors share no configuration
 * A (pair, query) result is bit-identical in any list of pairs, any batch of queries and any chunking.  The models are not
 * modified.  RMX_EARG, with nothing launched: a pair index out of range, a query that crosses a chain end, a permutation index
 * out of range, a permutation row that is not a bijection, a mode other than 0 or 1, batches of different problems or devices.
 * RMX_EVALUE, with nothing launched: a restart without update_p_cn (rmx_last_error_restarts lists them), or a pair whose two
 * snapshots were taken under different transition models (the message names the pair).  RMX_EASSERT: a backward step had a
 * zero or non-finite normaliser; the failing results are NaN and the message names the first such pair.  RMX_EUNSUPPORTED:
 * more than 1024 states. */
int rmx_restart_overlap(rmx_batch *batch_a, rmx_batch *batch_b, int32_t npairs, const int32_t *pairs, int32_t nq, const int32_t *queries,
                        int32_t nperm, const int16_t *perms, int32_t mode, double *logz_out);

/* -- call probabilities (no reference counterpart) ---------------------------- */
/* log-probabilities that the copy-number path agrees with a reference path over runs of model segments, under the
 * structured posterior q of the last update_p_cn of restarts r0 .. r0+nr-1.  Query i = (a, b, label index or
 * -1, path index) over the model segments [a, b] of one chain, with ref = path `path index` of the restart:
 *   logp_out[r][i] = log P(label(c_n) == label(ref_n) at every n in [a, b] with constrain[n] != 0),
 * the label table being the one of n's state class; label -1 asks for c_n == ref_n.  There is no adjacency constraint.
 * A whole chain with label -1 gives log q of that chain's part of the path.  The model is not modified.
 *   paths     int16 [nr][npaths][N], state indices in [0, S) into each segment's class table (every entry is
 *             checked, the ones no query reads included); staged whole: keeping a call small is the caller's job
 *   queries   int32 [nq][4]; a <= b, both in [0, N) and in the same chain; nq = 0 is valid and does nothing
 *   labels    int16 [C][nlabel][S], one table per state class; NULL with nlabel = 0
 *   constrain uint8 [N]: whether the event binds at the segment; NULL = everywhere
 *   logp_out  [nr][nq]; -inf for an impossible event -- and for a reference state whose forward entry underflowed to 0
 *             in the sweep's scaled rows, where the true probability is merely tiny
 * A (restart, query) result is bit-identical in any restart range, any batch of queries and any number of paths.
 * RMX_EARG, with nothing launched and logp_out untouched: a bad range, npaths < 1, nq < 0, a query with a > b, an end
 * outside [0, N), ends in different chains, a label or path index out of range, a path entry outside [0, S).
 * RMX_EVALUE with the restarts listed by rmx_last_error_restarts: a restart has had no update_p_cn.  RMX_EASSERT with
 * the restarts listed: a backward step met a zero or non-finite normaliser under positive mass, or a sum that is not a
 * finite number >= 0 (that query's result is NaN).  RMX_EUNSUPPORTED: more than 1024 states. */
int rmx_call_prob(rmx_batch *b, int32_t r0, int32_t nr, int32_t npaths, const int16_t *paths, int32_t nq, const int32_t *queries,
                  int32_t nlabel, const int16_t *labels, const uint8_t *constrain, double *logp_out);

/* Region moments: the exact mean and covariance, under the structured posterior of the last update_p_cn, of weighted sums
 * of state features over runs of segments: F_f = sum_{n in [first, last]} w[n] phi_f(c_n) for the nf features f0 .. f0+nf-1 of
 * a query.  It complements rmx_posterior_summary, whose per-segment means and SDs do not combine over a region because
 * neighbouring segments are correlated, and rmx_sample_cn, which gives the same numbers to 1 / sqrt(samples): this is what
 * puts an exact error bar on ploidy, on the mean copy number of an arm or on the fraction of a region in LOH.
 *   queries   int32 [nq][4]: first, last (as rmx_region_prob), f0 in [0, nfeat - nf], weight vector in [0, nw)
 *   features  double [C][nfeat][S], one table per state class; weights double [nw][N]; all finite
 *   nf        features per query, 1 .. 4 (the same for every query of a call)
 *   out       [nr][nq][nf + nf (nf + 1) / 2]: E[F_f] for f = 0 .. nf-1, then Cov(F_f, F_g) for f <= g in row-major order of the
 *             upper triangle
 * A (restart, query) result is bit-identical in any restart range and any batch of queries, and a feature's mean and
 * variance do not depend on the other features of its query.
 * RMX_EARG, with nothing launched and out untouched: a bad range, nq < 1, nf outside [1, 4] or above nfeat, nw < 1, a NULL
 * table, a feature or weight that is not finite, a query as for rmx_region_prob, f0 or the weight index out of range.
 * RMX_EVALUE with the restarts listed: a restart has had no update_p_cn.  RMX_EASSERT with the restarts listed: a backward
 * step met a zero or non-finite normaliser under non-zero mass, or an output is not finite (every output of that query is
 * NaN).  RMX_EUNSUPPORTED: more than 1024 states. */
int rmx_region_moments(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nfeat, const double *features,
                       int32_t nw, const double *weights, int32_t nf, double *out);

/* Region event extents: where an event of rmx_region_prob begins and ends around an anchor segment.  Query i =
 * (anchor n0, mask index or -1, label index or -1, 0); with the event E of rmx_region_prob (c_n in the mask at every n with
 * constrain[n] != 0, equal labels across every adjacency), slot k of a query stands for model segment n = n0 - wl + k:
 *   logp_out[r][i][k] = log P(E on [min(n, n0), max(n, n0)]),   k = 0 .. wl + wr.
 * Slot wl is log P(E on [n0, n0]): the logarithm of the masked sum of the anchor's marginal, 0 without a mask or where
 * constrain[n0] is 0.  A slot whose segment lies outside the anchor's chain or outside [0, N) is -inf (a run cannot pass a
 * chain end), as is an impossible event -- and a slot to the right of the anchor whose probability lies below the range of a double
 * (log P under about -750) may come out as -inf as well.  Both halves are survival curves: they do not increase away from the anchor.  The
 * whole row costs wl + wr steps, against one rmx_region_prob query per slot.  The model is not modified.
 *   masks, labels, constrain   as rmx_region_prob
 *   wl, wr    window widths to the left and right of the anchor, >= 0, wl + wr + 1 <= 4096
 * A (restart, query) slot is bit-identical in any restart range, any batch of queries and any (wl, wr) that covers it.
 * RMX_EARG, with nothing launched and logp_out untouched: a bad range, nq < 1, an anchor outside [0, N), a mask or label
 * index out of range, a non-zero fourth field, wl or wr < 0, wl + wr + 1 > 4096.  RMX_EVALUE with the restarts listed: a
 * restart has had no update_p_cn.  RMX_EASSERT with the restarts listed: a step met a zero or non-finite normaliser under a
 * non-zero numerator, or a step sum that is not a finite number >= 0 (every slot of that query is NaN).
 * RMX_EUNSUPPORTED: more than 1024 states. */
int rmx_region_extent(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, const uint8_t *masks,
                      int32_t nlabel, const int16_t *labels, const uint8_t *constrain, int32_t wl, int32_t wr, double *logp_out);

/* Region conditionals: the marginal of every segment of a window given that an event of rmx_region_prob holds over an evidence
 * run inside it -- "suppose it is so: what follows?".  The structured posterior is the Markov chain of the
 * reference's forward-backward pass (remixt/bpmodel.pyx:1213-1246: alphas, betas and the pairwise posterior of neighbouring
 * segments; the reference itself only reads the unconditional marginals off it), so c_n separates the two sides of n and
 *   q(c_n = s | E) = P(E on [a, n] | c_n = s) * q(c_n = s, E on [n, b]) / P(E)
 * at every n of the chain, from one walk per direction.  Query i = (a, b, mask index or -1, label index or -1) is the evidence
 * run with the event E of rmx_region_prob; windows[i] = (lo, hi), lo <= a, b <= hi, all of one chain, names the segments that
 * come back.  Slot k of a query stands for model segment lo + k and holds Q + 3 doubles:
 *   out[r][i][k][q]     = sum_s q(c_n = s | E) * weights[seg_class[n]][s][q],   q < Q   (weights [C][S][Q], as rmx_posterior_summary)
 *   out[r][i][k][Q]     = max_s q(c_n = s | E)
 *   out[r][i][k][Q + 1] = the first index of that maximum, as a double
 *   out[r][i][k][Q + 2] = q(c_n = states[r][n] | E), 0 where states is NULL (states [nr][N], indices into the segment's class table)
 * and logp_out[r][i] = log P(E).  Slots past hi are NaN.  An impossible event gives logp_out = -inf and NaN in every slot of the
 * query; it is no error.  Without mask and label the slots are rmx_posterior_summary's.  The model is not modified.
 *   masks, labels, constrain   as rmx_region_prob
 *   nslot     slots per query: the longest window or more, <= 16384; an evidence run holds at most 4096 segments
 *   Q         1 .. 64
 * A (restart, query) slot is bit-identical in any restart range, any batch of queries, any chunking and any window that covers
 * it.  A call is split into chunks of (restart, query) pairs whose outputs fit 64 MiB of staging and whose evidence rows fit a
 * 256 MiB device workspace ((longest run) * S doubles per pair); both buffers stay with the batch and only grow.
 * RMX_EARG, with nothing launched and both outputs untouched: a bad range, nq < 1, a missing pointer, Q outside [1, 64], nslot
 * outside [1, 16384], a run or window outside [0, N) or out of order, a window that does not cover its run, crosses a chain end
 * or is longer than nslot, a run longer than 4096, a mask or label index out of range, a state index outside [0, S).
 * RMX_EVALUE with the restarts listed: a restart has had no update_p_cn.  RMX_EASSERT with the restarts listed: a step met a
 * zero or non-finite normaliser, or a sum that is not a finite number >= 0 (logp_out and every slot of that query are NaN).
 * RMX_EUNSUPPORTED: more than 1024 states. */
int rmx_region_conditional(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, const int32_t *windows, int32_t nslot,
                           int32_t nmask, const uint8_t *masks, int32_t nlabel, const int16_t *labels, const uint8_t *constrain, int32_t Q,
                           const double *weights, const int16_t *states, double *logp_out, double *out);

/* Region event spans: the joint law of where an event of rmx_region_prob begins and ends around an anchor segment, and so of
 * its length.  Query i = (anchor n0, mask index or -1, label index or -1, 0); with the event E of rmx_region_prob,
 *   logp_out[r][i][a][c] = log P(E on [n0 - a, n0 + c]),   a = 0 .. wl,   c = 0 .. wr.
 * Entry (0, 0) is the event at the anchor alone; row 0 is the right half of rmx_region_extent and column 0 its left half,
 * mirrored.  An entry whose interval leaves the anchor's chain or [0, N) is -inf (a run cannot pass a chain end), as is an
 * impossible event.  The table does not increase in a or in c.  The model is not modified.
 *   masks, labels, constrain   as rmx_region_prob
 *   wl, wr    window widths to the left and right of the anchor, >= 0, (wl + 1) (wr + 1) <= 16384
 * An entry is bit-identical in any restart range, any batch of queries and any (wl, wr) that covers it.
 * RMX_EARG, with nothing launched and logp_out untouched: a bad range, nq < 1, an anchor outside [0, N), a mask or label
 * index out of range, a non-zero fourth field, wl or wr < 0, (wl + 1) (wr + 1) > 16384.  RMX_EVALUE with the restarts listed: a
 * restart has had no update_p_cn.  RMX_EASSERT with the restarts listed: a backward step met a zero or non-finite
 * normaliser under a column with mass, or a column sum that is not a finite number >= 0 (every entry of that query is NaN).
 * RMX_EUNSUPPORTED: more than 1024 states. */
int rmx_region_span(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, const uint8_t *masks,
                    int32_t nlabel, const int16_t *labels, const uint8_t *constrain, int32_t wl, int32_t wr, double *logp_out);

/* Region event patterns: the joint probability of several events of rmx_region_prob along one chain -- a rearrangement's
 * two breakends, a focal event with its flanks, co-occurrence of two events on one chromosome.  Query i =
 * (first piece p0, piece count np, 0, 0) names the pieces pieces[p0 .. p0+np-1]; piece j = (a, b, mask index or -1, label
 * index or -1) is the event E_j of rmx_region_prob over the model segments [a, b]: c_n in the mask at every n of [a, b] with
 * constrain[n] != 0, and equal labels across every adjacency inside [a, b].
 *   logp_out[r][i] = log P(E_p0 and ... and E_p0+np-1).
 * Nothing binds at a segment in a gap between two pieces, and nothing binds at the adjacency between two pieces, even where
 * they touch (b_j + 1 == a_j+1): a focal pattern may change state at the region's edges.  The model is not modified.
 *   queries   int32 [nq][4]; the pieces of a query ascending and pairwise disjoint (b_j < a_j+1), all in one chain;
 *             different queries may share pieces
 *   pieces    int32 [npieces][4], 1 <= npieces <= 4194304 (staged whole per call: 64 MiB at the cap)
 *   masks, labels, constrain   as rmx_region_prob
 *   logp_out  [nr][nq]; -inf for an impossible event
 * A (restart, query) result is bit-identical in any restart range, in any batch of queries and for any placement of its
 * pieces inside the pieces array.
 * RMX_EARG, with nothing launched and logp_out untouched: a bad restart range, nq < 1, np < 1, p0 / np outside the array,
 * non-zero third or fourth query fields, a piece with a > b or an end outside [0, N), pieces of a query that are out of
 * order or overlap, pieces of a query in different chains, a mask or label index out of range, npieces < 1 or above the
 * cap.  RMX_EVALUE with the restarts listed by rmx_last_error_restarts: a restart has had no update_p_cn.  RMX_EASSERT
 * with the restarts listed: a backward step met a zero or non-finite normaliser under positive mass, or a sum that is not
 * a finite number >= 0 (that query's result is NaN).  RMX_EUNSUPPORTED: more than 1024 states. */
int rmx_region_pattern(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t npieces, const int32_t *pieces,
                       int32_t nmask, const uint8_t *masks, int32_t nlabel, const int16_t *labels, const uint8_t *constrain, double *logp_out);

/* Region decode: the most probable copy-number configuration of a region, and its probability.  Queries,
 * tables and constrain are those of rmx_region_prob; for the event E of query i over the model segments [a, b],
 *   logp_out[r][i] = log P*,  P* = max over (c_a .. c_b) satisfying E of q(c_a, .., c_b),
 * q the marginal of the run under the structured posterior of the last update_p_cn (everything outside [a, b] summed
 * out: comparable with P(E) of rmx_region_prob, which is the sum over the same paths), and states_out[r][i][k] = c*_{a+k},
 * one path that attains it.  Ties go to the lowest state index at every step.  The model is not modified.
 *   max_len    1 .. 16384, at least every query's b - a + 1
 *   states_out int16 [nr][nq][max_len]: state indices in [0, S) into each segment's class table; entries past the run,
 *              and every entry of an impossible or failed query, are -1
 *   logp_out   [nr][nq]; -inf for an impossible event.  A state whose forward entry underflowed to 0 in the sweep's scaled
 *              rows cannot be chosen, where its true probability is merely tiny (as rmx_call_prob)
 * A (restart, query) result, value and path, is bit-identical in any restart range, any batch of queries and for any
 * max_len.  Device memory a call holds beyond the model, kept with the batch: at most 64 MiB of staged outputs and
 * queries (the buffer rmx_region_prob uses) and at most 1 GiB of int16 back-pointers, max_len * S per (restart, query)
 * of a chunk; a call that needs more runs in chunks of queries and blocks of restarts (rmxh::decode_plan, rmx_host.h).
 * Errors as rmx_region_prob, and RMX_EARG with nothing launched and both outputs untouched for max_len out of range, a
 * query longer than max_len, or a NULL output.  RMX_EVALUE with the restarts listed: a restart has had no update_p_cn.
 * RMX_EASSERT with the restarts listed: a backward step met a zero or non-finite normaliser under positive mass, or a
 * maximum that is not a finite number >= 0 (that query's result is NaN, its states -1).  RMX_EUNSUPPORTED: more than
 * 1024 states. */
int rmx_region_decode(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries,
                      int32_t nmask, const uint8_t *masks, int32_t nlabel, const int16_t *labels, const uint8_t *constrain,
                      int32_t max_len, int16_t *states_out, double *logp_out);

/* Region alternatives: the K most probable copy-number configurations of a region, and their probabilities.
 * Queries, tables and constrain are those of rmx_region_decode; for the event E of query i over the model segments [a, b],
 *   logp_out[r][i][k] = log P*_k,  P*_0 >= P*_1 >= .. the K largest values of q(c_a, .., c_b) over pairwise distinct
 * configurations that satisfy E, q the marginal of the run as in rmx_region_decode, and states_out[r][i][k][j] = c_{a+j} of
 * the configuration of rank k.  Every state keeps its K best continuations, so the K configurations are distinct paths by
 * construction.  If fewer than K configurations have positive probability, the remaining ranks are -inf with states -1.
 * Tie rule: at every step the candidates W_n(s, s') h(s', j) are compared before the multiplication by fa_n(s) and the scaling;
 * one enters a state's list only if it is strictly greater than the entry it displaces, and candidates are met in order of s'
 * ascending, then rank j ascending, so equal values keep the lower (s', j) first; the final selection orders by value
 * descending, then state, then rank ascending.  Rank 0 -- value and states -- equals rmx_region_decode's result bit for bit.
 * A lower rank more than about 1e-308 below the most probable partial path of a step underflows and drops out, as a state
 * does in rmx_region_decode.  The model is not modified.
 *   K          1 .. 8
 *   max_len    1 .. 16384, at least every query's b - a + 1
 *   states_out int16 [nr][nq][K][max_len]; entries past the run, every entry of an empty rank and of a failed query are -1
 *   logp_out   [nr][nq][K]; -inf for an empty rank (all K for an impossible event)
 * A (restart, query) result, all K values and paths, is bit-identical in any restart range, any batch of queries, any
 * chunking and for any max_len, and ranks 0 .. K' - 1 of a call with K equal a call with K' < K.  Device memory a call holds
 * beyond the model, kept with the batch and shared with rmx_region_decode: at most 64 MiB of staged outputs and queries and
 * at most 1 GiB of int16 back-pointers, max_len * K * S per (restart, query) of a chunk (the largest strip is 256 MiB); a
 * call that needs more runs in chunks of queries and blocks of restarts (rmxh::kbest_plan, rmx_host.h).
 * Errors as rmx_region_decode, and RMX_EARG with nothing launched and both outputs untouched for K outside [1, 8].
 * RMX_EASSERT with the restarts listed: every rank of the failed query is NaN, its states -1. */
int rmx_region_kbest(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries,
                     int32_t nmask, const uint8_t *masks, int32_t nlabel, const int16_t *labels, const uint8_t *constrain,
                     int32_t K, int32_t max_len, int16_t *states_out, double *logp_out);

/* Locus joints: the exact joint posterior of copy number at two loci of a chain.  Query i is (a, t, row level
 * index, column level index): model segments a <= t of one chain and two of the level tables, levels int16 [C][nlevel][S]
 * with every entry >= 0 (a per-state integer under the state class of a segment: a clone's total, a 0/1 event).  With post,
 * fa, W_n and D_n as in rmx_region_prob,
 *   G_t(s, j) = [level_col,t(s) = j] post_t(s),   G_n(s, j) = fa_n(s) sum_s' W_n(s, s') G_n+1(s', j) / D_n(s'),
 *   cell(n; i, j) = log sum_{s: level_row,n(s) = i} G_n(s, j) = log P(level_row(c_n) = i and level_col(c_t) = j);
 * nothing binds between the loci.  nrow and ncol lie in 1 .. 16; a state whose level is >= ncol (>= nrow) is in no column
 * (row); an empty cell is -inf and is not an error.
 *   nslot = 0    the pair form: logp_out [nr][nq][nrow][ncol] holds the table at n = a
 *   nslot >= 1   the profile form: logp_out [nr][nq][nslot][nrow][ncol]; slot k holds the table at segment t - k for
 *                k = 0 .. t - a, later slots are NaN.  nslot <= 4096, every query has t - a + 1 <= nslot
 * Slot 0, and a pair with a = t, is log sum post_t(s) over the states that carry both levels.  max(nslot, 1) nrow ncol may
 * not exceed 2^20.  Every column keeps its own scale and running logarithm and is divided by its own sum after every step, the
 * start included (in real arithmetic that sum is 1: the division removes rounding drift).  Inside a column the rows share
 * the scale: a cell more than about 1e-308 below its column's total comes out -inf.  An fa entry that underflowed to 0 in the
 * sweep is a state the walk cannot pass.  The model is not modified.
 * A cell is bit-identical in any restart range, any batch and order of queries, any chunking, for any nrow that contains it
 * and any nslot; slot k of a profile query equals the pair form's table of (t - k, t) bit for bit.
 * Errors: RMX_EARG with nothing launched and the output untouched for a bad restart range, nq < 1, a NULL pointer, nrow or
 * ncol outside [1, 16], nlevel < 1, a level index out of range, a negative level entry, nslot outside [0, 4096], a profile
 * query longer than nslot, segments outside the model, a > t or in two chains; RMX_EVALUE with the restarts listed before
 * update_p_cn; RMX_EASSERT with the restarts listed for a normaliser D that is 0 or not finite under mass or a sum that is not
 * a finite number >= 0: every cell of that query is NaN; RMX_EUNSUPPORTED above 1024 states.  The kernel has no profile id. */
int rmx_locus_joint(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nlevel, const int16_t *levels,
                    int32_t nrow, int32_t ncol, int32_t nslot, double *logp_out);

/* Region automata: the exact posterior of regular path events over regions.  A deterministic finite automaton
 * with Q <= 16 states and A <= 16 symbols reads one symbol per segment of a run and the call returns the distribution of its
 * final state: the number of separate events of a run, whether some event spans k consecutive segments, how often copy
 * number switches between two levels, an ordered pattern.
 *   symbols int16 [C][nsym][S], every entry in [0, A): the symbol of a state under a state class (the levels' layout)
 *   delta uint8 [nauto][Q][A], every entry in [0, Q), and start int32 [nauto], every entry in [0, Q)
 *   1 <= Q <= 16, 1 <= A <= 16, 1 <= nauto <= 64
 *   query i = (a, b, symbol table index, automaton index) over the model segments a <= b of one chain
 *   constrain uint8 [N], or NULL for "every segment"
 * THE AUTOMATON READS THE RUN FROM ITS LAST SEGMENT TO ITS FIRST: b, b - 1, .. a, the direction of the walk.  A segment with
 * constrain[n] == 0 is NOT READ: its state is marginalised and the automaton does not move (unlike rmx_region_counts, where
 * such a segment still takes part in the label changes; deliberately so: an inserted zero-length segment is no segment of a
 * run).  With post, fa, W_n and D_n as in rmx_region_prob, sigma_n(s) the symbol of state s under the class of segment n
 * and q0 the start state,
 *   G_b(s, q) = post_b(s) [q = delta(q0, sigma_b(s))]                        (b not read: [q = q0])
 *   H(s', q)  = G_n+1(s', q) / D_n(s'),   X(s, q) = fa_n(s) sum_s' W_n(s, s') H(s', q)
 *   G_n(s, q) = sum_{q' ascending: delta(q', sigma_n(s)) = q} X(s, q')       (n not read: X(s, q))
 *   logp_out [nr][nq][Q]: out(q) = log sum_s G_a(s, q) = log P(the automaton ends in q).
 * A state that cannot be reached gives -inf and is no error.  Nothing binds, so in real arithmetic the total over (s, q) is 1
 * at every step and the Q outputs sum to 1; G is still divided by its total after every step, the start included, and the
 * logarithm is accumulated, which only removes rounding drift.  One scale carries all columns, because columns mix under
 * delta: a column more than about 1e-308 below the total comes out -inf.  The model is not modified.
 * A (restart, query) result is bit-identical in any restart range, any batch and order of queries, any chunking, and when
 * the automaton is padded with unreachable states up to a larger Q.
 * Errors: RMX_EARG with nothing launched and the output untouched for a bad restart range, nq < 1, a NULL pointer (constrain
 * excepted), nauto, Q or A out of bounds, nsym < 1, a delta or start entry outside [0, Q), a symbol outside [0, A), a symbol
 * table or automaton index out of range, segments outside the model, a > b or in two chains; RMX_EVALUE with the restarts
 * listed before update_p_cn; RMX_EASSERT with the restarts listed for a normaliser D that is 0 or not finite under mass or a
 * sum that is not a finite number >= 0: all Q entries of that query are NaN; RMX_EUNSUPPORTED above 1024 states.  The kernel
 * has no profile id. */
int rmx_region_automaton(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nsym, const int16_t *symbols,
                         int32_t nauto, int32_t Q, int32_t A, const uint8_t *delta, const int32_t *start, const uint8_t *constrain,
                         double *logp_out);

/* Path entropy: the exact Shannon entropy, in nats, of the copy-number path posterior over any run of segments,
 * as two arrays from which the host forms every run's entropy by prefix sums.  Under the structured posterior of the last
 * update_p_cn (the forward recursion of bpmodel.pyx:1213-1246) a chain is Markov with the backward kernel
 * q(c_n = s | c_n+1 = s') = fa_n(s) W_n(s, s') / D_n(s'), so  H(c_a .. c_b) = marg_b + sum_{n = a}^{b-1} step_n  with, for an
 * adjacency n -> n + 1 and post, fa, W_n as in rmx_region_prob,
 *   D(s')  = sum_s fa_n(s) W_n(s, s')
 *   E1(s') = sum_s fa_n(s) log fa_n(s) W_n(s, s')            (fa = 0: the term is 0)
 *   E2(s') = sum_s fa_n(s) W_n(s, s') log W_n(s, s')         (W = 0: the term is 0)
 *   step_n = H(c_n | c_n+1) = sum_{s': post_n+1(s') > 0} post_n+1(s') (log D(s') - (E1(s') + E2(s')) / D(s'))
 *   marg_n = H(post_n) = -sum_{s: post_n(s) > 0} post_n(s) log post_n(s)
 * marginal_out, step_out [nr][n1 - n0]: entry n - n0 of a restart's row; either may be NULL, not both.  step_n is +0.0 where
 * segment n ends a chain (there is no adjacency).  Both are >= 0; a sum that rounding left below zero is returned as +0.0.
 * The scale of a row of fa cancels.  The model is not modified.
 * An entry is bit-identical in any restart range, any segment range and any chunking.
 * Errors: RMX_EARG with nothing launched and the outputs untouched for a bad restart range, a segment range without
 * 0 <= n0 < n1 <= num_segments, or two NULL outputs; RMX_EVALUE with the restarts listed before update_p_cn; RMX_EASSERT with
 * the restarts listed where a D(s') is 0 or not finite under post_n+1(s') > 0 or a result is not a finite number: that entry is
 * NaN; RMX_EUNSUPPORTED above 1024 states.  The kernels have no profile id. */
int rmx_path_entropy(rmx_batch *b, int32_t r0, int32_t nr, int32_t n0, int32_t n1, double *marginal_out, double *step_out);

/* Region sums: the exact posterior distribution of a length-weighted event occupancy over regions: of the
 * additive functional sum_n w_n level_n(c_n) of the path over a run, with non-negative integer weights and levels -- how many
 * segments of a run are in an event, how many weight units of it are, how many copies its segments carry between them.
 *   levels int16 [C][nlevel][S], every entry >= 0: the level of a state under a state class (rmx_region_extremes' layout);
 *     a mask is a 0/1 table
 *   weights int32 [nwt], every entry >= 0: a flat pool
 *   query i = (a, b, level table index, weight offset o) over the model segments a <= b of one chain: segment n of the run
 *     has the weight w_n = weights[o + n - a]; 0 <= o and o + (b - a) < nwt
 *   1 <= nbins <= 64, and nbins <= the bins the kernel's LDS plan holds at S states: 64 up to 304 states, 32 up to 608, 16 up
 *     to 1024 (rmxh::sums_max_bins in remixt_amd/csrc/rmx_host.h)
 * There is no constrain vector: a weight of 0 is "this segment does not count".  With B = nbins, the increment
 * d_n(s) = min((int64) w_n level_n(s), B - 1) under the class of segment n, and post, fa, W_n and D_n as in rmx_region_prob,
 *   G_b(s, k) = post_b(s) [k = d_b(s)]
 *   H(s', k)  = G_n+1(s', k) / D_n(s'),   X(s, k) = fa_n(s) sum_s' W_n(s, s') H(s', k)
 *   G_n(s, k) = X(s, k - d_n(s))                          for d_n(s) <= k < B - 1   (0 for k < d_n(s))
 *   G_n(s, B-1) = sum_{k' = B-1-d_n(s)}^{B-1} X(s, k')    (ascending k'; d = 0: X(s, B-1))
 *   logp_out [nr][nq][B]: out(k) = log sum_s G_a(s, k) = log P(sum_n w_n level(c_n) == k); the last bin: >= B - 1.
 * A bin that cannot be reached gives -inf and is no error.  Nothing binds, so in real arithmetic the total over (s, k) is 1 at
 * every step and the B outputs sum to 1; G is still divided by its total after every step, the start included, and the
 * logarithm is accumulated, which only removes rounding drift.  ONE SCALE CARRIES ALL COLUMNS, because columns mix under the
 * shift: a bin more than about 1e-308 below the total comes out -inf.  The model is not modified.
 * A (restart, query) result is bit-identical in any restart range, any batch and order of queries, any chunking, and wherever
 * its weights lie in the pool.
 * Errors: RMX_EARG with nothing launched and the output untouched for a bad restart range, nq < 1, a NULL pointer, nlevel < 1,
 * nwt < 1, nbins outside [1, 64], a negative level or weight, a level index or a weight span out of range, segments outside
 * the model, a > b or in two chains; RMX_EVALUE with the restarts listed before update_p_cn; RMX_EASSERT with the restarts
 * listed for a normaliser D that is 0 or not finite under mass or a total that is not a finite number >= 0: all B entries of
 * that query are NaN; RMX_EUNSUPPORTED above 1024 states, or for more bins than the LDS plan holds at the batch's state count
 * (an argument check: nothing is launched).  The kernel has no profile id. */
int rmx_region_sums(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nlevel, const int16_t *levels,
                    int32_t nwt, const int32_t *weights, int32_t nbins, double *logp_out);

/* -- module-level functions on caller-supplied dense inputs ----------------- */
/* sum_product (:1213-1246): f [N][S], T [N-1][S][S] -> alphas, betas [N][S] */
int rmx_sum_product(const double *f, const double *T, double *alphas, double *betas,
                    int32_t N, int32_t S, int32_t device);
/* max_product (:1296-1333): returns path int64 [N] and the log probability */
int rmx_max_product(const double *f, const double *T, int64_t *state_sequence, double *logprob,
                    int32_t N, int32_t S, int32_t device);

/* -- measurement (bench.py): HIP events on the batch stream ----------------- */
int rmx_timer_start(rmx_batch *b);
int rmx_timer_stop(rmx_batch *b, double *elapsed_ms);
/* per-kernel accumulated device time since the last reset (HIP events around
 * each launch).  rmx_profile_enable: 0 = off, 1 = every kernel, 2 = only the kernels of the
 * variational sweep (the M-step objective kernels are launched thousands of times per EM
 * iteration; two event records per launch would perturb the host loop).  kernel ids: see
 * rmx_kernel_name(). */
int rmx_profile_enable(rmx_batch *b, int32_t on);
int rmx_profile_get(rmx_batch *b, int32_t kernel_id, double *total_ms, int64_t *launches);
int rmx_profile_reset(rmx_batch *b);
const char *rmx_kernel_name(int32_t kernel_id);
int rmx_num_kernels(void);
/* every id rmx_profile_get takes: the ids of rmx_num_kernels() first, under the names of rmx_kernel_name(), then the kernels added
 * after those two lists were closed (k_region_conditional).  "" outside [0, rmx_num_profile_ids()). */
const char *rmx_profile_name(int32_t profile_id);
int rmx_num_profile_ids(void);

#ifdef __cplusplus
}
#endif
#endif /* REMIXT_AMD_H */
