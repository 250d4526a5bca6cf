"""Region event extents (k_region_extent) of all 16 restarts of the bench workload (50 000 segments, one RestartSet) at 165 and 355
states, after one variational sweep, in one process.  Three workloads: every original segment as anchor with the 'state' label and a
window of 16 on each side; 500 anchors -- the segments with the largest posterior LOH probability in restart 0 -- with the 'loh' mask
and a window of 256 on each side (under a normal clone of (1, 1) no state is LOH: every slot is -inf and both routes end at once; the
workload is kept as the measure of that case); and 500 evenly spaced anchors with the 'total' label and a window of 256.  Per workload: the device time of k_region_extent from rmx_profile_get and the wall
time of the raw call, beside the nested-interval route -- rmx_region_prob with one query per slot, on the same anchors -- the calls
alternating, REPS times each, so that the spread between repeats stands beside the ratio; and the floor from the sizes: the S^2
weights a right step and the 2 S^2 weights a left step of a workgroup read from L2.  The nested route walks (w + 1) w / 2 steps per
side where the new call walks w: with --nested-anchors K both routes are also timed on K evenly spaced anchors of the workload
(the nested route alone takes minutes on all of the first).  The two routes are compared slot by slot: in P, and in log P where
log P > -300 (further down k_region_prob's sum-normalised recursion drops terms).  Then the sample route for the third
workload: posterior samples per restart (sample_states, 64 at a time) and the right end of the constant-total run around each anchor
counted on them in numpy.
Usage: python tools/extent_time.py [--samples K] [--reps N] [--nested-anchors K] [MAXCN ...]
(default 4096 samples, 3 repeats, every anchor; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK = 16, 64
L2 = 34.5e12      # aggregate L2 rate
args = sys.argv[1:]
K, REPS, NESTED = 4096, 3, 0
while args and args[0] in ('--samples', '--reps', '--nested-anchors'):
    if args[0] == '--samples':
        K = int(args[1])
    elif args[0] == '--reps':
        REPS = int(args[1])
    else:
        NESTED = int(args[1])
    args = args[2:]


def device_ms(b, fn, kernel):
    b.profile_reset(); b.profile_enable(1)
    t0 = time.perf_counter(); out = fn(); wall = time.perf_counter() - t0
    ms, n = b.profile().get(kernel, (0., 0)); b.profile_enable(0)
    return ms, n, wall * 1e3, out


def fmt(v):
    return ' '.join('%.3f' % x for x in v) + ' ms (median %.3f, spread %.1f %%)' % (np.median(v), 100. * (max(v) - min(v)) / np.median(v))


def nested_queries(n0, mi, li, wl, wr, cs, ce):
    """One rmx_region_prob query per in-chain slot of every anchor: (queries (Q, 4), anchor index (Q,), slot (Q,))."""
    c = np.searchsorted(ce, n0, side='left')
    k = np.arange(wl + wr + 1)
    n = n0[:, None] - wl + k[None]
    ok = (n >= cs[c][:, None]) & (n <= ce[c][:, None])
    a, s = np.nonzero(ok)
    q = np.stack([np.minimum(n[a, s], n0[a]), np.maximum(n[a, s], n0[a]), np.full(len(a), mi), np.full(len(a), li)], axis=1).astype(np.int32)
    return q, a, s


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    masks, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    fwd = np.asarray(m.seg_fwd_remap, dtype=np.int64)
    constrain = np.ascontiguousarray(np.asarray(m.seg_is_original) != 0, dtype=np.uint8)
    loh = posteriors.MASK_NAMES.index('loh')
    p_loh = b.posterior_summary_raw(0, 1, weights=np.ascontiguousarray(masks[:, loh:loh + 1].transpose(0, 2, 1).astype(float)),
                                    want_stats=False, want_argmax=False)[0][0, :, 0][fwd]
    top = np.sort(np.argsort(-p_loh, kind='stable')[:500])
    even = np.linspace(0, N - 1, 500).astype(int)
    workloads = [('every segment, state, w 16', np.arange(N), 'state', 16), ('500 LOH anchors, loh, w 256', top, 'loh', 256),
                 ('500 anchors, total, w 256', even, 'total', 256)]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts' % (S, N, N1, len(cs), R), flush=True)
    for name, anchors, event, w in workloads:
        mi, li = posteriors.parse_event(event)
        subsets = [('all %d anchors' % len(anchors), anchors, NESTED == 0 or NESTED >= len(anchors))]
        if NESTED and NESTED < len(anchors):
            subsets.append(('%d of them' % NESTED, anchors[np.linspace(0, len(anchors) - 1, NESTED).astype(int)], True))
        for sname, anc, with_nested in subsets:
            q, _ = posteriors.extent_queries(anc, event, fwd, constrain)
            n0 = q[:, 0].astype(np.int64)
            c = np.searchsorted(ce, n0, side='left')
            left, right = np.minimum(w, n0 - cs[c]), np.minimum(w, ce[c] - n0)
            steps = int(left.sum() + right.sum()) * R
            floor = (2. * left.sum() + right.sum()) * R * S * S * 8 / L2 * 1e3
            extent = lambda: b.region_extent_raw(0, R, q, masks, labels, constrain, w, w)
            extent()
            te, we, tn, wn = [], [], [], []
            if with_nested:
                qn, a_of, s_of = nested_queries(n0, mi, li, w, w, cs, ce)
                nested = lambda: b.region_logprob_raw(0, R, qn, masks, labels, constrain)
                nsteps = int((qn[:, 1] - qn[:, 0]).sum()) * R
                nested()
            for rep in range(REPS):
                ms, n, wall, out = device_ms(b, extent, 'k_region_extent'); te.append(ms); we.append(wall)
                if with_nested:
                    ms, nn, wall, lp = device_ms(b, nested, 'k_region_prob'); tn.append(ms); wn.append(wall)
            line = '  %s, %s: %d (restart, query) pairs, %d steps: k_region_extent %s over %d launches, call %.1f ms wall; %.3f us per step; floor (S^2 weights ' \
                   'per right step, 2 S^2 per left step / 34.5 TB/s of L2) %.3f ms (x%.2f)' % (name, sname, len(q) * R, steps, fmt(te), n, np.median(we),
                                                                                              np.median(te) * 1e3 / max(steps, 1), floor, np.median(te) / floor)
            if with_nested:
                got = np.full(out.shape, -np.inf)
                got[:, a_of, s_of] = lp
                fin = np.isfinite(got) & np.isfinite(out)
                near = fin & (np.where(fin, np.minimum(got, out), 0.) > -300.)
                same_inf = np.array_equal(np.isneginf(got), np.isneginf(out))
                line += '; nested route: %d queries, %d steps: k_region_prob %s over %d launches, call %.1f ms wall; nested / extent x%.2f device, x%.2f wall; ' \
                        'between the routes max |d P| %.3e over %d finite slots, max |d log P| %.3e over the %d of them with log P > -300, -inf slots %s' % (
                            len(qn) * R, nsteps, fmt(tn), nn, np.median(wn), np.median(tn) / np.median(te), np.median(wn) / np.median(we),
                            np.abs(np.exp(got[fin]) - np.exp(out[fin])).max() if fin.any() else 0., fin.sum(),
                            np.abs(got[near] - out[near]).max() if near.any() else 0., near.sum(), 'agree' if same_inf else 'differ')
                if not same_inf:
                    only_e, only_n = np.isneginf(out) & np.isfinite(got), np.isneginf(got) & np.isfinite(out)
                    line += ' (-inf from k_region_extent alone in %d slots, where k_region_prob has log P <= %.1f; from k_region_prob alone in %d slots, where ' \
                            'k_region_extent has log P <= %.1f)' % (only_e.sum(), got[only_e].max() if only_e.any() else -np.inf, only_n.sum(),
                                                                   out[only_n].max() if only_n.any() else -np.inf)
            print(line, flush=True)
    # the sample route for the third workload: the right end of the constant-total run around each anchor, on K samples per restart
    name, anchors, event, w = workloads[2]
    q, _ = posteriors.extent_queries(anchors, event, fwd, constrain)
    n0 = q[:, 0].astype(np.int64)
    exact = np.exp(b.region_extent_raw(0, R, q, masks, labels, constrain, 0, w))            # (R, A, w + 1): P(no change of the totals on [n0, n0 + k])
    lab_seg = labels[np.asarray(b.seg_class), posteriors.LABEL_NAMES.index('total')]         # (N1, S)
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    b.sample_states(0, R, CHUNK, seeds)
    t_draw = t_count = 0.
    reach = np.zeros((R, len(anchors), w + 1))
    c = np.searchsorted(ce, n0, side='left')
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
        t1 = time.perf_counter()
        lab = lab_seg[np.arange(N1)[None, None], st]                                       # (R, CHUNK, N1)
        # the first adjacency at or after n across which the label changes (N1 if none), by a reverse running minimum
        pos = np.full(lab.shape, N1, dtype=np.int32)
        pos[:, :, :-1] = np.where(lab[:, :, :-1] != lab[:, :, 1:], np.arange(N1 - 1, dtype=np.int32)[None, None], np.int32(N1))
        nxt = np.minimum.accumulate(pos[:, :, ::-1], axis=2)[:, :, ::-1]
        run_end = np.minimum(nxt[:, :, n0], ce[c][None, None])                              # the last segment of the run from n0
        length = np.clip(run_end - n0[None, None] + 1, 0, w + 1)                            # slots 0 .. length - 1 are reached
        for k in range(w + 1):
            reach[:, :, k] += (length > k).sum(axis=1)
        t_draw += t1 - t0; t_count += time.perf_counter() - t1
    est = reach / K
    err = np.abs(est - np.where(np.isfinite(exact), exact, 0.))
    print('  sample route, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall + counting the right end of the constant-total run of %d anchors in '
          'numpy %.0f ms = %.0f ms; |sample estimate - exact| of the right survival curve max %.3e, mean %.3e (1 / sqrt(K) = %.3e)' % (
              K, R, CHUNK, t_draw * 1e3, len(anchors), t_count * 1e3, (t_draw + t_count) * 1e3, err.max(), err.mean(), K ** -0.5), flush=True)
    rs.close()
