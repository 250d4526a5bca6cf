"""Region extremes (k_region_extremes) of all 16 restarts of the bench workload (50 000 segments, one RestartSet) at 165 and 355
states, after one variational sweep, in one process.  The three workloads of tools/region_time.py: every adjacency pair, 20 000
regions of one to three segments, 46 arm-sized regions; each asked for the peak of clone 1's total copy number with 16 columns.
The yardstick is the route to the same numbers without the kernel: rmx_region_prob on 16 nested custom masks (level <= j) per
run, in the same process with the two calls alternating; per side the median of five repeats of the kernel's device time
(rmx_profile_get) and of the call's wall time, with the spread (min .. max) and the number of launches.  Beside them
k_region_counts on the same runs (label `state`, 16 bins) for the per-step comparison, and the largest difference between the
two routes, in probability and -- where both are above -300 -- in the logarithm.  Then the route through posterior samples
(sample_states, 64 at a time) with the peak of the same runs taken on them in numpy.
Usage: python tools/region_extremes_time.py [--samples K] [MAXCN ...]   (default 512 samples; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK, NCOL, REPS = 16, 64, 16, 5
args = sys.argv[1:]
K = 512
while args and args[0] == '--samples':
    K = int(args[1])
    args = args[2:]


def alternating(b, sides):
    """sides: (call, kernel name) each; REPS rounds of every side in turn after one warm-up round.  Per side
    (device ms per repeat, wall ms per repeat, launches of one call)."""
    for fn, _ in sides:
        fn()
    dev, wall, launches = [[] for _ in sides], [[] for _ in sides], [0 for _ in sides]
    for rep in range(REPS):
        for i, (fn, kernel) in enumerate(sides):
            b.profile_reset(); b.profile_enable(1)
            t0 = time.perf_counter(); fn(); wall[i].append((time.perf_counter() - t0) * 1e3)
            ms, n = b.profile().get(kernel, (0., 0)); b.profile_enable(0)
            dev[i].append(ms); launches[i] = n
    return dev, wall, launches


def fmt(v):
    return '%9.3f (%.3f .. %.3f)' % (np.median(v), np.min(v), np.max(v))


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    _, labels = posteriors.event_tables(b.cn_classes)
    levels, names = posteriors.level_tables(b.cn_classes, NCOL)
    vi = names.index('peak_total_1')
    nested = np.ascontiguousarray((levels[:, vi, None, :] <= np.arange(NCOL)[None, :, None]).astype(np.uint8))      # (C, 16, S)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 3, size=20000)
    small = np.stack([first, first + rng.randint(0, 3, size=20000)], axis=1)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.stack([edges[:-1], edges[1:] - 1], axis=1)
    workloads = [('every adjacency', posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)[0]), ('20 000 regions of 1-3 segments', small),
                 ('46 arm-sized regions', arms)]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts, %d columns' % (S, N, N1, len(cs), R, NCOL), flush=True)
    pieces, exact = [], []
    for name, regions in workloads:
        runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
        P = len(runs)
        q = np.concatenate([runs, np.full((P, 1), -1), np.full((P, 1), vi)], axis=1).astype(np.int32)
        q16 = np.zeros((P, NCOL, 4), dtype=np.int32)
        q16[:, :, :2], q16[:, :, 2], q16[:, :, 3] = runs[:, None], np.arange(NCOL)[None], -1
        q16 = q16.reshape(-1, 4)
        qc = np.concatenate([runs, np.full((P, 1), -1), np.full((P, 1), posteriors.LABEL_NAMES.index('state'))], axis=1).astype(np.int32)
        pieces.append(runs.astype(np.int64))
        steps = int((runs[:, 1] - runs[:, 0]).sum()) * R
        one = lambda: b.region_extremes_raw(0, R, q, None, levels, constrain, NCOL)
        sixteen = lambda: b.region_logprob_raw(0, R, q16, nested, None, constrain)
        counts = lambda: b.region_counts_raw(0, R, qc, None, labels, constrain, NCOL)
        dev, wall, launches = alternating(b, [(one, 'k_region_extremes'), (sixteen, 'k_region_prob'), (counts, 'k_region_counts')])
        got, ref = one(), sixteen().reshape(R, P, NCOL)
        exact.append(np.exp(got))
        both = (got > -300) & (ref > -300)
        dlog = np.abs(got[both] - ref[both]).max() if both.any() else 0.
        print('  %-31s %8d (restart, run) pairs, %9d steps' % (name + ':', P * R, steps))
        print('    k_region_extremes, one walk:            device %s ms in %d launches, call %s ms wall' % (fmt(dev[0]), launches[0], fmt(wall[0])))
        print('    k_region_prob, 16 nested mask queries:  device %s ms in %d launches, call %s ms wall' % (fmt(dev[1]), launches[1], fmt(wall[1])))
        print('    k_region_counts, 16 bins, same runs:    device %s ms in %d launches, call %s ms wall' % (fmt(dev[2]), launches[2], fmt(wall[2])))
        print('    16 queries / one walk: x%.2f device, x%.2f wall; one walk / k_region_counts: x%.2f device; the two routes differ by at most %.3e in P, '
              '%.3e in log P over %d columns above -300 (%d of them below -20); -inf in %d columns of the walk, %d of the queries' % (
                  np.median(dev[1]) / np.median(dev[0]), np.median(wall[1]) / np.median(wall[0]), np.median(dev[0]) / np.median(dev[2]),
                  np.abs(np.exp(got) - np.exp(ref)).max(), dlog, both.sum(), (both & (ref < -20)).sum(), (got == -np.inf).sum(), (ref == -np.inf).sum()), flush=True)
    # the same distributions from posterior samples: the level of every sampled state (0 where a segment does not bind), the maximum over each run
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    lev_seg = np.where(np.asarray(m.seg_is_original, dtype=bool)[:, None], levels[b.seg_class, vi], 0).astype(np.int16)      # (N1, S)
    b.sample_states(0, R, CHUNK, seeds)
    t_draw = t_count = 0.
    hist = [np.zeros((R, len(runs), NCOL)) for runs in pieces]
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
        t1 = time.perf_counter()
        lv = np.zeros(st.shape[:2] + (N1 + 1,), dtype=np.int16)
        lv[:, :, :N1] = lev_seg[np.arange(N1)[None, None, :], st]
        for h, runs in zip(hist, pieces):
            if (runs[:, 1] - runs[:, 0]).max() <= 2:
                peak = np.maximum(np.maximum(lv[:, :, runs[:, 0]], lv[:, :, np.minimum(runs[:, 0] + 1, runs[:, 1])]), lv[:, :, runs[:, 1]])
            else:
                order = np.argsort(runs[:, 0])
                idx = np.stack([runs[order, 0], runs[order, 1] + 1], axis=1).ravel()
                peak = np.empty(st.shape[:2] + (len(runs),), dtype=np.int16)
                peak[:, :, order] = np.maximum.reduceat(lv, idx, axis=2)[:, :, ::2]
            for k in range(NCOL):
                h[:, :, k] += (peak <= k).sum(axis=1)
        t_draw += t1 - t0; t_count += time.perf_counter() - t1
    print('  sample route, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall + the peak of the three workloads\' runs in numpy '
          '%.0f ms = %.0f ms' % (K, R, CHUNK, t_draw * 1e3, t_count * 1e3, (t_draw + t_count) * 1e3), flush=True)
    for (name, _), h, p in zip(workloads, hist, exact):
        err = np.abs(h / K - p)
        print('  %s: |sample estimate - exact| of the CDF max %.3e, mean %.3e (1 / sqrt(K) = %.3e)' % (name, err.max(), err.mean(), K ** -0.5), flush=True)
    rs.close()
