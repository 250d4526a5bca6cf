"""Restart overlap (k_restart_overlap) between all pairs of the 16 restarts of the bench workload (50 000 segments, one
RestartSet) after one variational sweep, in one process.  The three workloads of tools/region_time.py: every adjacency pair,
20 000 regions of one to three segments, 46 arm-sized regions; each under the identity clone map, in both modes (0: the
Bhattacharyya overlap, 1: the coincidence probability).  Beside it k_region_prob on the same runs without a constraint for the
16 restarts: one chain's recursion of the same shape, which belongs to the parent commit.  The calls alternate; per side the
median of the repeats of the kernel's device time (rmx_profile_get) and of the call's wall time, with the spread (min .. max)
and the number of launches, and the device time divided by the number of workgroups -- a (pair, run) there, a (restart, run)
here: the chip's time per workgroup with all of them in flight, not one workgroup's latency.
Usage: python tools/overlap_time.py [--reps K] [MAXCN ...]   (default 3 repeats; 8: 165 states; 12 is 355)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, synthetic
from remixt_amd.restarts import RestartSet

R, REPS = 16, 3
args = sys.argv[1:]
while args and args[0] == '--reps':
    REPS = int(args[1])
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


for mcn in [int(a) for a in args] or [8]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    tables = posteriors.state_permutation_tables(b.cn_classes, posteriors.clone_permutations(3)[:1])
    pairs = np.array([(i, j) for i in range(R) for j in range(i + 1, R)])
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 3, size=20000)
    small = np.stack([first, first + rng.randint(0, 3, size=20000)], axis=1)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.stack([edges[:-1], edges[1:] - 1], axis=1)
    workloads = [('every adjacency', posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)[0]), ('20 000 regions of 1-3 segments', small),
                 ('46 arm-sized regions', arms)]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts, %d pairs' % (S, N, N1, len(cs), R, len(pairs)), flush=True)
    for name, regions in workloads:
        runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
        P = len(runs)
        q = np.concatenate([runs, np.zeros((P, 2), dtype=np.int32)], axis=1).astype(np.int32)
        qr = np.concatenate([runs, np.full((P, 2), -1)], axis=1).astype(np.int32)
        steps = int((runs[:, 1] - runs[:, 0]).sum())
        bc = lambda: b.restart_overlap_raw(None, pairs, q, tables, 0)
        co = lambda: b.restart_overlap_raw(None, pairs, q, tables, 1)
        one = lambda: b.region_logprob_raw(0, R, qr, None, None, constrain)
        dev, wall, launches = alternating(b, [(bc, 'k_restart_overlap'), (co, 'k_restart_overlap'), (one, 'k_region_prob')])
        got = bc()
        wg = [len(pairs) * P, len(pairs) * P, R * P]
        per = [np.median(d) * 1e3 / w for d, w in zip(dev, wg)]
        print('  %-31s %6d runs, %8d steps per chain' % (name + ':', P, steps))
        print('    k_restart_overlap, mode 0, %3d pairs:  device %s ms in %d launches, call %s ms wall, %8.3f us per (pair, run)' % (
            len(pairs), fmt(dev[0]), launches[0], fmt(wall[0]), per[0]))
        print('    k_restart_overlap, mode 1, %3d pairs:  device %s ms in %d launches, call %s ms wall, %8.3f us per (pair, run)' % (
            len(pairs), fmt(dev[1]), launches[1], fmt(wall[1]), per[1]))
        print('    k_region_prob, %2d restarts, same runs: device %s ms in %d launches, call %s ms wall, %8.3f us per (restart, run)' % (
            R, fmt(dev[2]), launches[2], fmt(wall[2]), per[2]))
        print('    per workgroup, overlap / one chain: x%.2f (mode 0), x%.2f (mode 1); log BC in [%.3f, %.3g], %d of %d are -inf or NaN' % (
            per[0] / per[2], per[1] / per[2], np.nanmin(got[np.isfinite(got)]), np.nanmax(got[np.isfinite(got)]), (~np.isfinite(got)).sum(), got.size), flush=True)
    rs.close()
