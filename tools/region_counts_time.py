"""Region change counts (k_region_counts) of all 16 restarts of the bench workload (50 000 segments, one RestartSet) at 165 and 355
states, after one variational sweep, in one process.  The three workloads of tools/region_time.py: every adjacency pair, 20 000
regions of one to three segments, 46 arm-sized regions; each asked for the `state` label with 16 bins.  Per workload: the device time
of k_region_counts from rmx_profile_get and the wall time of the raw call, beside the device time of k_region_prob on the same runs
with the same label (the one-bin answer "no change") and the L2 weight-traffic figure of DESIGN 4.10's table (2 S^2 weights per step
of a workgroup).  Then the route without the kernel: 4 096 posterior samples per restart (sample_states, 64 at a time) and the
changes of the same runs counted on them in numpy.
Usage: python tools/region_counts_time.py [--samples K] [--bins B] [MAXCN ...]   (default 4096 samples, 16 bins; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK = 16, 64
L2 = 34.5e12      # aggregate L2 rate
args = sys.argv[1:]
K, BINS = 4096, 16
while args and args[0] in ('--samples', '--bins'):
    if args[0] == '--samples':
        K = int(args[1])
    else:
        BINS = int(args[1])
    args = args[2:]


def timed(b, fn, kernel):
    fn()
    wall = []
    for rep in range(3):
        t0 = time.perf_counter(); fn(); wall.append(time.perf_counter() - t0)
    b.profile_reset(); b.profile_enable(1)
    fn()
    ms, n = b.profile().get(kernel, (0., 0)); b.profile_enable(0)
    return np.median(wall) * 1e3, ms, n


def count_changes(ne, runs):
    """ne (..., N1) with a leading column of zeros: cumulative number of unequal adjacencies -> the changes inside each run [a, b]."""
    return ne[..., runs[:, 1]] - ne[..., runs[:, 0]]


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    masks, labels = posteriors.event_tables(b.cn_classes)
    li = posteriors.LABEL_NAMES.index('state')
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 3, size=20000)
    small = np.stack([first, first + rng.randint(0, 3, size=20000)], axis=1)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.stack([edges[:-1], edges[1:] - 1], axis=1)
    workloads = [('every adjacency', posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)[0]), ('20 000 regions of 1-3 segments', small),
                 ('46 arm-sized regions', arms)]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts, %d bins' % (S, N, N1, len(cs), R, BINS), flush=True)
    pieces, exact = [], []
    for name, regions in workloads:
        runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
        q = np.concatenate([runs, np.full((len(runs), 1), -1), np.full((len(runs), 1), li)], axis=1).astype(np.int32)
        pieces.append(runs.astype(np.int64))
        steps = int((runs[:, 1] - runs[:, 0]).sum()) * R
        f_l2 = steps * 2. * S * S * 8 / L2 * 1e3
        wall, ms, n = timed(b, lambda: b.region_counts_raw(0, R, q, None, labels, constrain, BINS), 'k_region_counts')
        wall1, ms1, n1 = timed(b, lambda: b.region_logprob_raw(0, R, q, None, labels, constrain), 'k_region_prob')
        exact.append(np.exp(b.region_counts_raw(0, R, q, None, labels, constrain, BINS)))
        print('  %-31s %8d (restart, query) pairs, %9d steps: k_region_counts %9.3f ms device over %d launches, call %.1f ms wall; k_region_prob '
              '%9.3f ms device, call %.1f ms wall (x%.2f); 2 S^2 weights per step / 34.5 TB/s of L2: %.3f ms (x%.2f)' % (
                  name + ':', len(q) * R, steps, ms, n, wall, ms1, wall1, ms / ms1 if ms1 else float('nan'), f_l2, ms / f_l2 if f_l2 else float('nan')),
              flush=True)
    # the same distributions from posterior samples
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    b.sample_states(0, R, CHUNK, seeds)
    t_draw = t_count = 0.
    hist = [np.zeros((R, len(runs), BINS)) for runs in pieces]
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
        t1 = time.perf_counter()
        ne = np.zeros(st.shape[:2] + (N1,), dtype=np.int32)
        np.cumsum(st[:, :, :-1] != st[:, :, 1:], axis=2, out=ne[:, :, 1:])
        for h, runs in zip(hist, pieces):
            c = np.minimum(count_changes(ne, runs), BINS - 1)
            for k in range(BINS):
                h[:, :, k] += (c == k).sum(axis=1)
        t_draw += t1 - t0; t_count += time.perf_counter() - t1
    print('  sample route, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall + counting the changes of the three '
          'workloads in numpy %.0f ms = %.0f ms' % (K, R, CHUNK, t_draw * 1e3, t_count * 1e3, (t_draw + t_count) * 1e3), flush=True)
    for (name, _), h, p in zip(workloads, hist, exact):
        err = np.abs(h / K - p)
        print('  %s: |sample estimate - exact| max %.3e, mean %.3e (1 / sqrt(K) = %.3e)' % (name, err.max(), err.mean(), K ** -0.5), flush=True)
    rs.close()
