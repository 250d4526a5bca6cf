"""Region automata (k_region_automaton) of all 16 restarts of the bench workload (50 000 segments in 23 chains, one RestartSet) at
165 and 355 states, after one variational sweep, in one process.  The query is posteriors.automaton_runs(8) on the LOH mask: the
number of separate LOH events of a region.  Workloads:
  every pair of experiment segments that a reference adjacency joins;
  20 000 random regions of 1 .. 3 segments inside one chain;
  46 arm-sized regions (every 46th of the genome, cut back to the chain of its first segment).
Yardsticks, measured in the same run on the same runs of model segments:
  k_region_counts at 16 bins (label 'state'), from its profile id, and k_locus_joint (16 x 16, the tumour clones' highest total),
  from HIP events around the call: the per-step cost of the two siblings;
  the route that gave the same numbers before: 4 096 posterior samples and host counting.  The samples of ONE restart are drawn
  and counted (16 restarts of 4 096 paths of 50 000 segments do not fit a host array); the line says so and gives that time
  times 16 beside it.
k_region_automaton has no profile id: it is timed by HIP events on the batch's stream around the whole call (rmx_timer_start /
rmx_timer_stop: the launches of every chunk and the copies of queries and results between them) and by wall clock.  Per workload
the calls alternate REPS times after a warm-up of each; medians and spreads are printed.
Usage: python tools/region_automaton_time.py [--reps N] [--regions P] [MAXCN ...]   (default 5 repeats, 20 000 regions; 8 12)"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from remixt_amd import posteriors, synthetic
from remixt_amd.restarts import RestartSet

R, NS = 16, 4096
args = sys.argv[1:]
REPS, NREG = 5, 20000
while args and args[0] in ('--reps', '--regions'):
    if args[0] == '--reps':
        REPS = int(args[1])
    else:
        NREG = int(args[1])
    args = args[2:]


def timed(b, fn):
    b.synchronize()
    b.timer_start()
    t0 = time.perf_counter(); out = fn(); wall = time.perf_counter() - t0
    return b.timer_stop(), wall * 1e3, out


def fmt(v):
    return 'median %.3f ms, spread %.1f %%' % (np.median(v), 100. * (max(v) - min(v)) / np.median(v))


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    fwd = np.asarray(m.seg_fwd_remap, dtype=np.int64)
    orig = np.asarray(m.seg_is_original) != 0
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    chain = np.searchsorted(ce, fwd, side='left')
    au = posteriors.automaton_runs(8)
    sym = posteriors.symbols_from(b.cn_classes, ['loh'])
    masks, labels = posteriors.event_tables(b.cn_classes)
    levels, names = posteriors.locus_level_tables(b.cn_classes, 16)
    lv = names.index('peak_total_any')
    rng = np.random.RandomState(0)
    adj, _ = posteriors.adjacency_regions(fwd, m.is_telomere)
    first = rng.randint(0, N - 3, size=NREG)
    last = first + rng.randint(0, 3, size=NREG)
    small = np.stack([first, last], axis=1)[chain[first] == chain[last]]
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.array([[x, max(x, min(y - 1, int(np.flatnonzero(chain == chain[x])[-1])))] for x, y in zip(edges[:-1], edges[1:])])
    print('%d states, %d segments (%d in the model), %d chains, %d restarts, automaton_runs(8): Q %d, A %d' % (S, N, N1, len(cs), R, au.delta.shape[0], au.alphabet), flush=True)
    st = None
    for name, regions in (('%d adjacency pairs' % len(adj), adj), ('%d regions of 1-3 segments' % len(small), small), ('%d arm-sized regions' % len(arms), arms)):
        runs = np.stack([fwd[regions[:, 0]], fwd[regions[:, 1]]], axis=1).astype(np.int32)
        steps = int((runs[:, 1] - runs[:, 0]).sum()) * R
        zero = np.zeros((len(runs), 2), dtype=np.int32)
        qa = np.concatenate([runs, zero], axis=1)
        qc = np.concatenate([runs, np.full((len(runs), 1), -1, dtype=np.int32), np.full((len(runs), 1), posteriors.LABEL_NAMES.index('state'), dtype=np.int32)], axis=1)
        ql = np.concatenate([runs, np.full((len(runs), 2), lv, dtype=np.int32)], axis=1)
        new = lambda: b.region_automaton_raw(0, R, qa, sym[:, None, :], au.delta[None], np.array([au.start]), orig)
        cnt = lambda: b.region_counts_raw(0, R, qc, None, labels, orig, 16)
        loc = lambda: b.locus_joint_raw(0, R, ql, levels, 16, 16, 0)
        out = new(); cnt(); loc()
        pmf = np.exp(out).reshape(R, len(runs), 8, 2).sum(axis=-1)
        tn, wn, tc, tl = [], [], [], []
        for rep in range(REPS):
            ms, wall, _ = timed(b, new); tn.append(ms); wn.append(wall)
            b.profile_reset(); b.profile_enable(1)
            cnt()
            tc.append(b.profile().get('k_region_counts', (0., 0))[0]); b.profile_enable(0)
            ms, wall, _ = timed(b, loc); tl.append(ms)
        us = lambda v: np.median(v) * 1e3 / max(steps, 1)
        print('  %s: %d (restart, region) walks, %d backward steps, longest run %d; sum P - 1 at most %.2e; mean number of LOH events %.4f' % (
            name, len(runs) * R, steps, int((runs[:, 1] - runs[:, 0]).max()) + 1, np.abs(pmf.sum(axis=-1) - 1).max(), (pmf * np.arange(8)).sum(axis=-1).mean()), flush=True)
        print('    rmx_region_automaton:                       stream %s; wall %s; %.3f us per step' % (fmt(tn), fmt(wn), us(tn)), flush=True)
        print('    k_region_counts on the same runs, 16 bins:  kernel %s; %.3f us per step; automaton / counts %.2f' % (fmt(tc), us(tc), np.median(tn) / np.median(tc)), flush=True)
        print('    rmx_locus_joint on the same runs, 16 x 16:  stream %s; %.3f us per step; automaton / locus %.2f' % (fmt(tl), us(tl), np.median(tn) / np.median(tl)), flush=True)
        if len(runs) > 30000:
            continue          # (the sample route is counted on the two region workloads)
        # the sample route, ONE restart: 4 096 paths, the LOH flag of every real segment, run starts by a cumulative sum
        ts, th = [], []
        for rep in range(max(3, REPS // 2)):
            t0 = time.perf_counter()
            b.synchronize()
            st = b.sample_states(0, 1, NS, [rep])[0]
            b.synchronize()
            t1 = time.perf_counter()
            real = np.flatnonzero(orig)
            ev = sym[np.asarray(b.seg_class)[real][None, :], st[:, real]] != 0
            begins = ev.copy()
            begins[:, 1:] &= ~ev[:, :-1]
            cum = np.concatenate([np.zeros((NS, 1), dtype=np.int32), np.cumsum(begins, axis=1, dtype=np.int32)], axis=1)
            x, y = regions[:, 0], regions[:, 1]
            nruns = cum[:, y + 1] - cum[:, x + 1] + ev[:, x]
            hist = np.stack([(np.minimum(nruns, 7) == k).mean(axis=0) for k in range(8)], axis=1)
            t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3); th.append((t2 - t1) * 1e3)
        dev = np.abs(hist - pmf[0]).max()
        print('    4 096 samples of ONE restart + host counting: sampling wall %s; counting wall %s; times 16 restarts %.0f ms = x%.1f of the automaton call\'s wall; '
              'largest |sampled - exact| %.4f' % (fmt(ts), fmt(th), 16 * (np.median(ts) + np.median(th)), 16 * (np.median(ts) + np.median(th)) / np.median(wn), dev), flush=True)
        st = None
    rs.close()
