"""Region sums (k_region_sums) of all 16 restarts of the bench workload (50 000 segments in 23 chains, one RestartSet) at 165 and
355 states, after one variational sweep, in one process.  The query is the number of real segments of a region in LOH (weights
seg_is_original, the LOH mask as a 0/1 level table).  Workloads, those of tools/region_automaton_time.py:
  every pair of experiment segments that a reference adjacency joins;
  20 000 random regions of 1 .. 3 segments inside one chain;
  46 arm-sized regions (every 46th of the genome, cut back to the chain of its first segment).
Measured in the same run on the same runs of model segments:
  rmx_region_sums at 16 bins against rmx_region_automaton with the saturating counter automaton (16 states, delta(q, 1) =
  min(q + 1, 15), delta(q, 0) = q) on the same constrain: the same question, and the largest difference of the two answers;
  rmx_region_sums at the most bins of the state count (64 at 165 states, 32 at 355) against its 16-bin instance;
  the route that gave such numbers before: 4 096 posterior samples and host counting, for ONE restart (16 restarts of 4 096
  paths of 50 000 segments do not fit a host array); the line gives that time times 16 beside it.
Neither kernel has a profile id: both are timed by HIP events on the batch's stream around the whole call (rmx_timer_start /
rmx_timer_stop: the launches of every chunk and the copies of queries and results between them) and by wall clock.  Per workload
the calls alternate REPS times after a warm-up of each; medians and spreads are printed.
Usage: python tools/region_sums_time.py [--reps N] [--regions P] [MAXCN ...]   (default 5 repeats, 20 000 regions; 8 12)"""
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
    top = posteriors.sums_max_bins(S)
    fwd = np.asarray(m.seg_fwd_remap, dtype=np.int64)
    orig = np.asarray(m.seg_is_original) != 0
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    chain = np.searchsorted(ce, fwd, side='left')
    loh = posteriors.symbols_from(b.cn_classes, ['loh'])                       # 0/1: a symbol table and a level table alike
    counter = np.array([[[q, min(q + 1, 15)] for q in range(16)]], dtype=np.uint8)
    rng = np.random.RandomState(0)
    adj, _ = posteriors.adjacency_regions(fwd, m.is_telomere)
    first = rng.randint(0, N - 3, size=NREG)
    last = first + rng.randint(0, 3, size=NREG)
    small = np.stack([first, last], axis=1)[chain[first] == chain[last]]
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.array([[x, max(x, min(y - 1, int(np.flatnonzero(chain == chain[x])[-1])))] for x, y in zip(edges[:-1], edges[1:])])
    print('%d states, %d segments (%d in the model), %d chains, %d restarts; the most bins: %d' % (S, N, N1, len(cs), R, top), flush=True)
    for name, regions in (('%d adjacency pairs' % len(adj), adj), ('%d regions of 1-3 segments' % len(small), small), ('%d arm-sized regions' % len(arms), arms)):
        runs = np.stack([fwd[regions[:, 0]], fwd[regions[:, 1]]], axis=1).astype(np.int32)
        steps = int((runs[:, 1] - runs[:, 0]).sum()) * R
        # the pool is seg_is_original itself: a run's weights begin at its first segment
        lens = runs[:, 1] - runs[:, 0] + 1
        pool = orig.astype(np.int32)
        qs = np.stack([runs[:, 0], runs[:, 1], np.zeros(len(runs), dtype=np.int32), runs[:, 0]], axis=1).astype(np.int32)
        qa = np.concatenate([runs, np.zeros((len(runs), 2), dtype=np.int32)], axis=1)
        s16 = lambda: b.region_sums_raw(0, R, qs, loh[:, None, :], pool, 16)
        stop = lambda: b.region_sums_raw(0, R, qs, loh[:, None, :], pool, top)
        aut = lambda: b.region_automaton_raw(0, R, qa, loh[:, None, :], counter, np.array([0]), orig)
        o16 = s16(); otop = stop(); oa = aut()
        with np.errstate(over='ignore'):
            pmf, pa, ptop = np.exp(o16), np.exp(oa), np.exp(otop)
        t16, w16, tt, ta = [], [], [], []
        for rep in range(REPS):
            ms, wall, _ = timed(b, s16); t16.append(ms); w16.append(wall)
            ms, wall, _ = timed(b, aut); ta.append(ms)
            ms, wall, _ = timed(b, stop); tt.append(ms)
        us = lambda v: np.median(v) * 1e3 / max(steps, 1)
        print('  %s: %d (restart, region) walks, %d backward steps, longest run %d; sum P - 1 at most %.2e; mean number of LOH segments %.4f; mass in the last of %d bins at most %.3g' % (
            name, len(runs) * R, steps, int(lens.max()), np.abs(pmf.sum(axis=-1) - 1).max(), (ptop * np.arange(top)).sum(axis=-1).mean(), top, ptop[..., -1].max()), flush=True)
        print('    rmx_region_sums, 16 bins:                    stream %s; wall %s; %.3f us per step' % (fmt(t16), fmt(w16), us(t16)), flush=True)
        print('    rmx_region_automaton, the counter automaton: stream %s; %.3f us per step; sums / automaton %.2f; largest |dP| %.2e' % (
            fmt(ta), us(ta), np.median(t16) / np.median(ta), np.abs(pmf - pa).max()), flush=True)
        print('    rmx_region_sums, %d bins:                    stream %s; %.3f us per step; %d bins / 16 bins %.2f' % (top, fmt(tt), us(tt), top, np.median(tt) / np.median(t16)), flush=True)
        if len(runs) > 30000:
            continue          # (the sample route is counted on the two region workloads)
        # the sample route, ONE restart: 4 096 paths, the LOH flag of every real segment, a cumulative sum, a histogram per region
        ts, th = [], []
        for rep in range(max(3, REPS // 2)):
            t0 = time.perf_counter()
            b.synchronize()
            st = b.sample_states(0, 1, NS, [rep])[0]
            b.synchronize()
            t1 = time.perf_counter()
            real = np.flatnonzero(orig)
            ev = loh[np.asarray(b.seg_class)[real][None, :], st[:, real]] != 0
            cum = np.concatenate([np.zeros((NS, 1), dtype=np.int32), np.cumsum(ev, axis=1, dtype=np.int32)], axis=1)
            x, y = regions[:, 0], regions[:, 1]
            count = cum[:, y + 1] - cum[:, x]
            hist = np.stack([(np.minimum(count, top - 1) == k).mean(axis=0) for k in range(top)], axis=1)
            t2 = time.perf_counter()
            ts.append((t1 - t0) * 1e3); th.append((t2 - t1) * 1e3)
            st = None
        dev = np.abs(hist - ptop[0]).max()
        print('    4 096 samples of ONE restart + host counting: sampling wall %s; counting wall %s; times 16 restarts %.0f ms = x%.1f of the 16-bin call\'s wall; '
              'largest |sampled - exact| %.4f' % (fmt(ts), fmt(th), 16 * (np.median(ts) + np.median(th)), 16 * (np.median(ts) + np.median(th)) / np.median(w16), dev), flush=True)
    rs.close()
