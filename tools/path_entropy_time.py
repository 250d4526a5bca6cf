"""Path entropy (k_path_entropy, k_path_entropy_adj) of all 16 restarts of the bench workload (50 000 segments in 23 chains, one
RestartSet) at 165 and 355 states, after one variational sweep, in one process: one call over all model segments.
Yardsticks, measured in the same run, alternating with the call:
  cn_change_prob (posteriors.batch_change_prob): the sibling that forms the same D on the same adjacencies without sharing
  weights -- one k_region_prob workgroup per (restart, adjacency pair) -- from its profile id and by wall clock;
  the only route to a region's entropy before: K = 4 096 paths of rmx_sample_cn for ONE restart, their log q over the run from
  rmx_call_prob, and -mean with its standard error, for the longest chain (wall clock; the line gives that time times 16).
The two kernels have no profile id: the call is timed as a whole, by HIP events on the batch's stream around it (rmx_timer_start /
rmx_timer_stop: both kernels of every model run, the copy of the work lists and of the two result planes) and by wall clock; there is
no per-kernel time.  The calls alternate REPS times after a warm-up of each; medians and
spreads are printed.  Then the ten most uncertain of 46 arm-sized regions of restart 0.
Usage: python tools/path_entropy_time.py [--reps N] [MAXCN ...]   (default 5 repeats; 8 12)"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from remixt_amd import posteriors, synthetic
from remixt_amd.restarts import RestartSet

R, NS = 16, 4096
args = sys.argv[1:]
REPS = 5
while args and args[0] == '--reps':
    REPS = int(args[1])
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
    maps = (m.seg_fwd_remap, m.seg_is_original, m.is_telomere)
    fwd = np.asarray(m.seg_fwd_remap, dtype=np.int64)
    orig = np.asarray(m.seg_is_original) != 0
    tel = np.asarray(m.is_telomere) != 0
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    chain = np.searchsorted(ce, fwd, side='left')
    inner = ~tel
    inner[-1] = False
    nbe = int((inner & (np.asarray(m.breakpoint_idx) >= 0)).sum())
    nadj = int(inner.sum())
    print('%d states, %d segments (%d in the model), %d chains, %d restarts: %d adjacencies, %d of them breakends (%.1f %%)' % (
        S, N, N1, len(cs), R, nadj, nbe, 100. * nbe / nadj), flush=True)
    new = lambda: b.path_entropy_raw(0, R)
    old = lambda: posteriors.batch_change_prob(b, 0, R, *maps)
    (marg, step), pc = new(), old()
    tn, wn, tk, wo = [], [], [], []
    for rep in range(REPS):
        ms, wall, _ = timed(b, new); tn.append(ms); wn.append(wall)
        b.profile_reset(); b.profile_enable(1)
        t0 = time.perf_counter(); old(); b.synchronize(); wo.append((time.perf_counter() - t0) * 1e3)
        tk.append(b.profile().get('k_region_prob', (0., 0))[0]); b.profile_enable(0)
    flop = 6. * S * S * nadj * R
    print('  rmx_path_entropy, all %d segments:   stream %s; wall %s; %.3f us per (restart, adjacency); %.2f TFLOP/s on 6 S^2 flop per (restart, adjacency)' % (
        N1, fmt(tn), fmt(wn), np.median(tn) * 1e3 / (nadj * R), flop / (np.median(tn) * 1e-3) / 1e12), flush=True)
    print('  cn_change_prob, the same adjacencies:   k_region_prob %s; wall %s; k_region_prob / path_entropy stream %.2f' % (
        fmt(tk), fmt(wo), np.median(tk) / np.median(tn)), flush=True)
    out = posteriors.batch_path_entropy(b, 0, R, None, *maps)
    print('  genome, per restart: path entropy %s nats' % np.array2string(out['path_entropy'][:, 0], precision=3), flush=True)
    print('  genome, restart 0: sum of marginal entropies %.4f, path entropy %.4f, total correlation %.4f, inserted slack %.3e' % (
        out['marginal_entropy_sum'][0, 0], out['path_entropy'][0, 0], out['total_correlation'][0, 0], out['inserted_slack'][0, 0]), flush=True)
    # the sample route, ONE restart, the longest chain
    c = int(np.argmax(ce - cs))
    a, z = int(cs[c]), int(ce[c])
    er = posteriors.entropy_runs(marg[0], step[0], [(a, z)], orig)
    ts = []
    for rep in range(max(2, REPS // 2)):
        b.synchronize()
        t0 = time.perf_counter()
        st = b.sample_states(0, 1, NS, [rep])
        q = np.array([[a, z, -1, k] for k in range(NS)], dtype=np.int32)
        lq = b.call_logprob_raw(0, 1, st, q, None, orig)[0]
        est, se = -lq.mean(), lq.std(ddof=1) / np.sqrt(NS)
        ts.append((time.perf_counter() - t0) * 1e3)
    st = None
    print('  4 096 samples of ONE restart + rmx_call_prob over the longest chain (%d model segments): wall %s; times 16 restarts %.0f ms = x%.0f of the call\'s wall; '
          '-mean log q %.4f +- %.4f against the exact %.4f (slack %.2e)' % (z - a + 1, fmt(ts), 16 * np.median(ts), 16 * np.median(ts) / np.median(wn), est, se,
                                                                         er['path_entropy'][0], er['inserted_slack'][0]), flush=True)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.array([[x, max(x, min(y - 1, int(np.flatnonzero(chain == chain[x])[-1])))] for x, y in zip(edges[:-1], edges[1:])])
    t0 = time.perf_counter()
    ar = posteriors.batch_path_entropy(b, 0, 1, arms, *maps)
    print('  46 arm-sized regions of restart 0 (device call + prefix sums: %.1f ms); the ten most uncertain:' % ((time.perf_counter() - t0) * 1e3))
    print('    %-18s %12s %12s %12s %14s %12s' % ('region', 'entropy', 'slack', 'total corr.', 'perplexity', 'per segment'))
    for i in np.argsort(-ar['path_entropy'][0])[:10]:
        print('    [%6d, %6d]   %12.5f %12.3e %12.5f %14.3e %12.3e' % (arms[i, 0], arms[i, 1], ar['path_entropy'][0, i], ar['inserted_slack'][0, i],
                                                                     ar['total_correlation'][0, i], ar['perplexity'][0, i], ar['entropy_per_segment'][0, i]), flush=True)
    rs.close()
