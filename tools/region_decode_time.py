"""Region decode (k_region_decode) of all 16 restarts of the bench workload (50 000 segments in 23 chains, one RestartSet) at 165 and
355 states, after one variational sweep, in one process, beside k_region_prob on identical queries.  The three workloads of
tools/region_time.py: every adjacency (the 'state' label over a pair), 20 000 regions of one to three segments and 46 arm-sized
regions (the seven events of posteriors.REGION_EVENTS each).  Per workload: the device time of both kernels from rmx_profile_get,
the calls alternating, REPS times each after a warm-up of both, so that the spread between repeats stands beside the ratio; the
time per backward step; the launches (a decode call runs in chunks: its back-pointer strips, max_len S int16 per (restart, query),
stay within 1 GiB); the wall time of the calls.  The two kernels share the D pass; the decode's second pass trades the fused
multiply-add for a multiply, a compare and two selects, writes 2 S bytes of back-pointers per step, and ends with a trace of L
dependent loads by one thread.
Then the sample route: how often the modal configuration of K posterior samples (sample_states, 64 at a time) equals the exact
most probable one, over the small regions without a constraint -- and how many distinct configurations the samples hold.
Usage: python tools/region_decode_time.py [--samples K] [--reps N] [MAXCN ...]
(default 4096 samples, 5 repeats; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK = 16, 64
args = sys.argv[1:]
K, REPS = 4096, 5
while args and args[0] in ('--samples', '--reps'):
    if args[0] == '--samples':
        K = int(args[1])
    else:
        REPS = int(args[1])
    args = args[2:]


def device_ms(b, fn, kernel):
    b.profile_reset(); b.profile_enable(1)
    t0 = time.perf_counter(); out = fn(); wall = time.perf_counter() - t0
    ms, n = b.profile().get(kernel, (0., 0)); b.profile_enable(0)
    return ms, n, wall * 1e3, out


def fmt(v):
    return ' '.join('%.3f' % x for x in v) + ' ms (median %.3f, spread %.1f %%)' % (np.median(v), 100. * (max(v) - min(v)) / np.median(v))


def queries(runs, variants):
    q = np.zeros((len(variants), len(runs), 4), dtype=np.int32)
    q[:, :, :2] = runs[None]
    for e, (mask, label) in enumerate(variants):
        q[e, :, 2] = -1 if mask is None else posteriors.MASK_NAMES.index(mask)
        q[e, :, 3] = -1 if label is None else posteriors.LABEL_NAMES.index(label)
    return q.reshape(-1, 4)


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    masks, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 3, size=20000)
    small = np.stack([first, first + rng.randint(0, 3, size=20000)], axis=1)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.stack([edges[:-1], edges[1:] - 1], axis=1)
    events = [(mask, label) for _, mask, label, _ in posteriors.REGION_EVENTS]
    workloads = [('every adjacency', posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)[0], [(None, 'state')]),
                 ('20 000 regions of 1-3 segments', small, events), ('46 arm-sized regions', arms, events)]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts' % (S, N, N1, len(cs), R), flush=True)
    for name, regions, variants in workloads:
        runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
        q = queries(runs, variants)
        L = (q[:, 1] - q[:, 0] + 1).astype(np.int64)
        steps = int((L - 1).sum()) * R
        prob = lambda: b.region_logprob_raw(0, R, q, masks, labels, constrain)
        dec = lambda: b.region_decode_raw(0, R, q, masks, labels, constrain)
        total, (best, states) = prob(), dec()                      # (warm-up of both; and the maximum is not above the sum)
        # the maximum is not above the sum -- where the event's probability is inside the range of the scaled rows: far below it
        # (log P(E) < -700) states flush to 0 in both kernels, at different steps under a sum scale and a maximum scale
        fin = np.isfinite(best) & np.isfinite(total)
        with np.errstate(invalid='ignore'):
            over = (best - total) / (L[None] * 1e-9)
        inside, deep = fin & (total > -700.), fin & (total <= -700.)
        print('  %s: (log P* - log P(E)) / (L 1e-9): max %.3e over the %d results with log P(E) > -700, max %.3e over the %d below; finite in one kernel alone: %d' % (
            name, over[inside].max() if inside.any() else 0., inside.sum(), over[deep].max() if deep.any() else 0., deep.sum(),
            int((np.isfinite(best) != np.isfinite(total)).sum())), flush=True)
        td, wd, tp, wp = [], [], [], []
        for rep in range(REPS):
            ms, nd, wall, _ = device_ms(b, dec, 'k_region_decode'); td.append(ms); wd.append(wall)
            ms, np_, wall, _ = device_ms(b, prob, 'k_region_prob'); tp.append(ms); wp.append(wall)
        print('  %s: %d (restart, query) pairs, %d backward steps, longest run %d, %d of the results finite: k_region_decode %s over %d launches, call %.1f ms wall; '
              '%.3f us per step; k_region_prob on the same queries %s over %d launches, call %.1f ms wall; %.3f us per step; decode / prob x%.3f device' % (
                  name, len(q) * R, steps, int(L.max()), int(fin.sum()), fmt(td), nd, np.median(wd), np.median(td) * 1e3 / max(steps, 1),
                  fmt(tp), np_, np.median(wp), np.median(tp) * 1e3 / max(steps, 1), np.median(td) / np.median(tp)), flush=True)
    # the sample route: the modal configuration of K samples per restart against the exact one, small regions, no constraint
    runs, piece_region, constrain = posteriors.region_queries(small, m.seg_fwd_remap, m.seg_is_original, cs, ce)
    whole = np.flatnonzero(np.bincount(piece_region, minlength=len(small)) == 1)      # (regions of one piece)
    sel = np.flatnonzero(np.isin(piece_region, whole))[:500]
    runs = runs[sel]
    q = queries(runs, [(None, None)])
    best, states = b.region_decode_raw(0, R, q, None, None, None)
    Lmax = states.shape[2]
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    b.sample_states(0, R, CHUNK, seeds)
    cols = np.minimum(runs[:, :1] + np.arange(Lmax)[None], runs[:, 1:2])              # (past the run: its last segment again)
    place = (np.int64(S) ** np.arange(Lmax)).astype(np.int64)
    keys = np.zeros((R, K, len(runs)), dtype=np.int64)
    t_draw = 0.
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])
        t_draw += time.perf_counter() - t0
        keys[:, k0:k0 + CHUNK] = (st[:, :, cols].astype(np.int64) * place).sum(axis=3)
    exact = (np.where(states >= 0, states, np.take_along_axis(states, np.broadcast_to((runs[:, 1] - runs[:, 0])[None, :, None], states.shape[:2] + (1,)), axis=2)).astype(np.int64) * place).sum(axis=2)
    t0 = time.perf_counter()
    hit = distinct = 0
    for r in range(R):
        for i in range(len(runs)):
            vals, counts = np.unique(keys[r, :, i], return_counts=True)
            hit += int(vals[np.argmax(counts)] == exact[r, i]); distinct += len(vals)
    t_count = time.perf_counter() - t0
    print('  sample route, %d samples x %d restarts in chunks of %d over %d regions of 1-3 segments (up to %d model segments), no constraint: the modal sampled '
          'configuration equals the exact one in %d of %d (restart, region) pairs (%.2f %%); %.1f distinct configurations per pair on average; exact P* median %.4f, '
          'min %.4f; sample_states %.0f ms wall, counting in numpy %.0f ms' % (
              K, R, CHUNK, len(runs), Lmax, hit, R * len(runs), 100. * hit / (R * len(runs)), distinct / float(R * len(runs)), np.exp(np.median(best)), np.exp(best.min()),
              t_draw * 1e3, t_count * 1e3), flush=True)
    rs.close()
