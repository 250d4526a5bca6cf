"""Call probabilities (k_call_prob) of all 16 restarts of the bench workload (50 000 segments, 23 chains, one RestartSet) at 165 and
355 states, after one variational sweep, in one process.  Three workloads, each against the restarts' decoded paths:
  (a) 20 000 regions of one to three segments x the three labels of posteriors.CALL_LABELS;
  (b) 46 arm-sized regions x the three labels;
  (c) the whole-genome log-probability of the decoded path and of 64 sampled paths per restart (posteriors.batch_cn_logprob).
Per workload: the device time of k_call_prob from rmx_profile_get and the wall time of the raw call.  Beside (a) and (b): k_region_prob
on the same runs with a one-state mask (the decoded state of restart 0 at the run's last segment) -- the nearest existing kernel; it
stops a run whose mass reaches 0, so the share of its results that are -inf is printed with its time.  Then the route without the
kernel: 4 096 posterior samples per restart (sample_states, 64 at a time) and the agreement with the decoded path over the runs of
(a) and (b) counted on them in numpy.
Usage: python tools/call_time.py [--samples K] [--count K2] [MAXCN ...]   (default 4096 samples, all of them counted -- K2 < K counts the
first K2 only, the numpy part being the slow one; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK, NPATHS = 16, 64, 64
args = sys.argv[1:]
K, K2 = 4096, None
while args and args[0] in ('--samples', '--count'):
    if args[0] == '--samples':
        K = int(args[1])
    else:
        K2 = int(args[1])
    args = args[2:]
K2 = K if K2 is None else min(K, K2)


def timed(b, fn, kernel):
    fn()
    wall = []
    for rep in range(3):
        t0 = time.perf_counter(); fn(); wall.append(time.perf_counter() - t0)
    b.profile_reset(); b.profile_enable(1)
    fn()
    ms, n = b.profile().get(kernel, (0., 0)); b.profile_enable(0)
    return np.median(wall) * 1e3, ms, n


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    _, labels = posteriors.event_tables(b.cn_classes)
    lis = [posteriors.LABEL_NAMES.index(lb) for _, lb in posteriors.CALL_LABELS]
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    decoded = rs._call_states(None)                                       # (R, N1)
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 3, size=20000)
    small = np.stack([first, first + rng.randint(0, 3, size=20000)], axis=1)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.stack([edges[:-1], edges[1:] - 1], axis=1)
    workloads = [('(a) 20 000 regions of 1-3 segments', small), ('(b) 46 arm-sized regions', arms)]
    one_state = np.broadcast_to(np.eye(S, dtype=np.uint8)[None], (b.cn_classes.shape[0], S, S)).copy()      # mask i: state i alone
    print('%d states, %d segments (%d in the model), %d chains, %d restarts' % (S, N, N1, len(cs), R), flush=True)
    pieces, exact = [], []
    for name, regions in workloads:
        runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
        q = np.concatenate([np.concatenate([runs, np.full((len(runs), 1), li), np.zeros((len(runs), 1), dtype=int)], axis=1) for li in lis]).astype(np.int32)
        pieces.append(runs.astype(np.int64))
        steps = int((runs[:, 1] - runs[:, 0]).sum()) * R * len(lis)
        wall, ms, n = timed(b, lambda: b.call_logprob_raw(0, R, decoded[:, None], q, labels, constrain), 'k_call_prob')
        lp = b.call_logprob_raw(0, R, decoded[:, None], q, labels, constrain)
        exact.append(np.exp(lp.reshape(R, len(lis), len(runs))))
        # the nearest existing kernel on the same runs, once per label as well (three times the queries)
        q1 = np.concatenate([runs, decoded[0][runs[:, 1]][:, None], np.full((len(runs), 1), -1)], axis=1).astype(np.int32)
        q1 = np.concatenate([q1] * len(lis))
        wall1, ms1, n1 = timed(b, lambda: b.region_logprob_raw(0, R, q1, one_state, None, constrain), 'k_region_prob')
        dead = np.mean(b.region_logprob_raw(0, R, q1, one_state, None, constrain) == -np.inf)
        print('  %-36s %8d (restart, query) pairs, %9d steps: k_call_prob %9.3f ms device over %d launches, call %.1f ms wall; k_region_prob with a '
              'one-state mask %9.3f ms device, call %.1f ms wall (%.0f %% of its results -inf: stopped early); k_region_prob / k_call_prob x%.2f device, x%.2f wall' % (
                  name + ':', len(q) * R, steps, ms, n, wall, ms1, wall1, 100 * dead, ms1 / ms if ms else float('nan'), wall1 / wall), flush=True)
    # (c) whole-genome log q of the decoded path and of 64 sampled paths per restart
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    paths = np.concatenate([decoded[:, None], b.sample_states(0, R, NPATHS, seeds)], axis=1)      # (R, 65, N1)
    fn = lambda: posteriors.batch_cn_logprob(b, 0, R, paths, m.seg_is_original, m.is_telomere)
    wall, ms, n = timed(b, fn, 'k_call_prob')
    lq = fn()
    print('  %-36s %8d (restart, query) pairs, %9d steps: k_call_prob %9.3f ms device over %d launches, batch_cn_logprob %.1f ms wall; log q of the '
          'decoded path %.1f .. %.1f, of the samples %.1f .. %.1f' % ('(c) whole genome, 1 + %d paths:' % NPATHS, R * paths.shape[1] * len(cs),
                                                                    R * paths.shape[1] * (N1 - len(cs)), ms, n, wall, lq[:, 0].min(), lq[:, 0].max(),
                                                                    lq[:, 1:].min(), lq[:, 1:].max()), flush=True)
    print('  the decoded path is the mode of them: %s' % bool((lq[:, :1] >= lq[:, 1:] - N1 * 1e-9).all()), flush=True)
    del paths
    # the same probabilities from posterior samples: agreement with the decoded path, per label, over the runs of (a) and (b)
    orig = np.asarray(m.seg_is_original, dtype=bool)
    lut = [labels[0, li] for li in lis]                                   # (one state class here)
    assert b.cn_classes.shape[0] == 1
    b.sample_states(0, R, CHUNK, seeds)
    t_draw = t_count = 0.
    hits = [np.zeros((R, len(lis), len(runs))) for runs in pieces]
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
        t1 = time.perf_counter()
        t_draw += t1 - t0
        if k0 >= K2:
            continue
        for j, tab in enumerate(lut):
            miss = np.zeros(st.shape[:2] + (N1 + 1,), dtype=np.int32)     # cumulative disagreements at real segments, a leading 0
            np.cumsum((tab[st] != tab[decoded][:, None]) & orig, axis=2, out=miss[:, :, 1:])
            for h, runs in zip(hits, pieces):
                h[:, j] += (miss[:, :, runs[:, 1] + 1] == miss[:, :, runs[:, 0]]).sum(axis=1)
        t_count += time.perf_counter() - t1
    print('  sample route, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall; counting the agreement of the first %d over (a) and (b) '
          'for three labels in numpy %.0f ms' % (K, R, CHUNK, t_draw * 1e3, K2, t_count * 1e3), flush=True)
    for (name, _), h, p in zip(workloads, hits, exact):
        err = np.abs(h / K2 - p)
        print('  %s: |sample estimate - exact| max %.3e, mean %.3e (1 / sqrt(%d) = %.3e)' % (name, err.max(), err.mean(), K2, K2 ** -0.5), flush=True)
    rs.close()
