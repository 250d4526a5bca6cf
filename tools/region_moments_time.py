"""Region moments (k_region_moments) of all 16 restarts of the bench workload (50 000 segments, one RestartSet) at 165 and 355 states,
after one variational sweep, in one process.  The three workloads of tools/region_counts_time.py: every adjacency pair, 20 000 regions
of one to three segments, 46 arm-sized regions; each asked for the four fraction features (nf = 4: 14 outputs) under length weights.
Per workload: the device time of k_region_moments from rmx_profile_get and the wall time of the raw call, beside k_region_counts at 16
bins on the same runs -- the calls alternate, REPS times each, so the spread between repeats of the same call stands beside the ratio --
and the two floors from the sizes: 2 S^2 weights per step of a workgroup from L2, and one v_mfma_f64_16x16x4_f64 per (16 states, four
s') on the matrix cores.  Then the route without the kernel: 4 096 posterior samples per restart (sample_states, 64 at a time), before
any host averaging, and the sample estimate of the arm-sized regions' moments beside the exact ones.
Usage: python tools/region_moments_time.py [--samples K] [--reps N] [MAXCN ...]   (default 4096 samples, 3 repeats; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK, BINS, NF = 16, 64, 16, 4
L2 = 34.5e12      # aggregate L2 rate
MFMA64 = 78.6e12  # dense FP64 matrix rate (flop / s)
args = sys.argv[1:]
K, REPS = 4096, 3
while args and args[0] in ('--samples', '--reps'):
    if args[0] == '--samples':
        K = int(args[1])
    else:
        REPS = int(args[1])
    args = args[2:]


def device_ms(b, fn, kernel):
    b.profile_reset(); b.profile_enable(1)
    t0 = time.perf_counter(); fn(); wall = time.perf_counter() - t0
    ms, n = b.profile().get(kernel, (0., 0)); b.profile_enable(0)
    return ms, n, wall * 1e3


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    _, labels = posteriors.event_tables(b.cn_classes)
    li = posteriors.LABEL_NAMES.index('state')
    feats = posteriors.moment_features(b.cn_classes)
    M = feats.shape[1] - NF
    weights = np.asarray(m.l1, dtype=float)[None]
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 3, size=20000)
    small = np.stack([first, first + rng.randint(0, 3, size=20000)], axis=1)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.stack([edges[:-1], edges[1:] - 1], axis=1)
    workloads = [('every adjacency', posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)[0]), ('20 000 regions of 1-3 segments', small),
                 ('46 arm-sized regions', arms)]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts; nf = %d (14 columns) against %d bins' % (S, N, N1, len(cs), R, NF, BINS), flush=True)
    arm_exact = None
    for name, regions in workloads:
        runs, piece_region, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
        qm = np.concatenate([runs, np.full((len(runs), 1), M), np.zeros((len(runs), 1))], axis=1).astype(np.int32)
        qc = np.concatenate([runs, np.full((len(runs), 1), -1), np.full((len(runs), 1), li)], axis=1).astype(np.int32)
        steps = int((runs[:, 1] - runs[:, 0]).sum()) * R
        f_l2 = steps * 2. * S * S * 8 / L2 * 1e3
        tiles = (S + 15) // 16
        f_mm = steps * tiles * ((S + 3) // 4) * (2. * 16 * 16 * 4) / MFMA64 * 1e3
        moments = lambda: b.region_moments_raw(0, R, qm, feats, weights, NF)
        counts = lambda: b.region_counts_raw(0, R, qc, None, labels, constrain, BINS)
        moments(); counts()
        tm, tc, wm, wc = [], [], [], []
        for rep in range(REPS):      # (alternating: both see the same clocks and cache state)
            ms, n, wall = device_ms(b, moments, 'k_region_moments'); tm.append(ms); wm.append(wall)
            ms, nc, wall = device_ms(b, counts, 'k_region_counts'); tc.append(ms); wc.append(wall)
        tm, tc = np.array(tm), np.array(tc)
        print('  %-31s %8d (restart, query) pairs, %9d steps: k_region_moments %s ms device (median %.3f, spread %.1f %%) over %d launches, call %.1f ms wall; '
              'k_region_counts %s ms device (median %.3f, spread %.1f %%), call %.1f ms wall; moments / counts x%.2f; floors: 2 S^2 weights per step / 34.5 TB/s '
              'of L2 %.3f ms (x%.2f), one matrix instruction per (tile, four s\') / 78.6 Tflop/s %.3f ms' % (
                  name + ':', len(qm) * R, steps, ' '.join('%.3f' % t for t in tm), np.median(tm), 100 * (tm.max() - tm.min()) / np.median(tm) if np.median(tm) else 0., n,
                  np.median(wm), ' '.join('%.3f' % t for t in tc), np.median(tc), 100 * (tc.max() - tc.min()) / np.median(tc) if np.median(tc) else 0., np.median(wc),
                  np.median(tm) / np.median(tc) if np.median(tc) else float('nan'), f_l2, np.median(tm) / f_l2 if f_l2 else float('nan'), f_mm), flush=True)
        if regions is arms:
            arm_exact = (runs.astype(np.int64), piece_region, posteriors.combine_moments(moments(), piece_region, len(arms)))
    # the sample route to the same numbers: the draws alone (the bar), then the arm-sized regions' moments from them
    if K <= 0:      # (--samples 0: the kernels alone)
        rs.close()
        continue
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    b.sample_states(0, R, CHUNK, seeds)
    runs, piece_region, exact = arm_exact
    fseg = feats[b.seg_class][:, M:]                      # (N1, 4, S)
    Fs = np.zeros((R, K, len(arms), NF))
    t_draw = t_host = 0.
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
        t1 = time.perf_counter()
        for f in range(NF):
            v = weights[0][None, None, :] * fseg[np.arange(N1)[None, None, :], f, st]
            c = np.concatenate([np.zeros(v.shape[:2] + (1,)), np.cumsum(v, axis=2)], axis=2)
            np.add.at(Fs[:, k0:k0 + CHUNK, :, f], (Ellipsis, piece_region), c[..., runs[:, 1] + 1] - c[..., runs[:, 0]])
        t_draw += t1 - t0; t_host += time.perf_counter() - t1
    print('  sample route, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall (the bar), + the weighted sums of the arm-sized regions '
          'in numpy %.0f ms' % (K, R, CHUNK, t_draw * 1e3, t_host * 1e3), flush=True)
    sd = np.sqrt(np.maximum(exact[..., NF + np.array([0, 4, 7, 9])], 0.))
    big = sd > 0
    em = np.abs(Fs.mean(axis=1) - exact[..., :NF])[big] / sd[big]
    es = np.abs(Fs.std(axis=1) - sd)[big] / sd[big]
    print('  arm-sized regions: |sample mean - exact| / exact SD max %.3e, median %.3e; |sample SD - exact SD| / exact SD max %.3e, median %.3e '
          '(1 / sqrt(K) = %.3e)' % (em.max(), np.median(em), es.max(), np.median(es), K ** -0.5), flush=True)
    rs.close()
