"""Region event probabilities (k_region_prob) of all 16 restarts of the bench workload (50 000 segments, one RestartSet) at 165 and
355 states, after one variational sweep, in one process.  Three workloads: every adjacency (cn_change_prob), region_events over
20 000 regions of one to three segments, region_events over 46 arm-sized regions.  Per workload: the device time of the kernel from
rmx_profile_get beside its floors (computed below from the shapes), and the wall time of the call.  Then the route without the
kernel: 4 096 posterior samples per restart (sample_states, 64 at a time) and the "no change" events of the same runs counted on
them in numpy -- the masks' events would cost that route more.
Usage: python tools/region_time.py [--samples K] [MAXCN ...]   (default 4096 samples; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK = 16, 64
HBM, L2, FP64 = 6.0e12, 34.5e12, 78.6e12      # measured sweep rate, aggregate L2 rate, FP64 vector peak (data sheet)
args = sys.argv[1:]
K = 4096
if args and args[0] == '--samples':
    K = int(args[1]); args = args[2:]


def floors(runs, nvariants, S):
    """(restart, query) pairs, backward steps, and the three floors in ms: fa / post rows from HBM, 4 S^2 flop per step on the FP64
    vector pipe, and the 2 S^2 weights a step of a workgroup reads from L2 (nothing is shared between workgroups)."""
    pairs = len(runs) * nvariants * R
    steps = int((runs[:, 1] - runs[:, 0]).sum()) * nvariants * R
    rows = (steps + pairs) * S * 8
    return pairs, steps, rows / HBM * 1e3, steps * 4. * S * S / FP64 * 1e3, steps * 2. * S * S * 8 / L2 * 1e3


def timed(b, fn):
    fn()
    wall = []
    for rep in range(3):
        t0 = time.perf_counter(); fn(); wall.append(time.perf_counter() - t0)
    b.profile_reset(); b.profile_enable(1)
    fn()
    ms, n = b.profile().get('k_region_prob', (0., 0)); b.profile_enable(0)
    return np.median(wall) * 1e3, ms, n


def all_equal(eq, runs):
    """eq (..., N1 - 1 + 1) with a trailing column of ones: whether every adjacency of each run [a, b] holds equal states."""
    idx = np.stack([runs[:, 0], runs[:, 1]], axis=1).ravel()      # reduce over [a, b), then a throw-away [b, next a)
    out = np.minimum.reduceat(eq, idx, axis=-1)[..., ::2]
    return np.where(runs[:, 1] > runs[:, 0], out, 1)


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    rng = np.random.RandomState(0)
    first = rng.randint(0, N - 3, size=20000)
    small = np.stack([first, first + rng.randint(0, 3, size=20000)], axis=1)
    edges = np.linspace(0, N, 47).astype(int)
    arms = np.stack([edges[:-1], edges[1:] - 1], axis=1)
    workloads = [('every adjacency', posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)[0], 1, rs.cn_change_prob),
                 ('20 000 regions of 1-3 segments', small, len(posteriors.REGION_EVENTS), lambda: rs.region_events(small)),
                 ('46 arm-sized regions', arms, len(posteriors.REGION_EVENTS), lambda: rs.region_events(arms))]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts' % (S, N, N1, len(cs), R), flush=True)
    pieces = []
    for name, regions, nvar, fn in workloads:
        runs = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)[0].astype(np.int64)
        pieces.append(runs)
        pairs, steps, f_hbm, f_flop, f_l2 = floors(runs, nvar, S)
        wall, ms, n = timed(b, fn)
        print('  %-31s %8d (restart, query) pairs, %9d steps: k_region_prob %9.3f ms device over %d launches; floors %.3f ms (rows / 6.0 TB/s), '
              '%.3f ms (4 S^2 flop per step / 78.6 TF), %.3f ms (2 S^2 weights per step / 34.5 TB/s of L2: this shape\'s own, x%.2f); call %.1f ms wall' % (
                  name + ':', pairs, steps, ms, n, f_hbm, f_flop, f_l2, ms / f_l2 if f_l2 else float('nan'), wall), flush=True)
    # the same events from posterior samples
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    b.sample_states(0, R, CHUNK, seeds)
    t_draw = t_count = 0.
    counts = [np.zeros((R, len(runs))) for runs in pieces]
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
        t1 = time.perf_counter()
        eq = np.ones(st.shape[:2] + (N1,), dtype=np.uint8)
        np.equal(st[:, :, :-1], st[:, :, 1:], out=eq[:, :, :-1], casting='unsafe')
        for c, runs in zip(counts, pieces):
            c += all_equal(eq, runs).sum(axis=1)
        t_draw += t1 - t0; t_count += time.perf_counter() - t1
    print('  sample route, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall + counting the no-change events of the three '
          'workloads in numpy %.0f ms = %.0f ms' % (K, R, CHUNK, t_draw * 1e3, t_count * 1e3, (t_draw + t_count) * 1e3), flush=True)
    exact = 1. - rs.cn_change_prob()
    est = counts[0] / K
    joined = ~np.isnan(exact)
    err = np.abs(est - exact[:, joined[0]])
    print('  every adjacency: |sample estimate - exact| max %.3e, mean %.3e (1 / sqrt(K) = %.3e)' % (err.max(), err.mean(), K ** -0.5), flush=True)
    rs.close()
