"""Region alternatives (k_region_kbest) of all 16 restarts of the bench workload (50 000 segments in 23 chains, one RestartSet) at 165
and 355 states, after one variational sweep, in one process, beside k_region_decode on identical queries.  The three workloads of
tools/region_decode_time.py: every adjacency (the 'state' label over a pair), 20 000 regions of one to three segments and 46
arm-sized regions (the seven events of posteriors.REGION_EVENTS each).  k_region_kbest has no profile id, so both calls are timed
the same way: HIP events on the batch's stream around the whole call (rmx_timer_start / rmx_timer_stop: the launches of every chunk
and the copies of queries and results between them); k_region_decode's kernel time from rmx_profile_get stands beside it.  Per
workload the calls alternate -- decode, then K = 1, 2, 4, 8 -- REPS times after a warm-up of each; medians and spreads are printed,
and the ratio of every K to the decode call.  Rank 0 of every K is compared with the decode result bit for bit on the way.
Two more workloads separate the exp(trans_value) branch, which has no cross-lane merge of lists: every breakend adjacency as a
two-segment run, and as many plain adjacencies, spread evenly, as two-segment runs (no constraint) -- one backward step each, of the
one kind or the other.
With --count the tool runs an instrumented build instead (-DRMX_KBEST_COUNT, built into tools/tmp/ on first use and kept out of the
library; it times nothing): per workload and K the (s, s') pairs the list passes met and the (s', j) candidates they evaluated,
counted on the device, and their ratio, the mean number of candidates per pair.
Then, over 500 small regions without a constraint: the coverage (the sum of the K probabilities) at each K, and how often the K most
frequent configurations among 4 096 posterior samples are the exact K-list (as a set, and in order).
Usage: python tools/region_alternatives_time.py [--count] [--samples K] [--reps N] [MAXCN ...]
(default 4096 samples, 5 repeats; 8 12: 165 and 355 states)"""
import sys, os, time, subprocess
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
COUNT = '--count' in sys.argv[1:]
if COUNT:
    import ctypes as C
    from remixt_amd import _lib
    src = [os.path.join(ROOT, 'remixt_amd', 'csrc', f) for f in ('rmx_api.hip', 'rmx_kernels.h', 'rmx_device.h', 'rmx_host.h')]
    _lib.LIB_PATH = os.path.join(ROOT, 'tools', 'tmp', 'lib_kbest_count.so')
    if not os.path.exists(_lib.LIB_PATH) or any(os.path.getmtime(f) > os.path.getmtime(_lib.LIB_PATH) for f in src):
        os.makedirs(os.path.dirname(_lib.LIB_PATH), exist_ok=True)
        subprocess.check_call([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-Wno-unused-result',
                               '-Wno-unused-value', '-DRMX_KBEST_COUNT', '-o', _lib.LIB_PATH, src[0]])
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK = 16, 64
KS = (1, 2, 4, 8)
args = [a for a in sys.argv[1:] if a != '--count']
NSAMP, REPS = 4096, 5
while args and args[0] in ('--samples', '--reps'):
    if args[0] == '--samples':
        NSAMP = int(args[1])
    else:
        REPS = int(args[1])
    args = args[2:]


def stream_ms(b, fn):
    b.synchronize()
    b.timer_start()
    t0 = time.perf_counter(); out = fn(); wall = time.perf_counter() - t0
    return b.timer_stop(), wall * 1e3, out


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
    # one backward step of one kind: every breakend adjacency of the model, and as many plain ones (model segments: `runs` below)
    inner = np.ones(N1 - 1, dtype=bool); inner[ce[:-1]] = False
    bidx = np.asarray(m.breakpoint_idx)
    be, plain = np.flatnonzero(inner & (bidx[:-1] >= 0)), np.flatnonzero(inner & (bidx[:-1] < 0))
    plain = plain[np.linspace(0, len(plain) - 1, len(be)).astype(int)]
    workloads = [('every adjacency', posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)[0], [(None, 'state')]),
                 ('20 000 regions of 1-3 segments', small, events), ('46 arm-sized regions', arms, events),
                 ('%d breakend adjacencies (exp(trans_value) steps)' % len(be), be, None), ('%d plain adjacencies (Wb steps)' % len(plain), plain, None)]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts' % (S, N, N1, len(cs), R), flush=True)
    for name, regions, variants in workloads:
        if variants is None:      # (model adjacencies n -> n + 1, as they are)
            runs, constrain, variants = np.stack([regions, regions + 1], axis=1).astype(np.int32), np.asarray(m.seg_is_original, dtype=np.uint8), [(None, None)]
        else:
            runs, _, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
        q = queries(runs, variants)
        L = (q[:, 1] - q[:, 0] + 1).astype(np.int64)
        steps = int((L - 1).sum()) * R
        dec = lambda: b.region_decode_raw(0, R, q, masks, labels, constrain)
        kb = dict((K, (lambda K=K: b.region_kbest_raw(0, R, q, K, masks, labels, constrain))) for K in KS)
        if COUNT:
            cnt = (C.c_uint64 * 2)()
            for K in KS:
                b._lib.rmx_kbest_counts(b._handle, cnt, 1)
                kb[K]()
                b._lib.rmx_kbest_counts(b._handle, cnt, 1)
                print("  %s: K %d: %d (s, s') pairs met, %d (s', j) candidates evaluated: %.4f per pair (counted on the device)" % (
                    name, K, cnt[0], cnt[1], cnt[1] / float(max(cnt[0], 1))), flush=True)
            continue
        best, states = dec()
        for K in KS:                                   # (warm-up of each; rank 0 against the decode, bit for bit)
            lp, st = kb[K]()
            same = np.array_equal(lp[:, :, 0], best, equal_nan=True) and np.array_equal(st[:, :, 0], states)
            print('  %s: K %d rank 0 %s k_region_decode bit for bit; %d of %d ranks finite' % (name, K, 'equals' if same else 'DIFFERS FROM', int(np.isfinite(lp).sum()), lp.size), flush=True)
            del lp, st
        td, tk, kd = [], dict((K, []) for K in KS), []
        for rep in range(REPS):
            b.profile_reset(); b.profile_enable(1)
            ms, wall, _ = stream_ms(b, dec); td.append(ms)
            kd.append(b.profile().get('k_region_decode', (0., 0))[0]); b.profile_enable(0)
            for K in KS:
                ms, wall, _ = stream_ms(b, kb[K]); tk[K].append(ms)
        print('  %s: %d (restart, query) pairs, %d backward steps, longest run %d: rmx_region_decode call on the stream %s, of it k_region_decode %s; %.3f us per step' % (
            name, len(q) * R, steps, int(L.max()), fmt(td), fmt(kd), np.median(td) * 1e3 / max(steps, 1)), flush=True)
        for K in KS:
            print('    rmx_region_kbest K %d: call on the stream %s; %.3f us per step; x%.3f of the decode call' % (
                K, fmt(tk[K]), np.median(tk[K]) * 1e3 / max(steps, 1), np.median(tk[K]) / np.median(td)), flush=True)
    if COUNT:
        rs.close()
        continue
    # coverage, and the sample route: the K most frequent of NSAMP sampled configurations against the exact list
    runs, piece_region, constrain = posteriors.region_queries(small, m.seg_fwd_remap, m.seg_is_original, cs, ce)
    whole = np.flatnonzero(np.bincount(piece_region, minlength=len(small)) == 1)      # (regions of one piece)
    sel = np.flatnonzero(np.isin(piece_region, whole))[:500]
    runs = runs[sel]
    q = queries(runs, [(None, None)])
    logp, states = b.region_kbest_raw(0, R, q, 8, None, None, None)
    Lmax = states.shape[3]
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    cols = np.minimum(runs[:, :1] + np.arange(Lmax)[None], runs[:, 1:2])              # (past the run: its last segment again)
    place = (np.int64(S) ** np.arange(Lmax)).astype(np.int64)
    keys = np.zeros((R, NSAMP, len(runs)), dtype=np.int64)
    for k0 in range(0, NSAMP, CHUNK):
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])
        keys[:, k0:k0 + CHUNK] = (st[:, :, cols].astype(np.int64) * place).sum(axis=3)
    last = np.broadcast_to((runs[:, 1] - runs[:, 0])[None, :, None, None], states.shape[:3] + (1,))
    exact = (np.where(states >= 0, states, np.take_along_axis(states, last, axis=3)).astype(np.int64) * place).sum(axis=3)      # (R, regions, 8)
    for K in KS:
        cov = np.exp(logp[:, :, :K]).sum(axis=2)
        as_set = in_order = full = 0
        for r in range(R):
            for i in range(len(runs)):
                if not np.isfinite(logp[r, i, :K]).all():
                    continue
                full += 1
                vals, counts = np.unique(keys[r, :, i], return_counts=True)
                top = vals[np.argsort(-counts, kind='stable')[:K]]
                as_set += int(len(top) == K and set(top) == set(exact[r, i, :K]))
                in_order += int(len(top) == K and np.array_equal(top, exact[r, i, :K]))
        print('  K %d over %d regions of 1-3 segments x %d restarts, no constraint: coverage mean %.6f, median %.6f, min %.4f; the %d most frequent of %d sampled '
              'configurations are the exact list as a set in %d, in order in %d of the %d pairs with K exact configurations' % (
                  K, len(runs), R, cov.mean(), np.median(cov), cov.min(), K, NSAMP, as_set, in_order, full), flush=True)
    rs.close()
