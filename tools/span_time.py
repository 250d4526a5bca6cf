"""Region event spans (k_region_span) of all 16 restarts of the bench workload (50 000 segments in 23 chains, one RestartSet) at 165
and 355 states, after one variational sweep, in one process: 500 evenly spaced anchors, the 'total' label, windows of 16 and of 64 on
each side.  Per window: the device time of k_region_span from rmx_profile_get and the wall time of the raw call, beside the rows
route to the same table -- one rmx_region_extent call with wl + 1 queries per anchor, at anchors n0 - a with window (0, wl + wr) --
the calls alternating, REPS times each, so that the spread between repeats stands beside the ratio; the two tables compared entry by
entry; the time per matrix step, and the floor from the sizes: the 2 S^2 weights a step of a workgroup reads from L2.  Then the
sample route at the window of 16: posterior samples per restart (sample_states, 64 at a time) and the joint survival function of the
two ends of the constant-total run around each anchor counted on them in numpy.
Usage: python tools/span_time.py [--samples K] [--reps N] [MAXCN ...]
(default 512 samples, 3 repeats; 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, sampling, synthetic
from remixt_amd.restarts import RestartSet

R, CHUNK = 16, 64
L2 = 34.5e12      # aggregate L2 rate
args = sys.argv[1:]
K, REPS = 512, 3
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


for mcn in [int(a) for a in args] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b, m = rs.batch, rs.models[0]
    rs.variational_update(1); b.synchronize()
    N, N1, S = len(e.l), b.num_segments, b.num_cn_states
    masks, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    fwd = np.asarray(m.seg_fwd_remap, dtype=np.int64)
    constrain = np.ascontiguousarray(np.asarray(m.seg_is_original) != 0, dtype=np.uint8)
    anchors = np.linspace(0, N - 1, 500).astype(int)
    event = 'total'
    mi, li = posteriors.parse_event(event)
    q, _ = posteriors.extent_queries(anchors, event, fwd, constrain)
    n0 = q[:, 0].astype(np.int64)
    c = np.searchsorted(ce, n0, side='left')
    c0, c1 = cs[c], ce[c]
    print('%d states, %d segments (%d in the model), %d chains, %d restarts, %d anchors, event %s' % (S, N, N1, len(cs), R, len(anchors), event), flush=True)
    for w in (16, 64):
        # matrix steps of the new call: every column group walks from its top to the window's (or the chain's) left end
        msteps = 0
        for g in range(w // 16 + 1):
            top = np.minimum(n0 + min(w, 16 * g + 15), c1)
            msteps += int(np.where(top >= n0 + 16 * g, top - np.maximum(n0 - w, c0), 0).sum())
        msteps *= R
        floor = msteps * 2. * S * S * 8 / L2 * 1e3
        span = lambda: b.region_span_raw(0, R, q, masks, labels, constrain, w, w)
        # the rows route: anchors n0 - a inside the chain, window (0, 2 w)
        a_of = np.concatenate([np.full(int(min(w, n - lo)) + 1, i) for i, (n, lo) in enumerate(zip(n0, c0))])
        off = np.concatenate([np.arange(int(min(w, n - lo)) + 1) for n, lo in zip(n0, c0)])
        qr = np.stack([n0[a_of] - off, np.full(len(off), mi), np.full(len(off), li), np.zeros(len(off), dtype=np.int64)], axis=1).astype(np.int32)
        vsteps = int(np.minimum(2 * w, c1[a_of] - (n0[a_of] - off)).sum()) * R
        rows = lambda: b.region_extent_raw(0, R, qr, masks, labels, constrain, 0, 2 * w)
        span(); rows()
        ts, ws, tr, wr_ = [], [], [], []
        for rep in range(REPS):
            ms, n, wall, out = device_ms(b, span, 'k_region_span'); ts.append(ms); ws.append(wall)
            ms, nn, wall, ext = device_ms(b, rows, 'k_region_extent'); tr.append(ms); wr_.append(wall)
        got = np.full(out.shape, -np.inf)                      # the rows route's table: entry (a, c) is slot a + c of the query at n0 - a
        for cc in range(w + 1):
            got[:, a_of, off, cc] = ext[:, np.arange(len(off)), off + cc]
        fin = np.isfinite(got) & np.isfinite(out)
        near = fin & (np.where(fin, np.minimum(got, out), 0.) > -300.)
        bound = (np.arange(w + 1)[:, None] + np.arange(w + 1)[None, :] + 1) * 1e-9
        with np.errstate(invalid='ignore'):      # (-inf - -inf outside `near`)
            rel = np.where(near, np.abs(np.where(near, got - out, 0.)), 0.) / bound
        only_s, only_r = np.isneginf(out) & np.isfinite(got), np.isneginf(got) & np.isfinite(out)
        print('  window %d: %d (restart, query) pairs in %d column groups each, %d matrix steps: k_region_span %s over %d launches, call %.1f ms wall; '
              '%.3f us per step; floor (2 S^2 weights per step / 34.5 TB/s of L2) %.3f ms (x%.2f); rows route: %d queries, %d vector steps: '
              'k_region_extent %s over %d launches, call %.1f ms wall; rows / span x%.2f device, x%.2f wall; between the routes max |d P| %.3e over %d '
              'finite entries, max |d log P| / ((a + c + 1) 1e-9) %.3e over the %d of them with log P > -300; -inf from k_region_span alone in %d entries '
              '(rows route log P <= %.1f), from the rows route alone in %d (k_region_span log P <= %.1f)' % (
                  w, len(q) * R, w // 16 + 1, msteps, fmt(ts), n, np.median(ws), np.median(ts) * 1e3 / max(msteps, 1), floor, np.median(ts) / floor,
                  len(qr) * R, vsteps, fmt(tr), nn, np.median(wr_), np.median(tr) / np.median(ts), np.median(wr_) / np.median(ws),
                  np.abs(np.exp(got[fin]) - np.exp(out[fin])).max() if fin.any() else 0., fin.sum(), rel.max(), near.sum(),
                  only_s.sum(), got[only_s].max() if only_s.any() else -np.inf, only_r.sum(), out[only_r].max() if only_r.any() else -np.inf), flush=True)
    # the sample route at the window of 16: the joint survival function of the two ends of the constant-total run around each anchor
    w = 16
    exact = np.exp(b.region_span_raw(0, R, q, masks, labels, constrain, w, w))               # (R, A, w + 1, w + 1)
    lab_seg = labels[np.asarray(b.seg_class), posteriors.LABEL_NAMES.index('total')]         # (N1, S)
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    b.sample_states(0, R, CHUNK, seeds)
    t_draw = t_count = 0.
    reach = np.zeros((R, len(anchors), w + 1, w + 1))
    for k0 in range(0, K, CHUNK):
        t0 = time.perf_counter()
        st = b.sample_states(0, R, CHUNK, [s + k0 for s in seeds])      # (a fresh stream per chunk: the cost is what is measured)
        t1 = time.perf_counter()
        lab = lab_seg[np.arange(N1)[None, None], st]                                       # (R, CHUNK, N1)
        chg = lab[:, :, :-1] != lab[:, :, 1:]                                               # a label change across adjacency n -> n + 1
        pos = np.full(lab.shape, N1, dtype=np.int32)
        pos[:, :, :-1] = np.where(chg, np.arange(N1 - 1, dtype=np.int32)[None, None], np.int32(N1))
        nxt = np.minimum.accumulate(pos[:, :, ::-1], axis=2)[:, :, ::-1]                    # the first changing adjacency at or after n
        prv = np.full(lab.shape, -1, dtype=np.int32)
        prv[:, :, 1:] = np.where(chg, np.arange(1, N1, dtype=np.int32)[None, None], np.int32(-1))
        prv = np.maximum.accumulate(prv, axis=2)                                            # the first segment of the run that holds n, or -1
        right = np.clip(np.minimum(nxt[:, :, n0], c1[None, None]) - n0[None, None] + 1, 0, w + 1)      # columns 0 .. right - 1 are reached
        left = np.clip(n0[None, None] - np.maximum(prv[:, :, n0], c0[None, None]) + 1, 0, w + 1)
        il = (left[..., None] > np.arange(w + 1)).astype(np.float32)                       # (R, CHUNK, A, w + 1)
        ir = (right[..., None] > np.arange(w + 1)).astype(np.float32)
        reach += np.einsum('rkax,rkay->raxy', il, ir)
        t_draw += t1 - t0; t_count += time.perf_counter() - t1
    err = np.abs(reach / K - np.where(np.isfinite(exact), exact, 0.))
    print('  sample route, window 16, %d samples x %d restarts in chunks of %d: sample_states %.0f ms wall + counting both ends of the constant-total run of %d '
          'anchors in numpy %.0f ms = %.0f ms; |sample estimate - exact| of the joint survival function max %.3e, mean %.3e (1 / sqrt(K) = %.3e)' % (
              K, R, CHUNK, t_draw * 1e3, len(anchors), t_count * 1e3, (t_draw + t_count) * 1e3, err.max(), err.mean(), K ** -0.5), flush=True)
    rs.close()
