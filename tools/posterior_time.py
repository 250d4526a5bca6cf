"""Exact posterior summaries (k_posterior_summary) of all 16 restarts of the bench workload (50 000 segments, one RestartSet) at 165
and 355 states, after one variational sweep, in one process: device time of the kernel, wall time of posterior_summary_raw for the
compact set (2M + 4 columns, statistics, arg-max) and for the set with the one-hot marginals, and the wall time of the route without
the kernel: rmx_get_array(posterior_marginals) per restart plus post @ W in numpy.
Usage: python tools/posterior_time.py [MAXCN ...]   (default 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import posteriors, synthetic
from remixt_amd.restarts import RestartSet

R = 16
for mcn in [int(a) for a in sys.argv[1:]] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b = rs.batch
    rs.variational_update(1); b.synchronize()
    N, S, SP = b.num_segments, b.num_cn_states, b.info(4)
    states = np.zeros((R, N), dtype=np.int16)
    print('%d states (rows of %d), %d segments, %d restarts' % (S, SP, N, R), flush=True)
    for name, marg in (('compact', False), ('with marginals', True)):
        W, lay = posteriors.feature_matrix(b.cn_classes, marginals=marg)
        Q = lay['Q']
        wall = []
        for rep in range(4):
            t0 = time.perf_counter(); b.posterior_summary_raw(0, R, weights=W, states=states); wall.append(time.perf_counter() - t0)
        b.profile_reset(); b.profile_enable(1)
        b.posterior_summary_raw(0, R, weights=W, states=states)
        ms, n = b.profile().get('k_posterior_summary', (0., 0)); b.profile_enable(0)
        read = R * N * S * 8; wrote = R * N * (Q * 8 + 24 + 2)
        floor = (read + wrote) / 6.0e12 * 1e3
        print('  %-14s Q %3d: k_posterior_summary %.3f ms device over %d launches (floor %.3f ms = (%.0f MB read + %.0f MB written) / 6.0 TB/s: x%.2f); '
              'posterior_summary_raw %.1f ms wall (median of 3 after warm-up: %s)' % (
                  name, Q, ms, n, floor, read / 1e6, wrote / 1e6, ms / floor, np.median(wall[1:]) * 1e3, ' '.join('%.1f' % (x * 1e3) for x in wall)), flush=True)
        # the same outputs without the kernel: every restart's marginals to the host, then numpy
        if not marg:
            t0 = time.perf_counter()
            for r in range(R):
                post = b.get_array(r, 'posterior_marginals')
                t1 = time.perf_counter()
                post @ W[b.seg_class[0]]; post.max(axis=1); post.argmax(axis=1)
                if r == 0:
                    t_copy, t_np = t1 - t0, time.perf_counter() - t1
            print('  read-back route (get_array per restart + post @ W, max, argmax in numpy; no entropy): %.0f ms wall for %d restarts '
                  '(restart 0: copy %.1f ms, numpy %.1f ms)' % ((time.perf_counter() - t0) * 1e3, R, t_copy * 1e3, t_np * 1e3), flush=True)
    rs.close()
