"""Posterior path sampling against the batched decode of the same restarts: 64 samples of all 16 restarts of the bench workload
(50 000 segments, one RestartSet) at 165 and 355 states, after one variational sweep, in one process.
Usage: python tools/sample_time.py [MAXCN ...]   (default 8 12: 165 and 355 states)"""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from remixt_amd import synthetic, sampling
from remixt_amd.restarts import RestartSet

K, R = 64, 16
for mcn in [int(a) for a in sys.argv[1:]] or [8, 12]:
    e = synthetic.make_experiment(50000, num_clones=3, max_copy_number=mcn, num_chains=23, seed=0)
    ps = synthetic.make_init_params(e, R, mcn)
    rs = RestartSet(e, ps, mcn, num_clones=3, quiet=True, seeds=list(range(R)))
    b = rs.batch
    rs.variational_update(1); b.synchronize()
    seeds = [sampling.restart_seed(0, i) for i in range(R)]
    t_dec, t_smp = [], []
    for rep in range(4):
        t0 = time.perf_counter(); b.infer_cn_batch(0, R); t1 = time.perf_counter()
        b.sample_states(0, R, K, seeds); t2 = time.perf_counter()
        t_dec.append(t1 - t0); t_smp.append(t2 - t1)
    b.profile_reset(); b.profile_enable(1)
    b.sample_states(0, R, K, seeds)
    prof = b.profile(); b.profile_enable(0)
    ms, n = prof.get('k_sample_cn', (0., 0))
    print('%d states, %d segments, %d chains, %d restarts: infer_cn_batch %.1f ms, sample_states(%d) %.1f ms (median of 4 after warm-up: %s / %s); '
          'k_sample_cn %.2f ms device over %d launches' % (b.num_cn_states, b.num_segments, b.info(1), R, np.median(t_dec[1:]) * 1e3, K, np.median(t_smp[1:]) * 1e3,
                                                           ' '.join('%.1f' % (x * 1e3) for x in t_dec), ' '.join('%.1f' % (x * 1e3) for x in t_smp), ms, n), flush=True)
    rs.close()
