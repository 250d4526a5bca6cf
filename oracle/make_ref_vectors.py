"""Generate tests/golden/oracle_vs_ref.npz from the REFERENCE itself (build container only).

TEST INFRASTRUCTURE.  Runs the trace functions of tests/test_oracle_vs_ref.py over the reference kernel built by
oracle/build_ref.py (and, for the host class, the reference's `remixt.cn_model.BreakpointModel` imported in place)
and stores what they return; the tests run the same traces over the oracle.  The storage (an attribute only after the updates
that changed it, joint posteriors as two factors and the entries they miss, one packed vector) is described in the test module.

Usage:  python oracle/make_ref_vectors.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import build_ref, refload  # noqa: E402
from tests import helpers as H  # noqa: E402
from tests import test_oracle_vs_ref as T  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'oracle_vs_ref.npz')


def main():
    build_ref.build()
    bp = refload.load_ref_bpmodel()
    cm = refload.load_ref_cn_model()
    out = {}
    for M, max_cn, N, nc in T.KERNEL_CASES:
        case = T.kernel_case(M, max_cn, N, nc)
        last = {}
        trace = T.kernel_trace(bp, M, max_cn, N, nc)
        for k, v in trace.items():
            name = k.rsplit('/', 1)[-1]
            if name in H.STATE_ATTRS + H.DENSE_ATTRS:
                if name in last and np.array_equal(last[name], v):
                    continue
                last[name] = v
            if name == 'joint_posterior_marginals':
                u, w, indices, values = T.factor(v, trace[k.rsplit('/', 1)[0] + '/log_transmat'])
                for part, x in (('u', u), ('v', w), ('indices', indices), ('values', values)):
                    out['%s/%s#%s' % (case, k, part)] = x
                continue
            out[case + '/' + k] = v
    for k, v in T.host_trace(cm.BreakpointModel).items():
        out['host/' + k] = v
    for nc in (True, False):
        for k, v in T.cell_trace(bp, nc).items():
            out['cells_nc%d/%s' % (int(nc), k)] = v
    np.savez_compressed(OUT, **T.pack(out))
    print('%s: %d values, %d bytes' % (os.path.relpath(OUT, ROOT), len(out), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
