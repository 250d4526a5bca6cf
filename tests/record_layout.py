"""The fixed-size result record on a synthetic result with a distinct value in every field, for every valid combination of
the optional sections.  Run as a script (python -m tests.record_layout) it stores what restarts._pack returns for each
combination in tests/golden/record_layout.npz; that file was written by the commit before the record's sections got one
description (restarts._record_sections), and tests/test_record_layout_cpu.py holds every later _pack to it."""
import itertools
import os

import numpy as np

from remixt_amd import posteriors, restarts, sampling

N, M, NREG, BINS = 5, 3, 3, 4
BRK_IDS = ['brk_a', 'brk_b']
PARAM_NAMES = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
REGION_NAMES = ['r0', 'r1', 'r2']
INIT_PARAMS = {'mode_idx': 2, 'divergence_weight': 1e-6}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'record_layout.npz')


def combos():
    """The 20 valid switch combinations: samples x posterior x {no regions; regions x bins on/off x call confidence on/off}."""
    tails = [(False, 0, False)] + [(True, bins, call) for bins in (0, BINS) for call in (False, True)]
    return [(smp, post) + t for smp, post in itertools.product((False, True), repeat=2) for t in tails]


def combo_key(combo):
    return 'smp%d_post%d_reg%d_bins%d_call%d' % tuple(int(v) for v in combo)


def combo_kwargs(combo):
    smp, post, reg, bins, call = combo
    return dict(cn_samples=smp, cn_posterior=post, region_names=REGION_NAMES if reg else None, change_bins=bins, call_confidence=call)


def synthetic_result():
    """A result with every optional output present and no value used twice: floats count up in quarters from 1000, the
    int8 fields count up from 0."""
    nf = itertools.count()
    ni = itertools.count()

    def fl(*shape):
        return np.array([1000. + 0.25 * next(nf) for _ in range(int(np.prod(shape)))]).reshape(shape)

    def i8(*shape):
        return np.array([next(ni) for _ in range(int(np.prod(shape)))], dtype=np.int64).reshape(shape)

    res = {'h': fl(M), 'cn': i8(N, M, 2), 'brk_cn': dict((k, i8(M)) for k in BRK_IDS), 'p_outlier_total': fl(N, 2), 'p_outlier_allele': fl(N, 2),
           'total_likelihood_mask': i8(N), 'allele_likelihood_mask': i8(N)}
    st = {'error_message': 'optimization failed (h kept)'}
    for k in ['elbo', 'elbo_diff', 'ploidy', 'proportion_divergent'] + PARAM_NAMES + list(sampling.SUMMARY_STATS) + list(posteriors.SUMMARY_STATS) + ['cn_logprob']:
        st[k] = float(fl(1)[0])
    res['stats'] = st
    res['cn_sample_agreement'] = fl(N, M); res['cn_state_agreement'] = fl(N)
    for k in posteriors.COMPACT_ARRAYS:
        res[k] = fl(N, M) if k.startswith('total_cn') else fl(N)
    res['region_events'] = dict([('names', list(REGION_NAMES))] + [(k, fl(NREG)) for k in posteriors.REGION_ARRAYS])
    res['region_change_counts'] = dict([('names', list(REGION_NAMES)), ('bins', BINS)] + [(k, fl(NREG, BINS)) for k in posteriors.COUNT_ARRAYS])
    res['call_confidence'] = dict([('names', list(REGION_NAMES))] + [(k, fl(NREG)) for k in posteriors.CALL_ARRAYS])
    assert next(ni) <= 127
    return res


def pack(res, combo):
    return restarts._pack(res, N, M, len(BRK_IDS), len(PARAM_NAMES), BRK_IDS, PARAM_NAMES, **combo_kwargs(combo))


def unpack(f, i8, combo):
    return restarts._unpack(f, i8, N, M, len(BRK_IDS), len(PARAM_NAMES), BRK_IDS, PARAM_NAMES, INIT_PARAMS, **combo_kwargs(combo))


def main():
    res = synthetic_result()
    out = {}
    for combo in combos():
        f, i8 = pack(res, combo)
        out[combo_key(combo) + '_f'] = f
        out[combo_key(combo) + '_i8'] = i8
    np.savez_compressed(GOLDEN, **out)
    print('%s: %d records' % (GOLDEN, len(out) // 2))


if __name__ == '__main__':
    main()
