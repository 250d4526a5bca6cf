"""The fixed-size result record on a synthetic result with a distinct value in every field, for 33 combinations of the
optional sections.  Run as a script (python -m tests.record_layout) it stores what restarts._pack returns for each
combination in tests/golden/record_layout.npz; that file was written by the commit before the optional outputs got one
table (remixt_amd/outputs.py), and tests/test_record_layout_cpu.py holds every later _pack to it."""
import itertools
import os

import numpy as np

from remixt_amd import posteriors, restarts, sampling

N, M, NREG, BINS, EDGES = 5, 3, 3, 4, 3
BRK_IDS = ['brk_a', 'brk_b']
PARAM_NAMES = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
REGION_NAMES = ['r0', 'r1', 'r2']
EXTENT_NAMES = ['e0', 'e1']
INIT_PARAMS = {'mode_idx': 2, 'divergence_weight': 1e-6}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'record_layout.npz')

# a combination: the five early switches (samples, posterior, regions, bins, call confidence) and the six later ones
LATER = ('mom', 'ext', 'len', 'brk', 'calls', 'extr')
_NEEDS_REGIONS = ('mom', 'calls', 'extr')


def early_combos():
    """The 20 valid combinations of the first five sections: samples x posterior x {no regions; regions x bins on/off x
    call confidence on/off}, the later sections off."""
    tails = [(False, 0, False)] + [(True, bins, call) for bins in (0, BINS) for call in (False, True)]
    return [(smp, post) + t + (False,) * len(LATER) for smp, post in itertools.product((False, True), repeat=2) for t in tails]


def later_combos():
    """13 more (not the cross product): each later section alone with its prerequisites (regions for moments, calls and
    extremes; extents for lengths), everything on, and everything on but one later section (without extents, no lengths)."""
    def combo(early, on):
        on = set(on)
        if 'ext' not in on:
            on.discard('len')
        return early + tuple(k in on for k in LATER)
    out = []
    for k in LATER:
        out.append(combo((False, False, k in _NEEDS_REGIONS, 0, False), (k, 'ext') if k == 'len' else (k,)))
    everything = (True, True, True, BINS, True)
    out.append(combo(everything, LATER))
    for k in LATER:
        out.append(combo(everything, [x for x in LATER if x != k]))
    return out


def combos():
    return early_combos() + later_combos()


def combo_key(combo):
    """(the first 20 under the keys they were first stored by)"""
    key = 'smp%d_post%d_reg%d_bins%d_call%d' % tuple(int(v) for v in combo[:5])
    if any(combo[5:]):
        key += '_mom%d_ext%d_len%d_brk%d_calls%d_extr%d' % tuple(int(v) for v in combo[5:])
    return key


def combo_kwargs(combo):
    smp, post, reg, bins, call, mom, ext, ln, brk, calls, extr = combo
    return dict(cn_samples=smp, cn_posterior=post, region_names=REGION_NAMES if reg else None, change_bins=bins, call_confidence=call,
                cn_moments=mom, extent_names=EXTENT_NAMES if ext else None, length_edges=EDGES if ln else None, breakend_changes=brk,
                region_calls=calls, region_extremes=extr)


def synthetic_result():
    """A result with every optional output present and no value used twice: the floats of the fixed part and of the first five
    sections count up in quarters from 1000, those of the six later sections in whole numbers from 5000 (a record carries
    segment positions, flags and counts as floats: whole numbers come back exactly), the int8 fields count up from 0."""
    nf = itertools.count()
    nw = itertools.count()
    ni = itertools.count()

    def fl(*shape):
        return np.array([1000. + 0.25 * next(nf) for _ in range(int(np.prod(shape)))]).reshape(shape)

    def wh(*shape):
        return np.array([5000. + next(nw) for _ in range(int(np.prod(shape)))]).reshape(shape)

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
    # the six later sections, from the second counter (the values above are those of the first 20 stored records)
    shapes = posteriors.moment_shapes(NREG, M)
    res['region_cn_moments'] = dict([('names', list(REGION_NAMES))] + [(k, wh(*shapes[k])) for k in posteriors.MOMENT_ARRAYS])
    for k in posteriors.MOMENT_STATS:
        st[k] = float(wh(1)[0])
    nent = len(EXTENT_NAMES)
    res['event_extents'] = dict([('names', list(EXTENT_NAMES))] + [(k, wh(nent)) for k in posteriors.EXTENT_ARRAYS])
    res['event_lengths'] = dict([('names', list(EXTENT_NAMES))] + [(k, wh(nent)) for k in posteriors.SPAN_ARRAYS] +
                                [(k, wh(nent, EDGES)) for k in posteriors.SPAN_EDGE_ARRAYS])
    for k in posteriors.BREAKEND_ARRAYS:
        res[k] = wh(len(BRK_IDS), 2) if k == 'p_change' else wh(len(BRK_IDS))
    res['region_calls'] = dict([('names', list(REGION_NAMES))] + [(k, wh(NREG)) for k in posteriors.REGION_CALL_ARRAYS])
    res['region_cn_extremes'] = dict([('names', list(REGION_NAMES)), ('bins', posteriors.EXTREME_BINS)] +
                                     [(k, wh(NREG, M - 1, posteriors.EXTREME_BINS)) for k in posteriors.EXTREME_ARRAYS])
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
    f, _ = pack(res, later_combos()[len(LATER)])
    assert len(f) == 527 and len(set(f.tolist())) == 527, 'with everything on: 527 floats, all distinct'
    # (the records already stored stay as they are, to the bit)
    old = np.load(GOLDEN)
    assert set(old.files) >= set(combo_key(c) + s for c in early_combos() for s in ('_f', '_i8'))
    for k in old.files:
        assert old[k].dtype == out[k].dtype and np.array_equal(old[k], out[k]), k
    np.savez_compressed(GOLDEN, **out)
    print('%s: %d records' % (GOLDEN, len(out) // 2))


if __name__ == '__main__':
    main()
