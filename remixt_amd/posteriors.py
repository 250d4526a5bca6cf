"""Exact per-segment posterior summaries from the marginals of the last variational sweep.

Every quantity here is a linear functional of a row of `posterior_marginals`, with weights that depend only on the
segment's state class; the device evaluates all of them in one read of the marginals (`rmx_posterior_summary`,
`RemixtBatch.posterior_summary_raw`).  This module is the host side: the weight tables (`feature_matrix`), the map from a
decoded path back to state indices (`cn_to_states`), the named arrays of a result (`unpack`) and the two whole-genome
expectations (`summary_stats`).  numpy only."""
import numpy as np

# the arrays a fit result gains with config cn_posterior_summary (all in experiment segment order) and the two stats
COMPACT_ARRAYS = ('cn_posterior_prob', 'cn_posterior_max', 'cn_posterior_entropy', 'p_subclonal', 'p_loh', 'p_hdel',
                  'total_cn_mean', 'total_cn_sd')
SUMMARY_STATS = ('ploidy_posterior_mean', 'proportion_divergent_posterior_mean')


def feature_matrix(cn_classes, marginals=False):
    """Weight tables of the posterior summaries: (weights (C, S, Q) float64, layout).

    Columns, for a class table cn (S, M, 2): each clone's total copy number tot_m (M columns), tot_m squared (M),
    num_alleles_subclonal (0, 1 or 2), num_alleles_subclonal > 0, is_loh, is_hdel -- the last four as bpmodel.pyx:505-507
    defines the reference's derived tables -- and with marginals=True the one-hot columns [cn[s][m][a] == c] for
    c = 0 .. cn_classes.max(), in (m, a, c) order.  layout names the columns: slices 'tot', 'tot2', 'marginals' (or
    None), indices 'alleles_subclonal', 'subclonal', 'loh', 'hdel', and 'M', 'cn_max', 'Q'."""
    cn = np.asarray(cn_classes)
    if cn.ndim != 4 or cn.shape[3] != 2:
        raise ValueError('cn_classes must have shape (num_classes, num_cn_states, num_clones, 2)')
    C, S, M, _ = cn.shape
    tot = cn.sum(axis=3).astype(float)                                          # (C, S, M)
    nas = (cn[:, :, 1:, :].max(axis=-2) != cn[:, :, 1:, :].min(axis=-2)).sum(axis=-1)
    is_hdel = np.all(cn == 0, axis=(-2, -1))
    is_loh = np.any(cn.sum(axis=-2) == 0, axis=-1)
    cols = [tot, tot * tot, nas[..., None] * 1., (nas > 0)[..., None] * 1., is_loh[..., None] * 1., is_hdel[..., None] * 1.]
    layout = {'tot': slice(0, M), 'tot2': slice(M, 2 * M), 'alleles_subclonal': 2 * M, 'subclonal': 2 * M + 1, 'loh': 2 * M + 2,
              'hdel': 2 * M + 3, 'marginals': None, 'M': M, 'cn_max': int(cn.max()), 'Q': 2 * M + 4}
    if marginals:
        cmax = int(cn.max())
        onehot = (cn[..., None] == np.arange(cmax + 1)) * 1.                    # (C, S, M, 2, cmax + 1)
        cols.append(onehot.reshape(C, S, M * 2 * (cmax + 1)))
        layout['marginals'] = slice(2 * M + 4, 2 * M + 4 + M * 2 * (cmax + 1))
        layout['Q'] = layout['marginals'].stop
    return np.ascontiguousarray(np.concatenate(cols, axis=2)), layout


def _state_keys(cn, base):
    """One integer per (M, 2) tuple: its digits in base `base`."""
    cn = np.asarray(cn, dtype=np.int64)
    M = cn.shape[-2]
    place = base ** np.arange(2 * M, dtype=np.int64)
    return (cn.reshape(cn.shape[:-2] + (2 * M,)) * place).sum(axis=-1)


def cn_to_states(cn, cn_classes, seg_class):
    """The inverse of RemixtBatch.states_to_cn: copy numbers (..., N, M, 2) -> state indices int16 (..., N) into each
    segment's class table.  ValueError if a segment's copy number is not in its table."""
    cn = np.asarray(cn)
    cn_classes = np.asarray(cn_classes)
    seg_class = np.asarray(seg_class)
    C, S, M, _ = cn_classes.shape
    if cn.shape[-3:] != (len(seg_class), M, 2):
        raise ValueError('cn must have shape (..., num_segments, num_clones, 2)')
    if cn.size and cn.min() < 0:
        raise ValueError('negative copy number')
    base = int(max(cn_classes.max(), cn.max() if cn.size else 0)) + 1
    if base ** (2 * M) >= 2 ** 62:
        raise ValueError('copy numbers too large to key')
    table_keys = _state_keys(cn_classes, base)                                  # (C, S)
    keys = _state_keys(cn, base)                                                # (..., N)
    states = np.zeros(keys.shape, dtype=np.int16)
    for c in range(C):
        sel = seg_class == c
        if not sel.any():
            continue
        order = np.argsort(table_keys[c], kind='stable')
        sorted_keys = table_keys[c][order]
        k = keys[..., sel]
        pos = np.minimum(np.searchsorted(sorted_keys, k), S - 1)
        if not np.array_equal(sorted_keys[pos], k):
            raise ValueError('a copy number is not in its segment\'s state table (class %d)' % c)
        states[..., sel] = order[pos]
    return states


def states_in_model_order(cn, batch, seg_fwd_remap):
    """A path decoded in experiment segment order (the `cn` of a fit result) as int16 (N,) state indices in the model
    order of `batch`; model segments the experiment does not hold get state 0 (their summaries are dropped again by the
    same remap)."""
    states = np.zeros(batch.num_segments, dtype=np.int16)
    states[seg_fwd_remap] = cn_to_states(cn, batch.cn_classes, batch.seg_class[seg_fwd_remap])
    return states


def unpack(proj, stats, argmax, layout, cn_classes=None, seg_class=None):
    """Named arrays of one restart's raw outputs: proj (N, Q) for the weights of feature_matrix (layout: its second
    value), stats (N, 3), argmax (N,); any of the three may be None, and cn_classes / seg_class are needed only for
    cn_mpm.  total_cn_mean / total_cn_sd (N, M), p_subclonal, p_loh, p_hdel, expected_alleles_subclonal (N,),
    cn_posterior_max, cn_posterior_entropy, cn_posterior_prob (the marginal at the state handed to the device), cn_mpm
    (N, M, 2): the copy numbers of the marginal arg-max state (posterior decoding, as opposed to Viterbi), and with
    one-hot columns cn_marginals (N, M, 2, cn_max + 1)."""
    out = {}
    if proj is not None:
        proj = np.asarray(proj)
        mean = proj[:, layout['tot']]
        out['total_cn_mean'] = mean.copy()
        out['total_cn_sd'] = np.sqrt(np.maximum(proj[:, layout['tot2']] - mean * mean, 0.))
        out['expected_alleles_subclonal'] = proj[:, layout['alleles_subclonal']].copy()
        out['p_subclonal'] = proj[:, layout['subclonal']].copy()
        out['p_loh'] = proj[:, layout['loh']].copy()
        out['p_hdel'] = proj[:, layout['hdel']].copy()
        if layout['marginals'] is not None:
            out['cn_marginals'] = proj[:, layout['marginals']].reshape(proj.shape[0], layout['M'], 2, layout['cn_max'] + 1).copy()
    if stats is not None:
        stats = np.asarray(stats)
        out['cn_posterior_max'] = stats[:, 0].copy()
        out['cn_posterior_entropy'] = stats[:, 1].copy()
        out['cn_posterior_prob'] = stats[:, 2].copy()
    if argmax is not None and cn_classes is not None:
        out['cn_mpm'] = np.asarray(cn_classes)[np.asarray(seg_class), np.asarray(argmax)]
    return out


def summary_stats(summary, l):
    """Exact posterior expectations of the two whole-genome statistics of a fit result (tumour_ploidy_and_divergence):
    ploidy_posterior_mean -- the l-weighted total_cn_mean of the tumour clones over (M - 1) sum(l) -- and
    proportion_divergent_posterior_mean -- the l-weighted expected_alleles_subclonal over 2 sum(l).  summary and l in the
    same segment order."""
    l = np.asarray(l, dtype=float)
    mean = np.asarray(summary['total_cn_mean'])
    M = mean.shape[1]
    ploidy = (mean[:, 1:].sum(axis=1) * l).sum() / ((M - 1) * l.sum())
    prop = (np.asarray(summary['expected_alleles_subclonal']) * l).sum() / (2. * l.sum())
    return {'ploidy_posterior_mean': float(ploidy), 'proportion_divergent_posterior_mean': float(prop)}


def batch_summaries(batch, r0, nr, states=None, marginals=False):
    """unpack()ed summaries of restarts r0 .. r0+nr-1 of a RemixtBatch from one device call, in model segment order.
    states: int16 (nr, N) decoded states for cn_posterior_prob, or None (the key is then left out)."""
    weights, layout = feature_matrix(batch.cn_classes, marginals)
    proj, stats, amax = batch.posterior_summary_raw(r0, nr, weights=weights, states=states)
    out = []
    for i in range(nr):
        s = unpack(proj[i], stats[i], amax[i], layout, batch.cn_classes, batch.seg_class)
        if states is None:
            del s['cn_posterior_prob']
        out.append(s)
    return out


def add_posterior_summary(res, summary, l):
    """Fit result dict `res` gains the compact arrays of `summary` (experiment segment order) next to `cn` and the two
    posterior means in `stats`."""
    for k in COMPACT_ARRAYS:
        res[k] = summary[k]
    res['stats'].update(summary_stats(summary, l))
    return res
