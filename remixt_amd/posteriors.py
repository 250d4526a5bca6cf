"""Exact per-segment posterior summaries from the marginals of the last variational sweep.

Every quantity here is a linear functional of a row of `posterior_marginals`, with weights that depend only on the
segment's state class; the device evaluates all of them in one read of the marginals (`rmx_posterior_summary`,
`RemixtBatch.posterior_summary_raw`).  This module is the host side: the weight tables (`feature_matrix`), the map from a
decoded path back to state indices (`cn_to_states`), the named arrays of a result (`unpack`) and the two whole-genome
expectations (`summary_stats`).  numpy only."""
import collections

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


# ---- probabilities of path events over regions (rmx_region_prob) ---------------------------------------
MASK_NAMES = ('loh', 'not_loh', 'hdel', 'not_hdel', 'subclonal', 'not_subclonal')
LABEL_NAMES = ('state', 'total', 'unphased')
# the arrays of region_events: name -> (mask or None, label or None, complement).  The "any" events are the complements
# of "all segments are not ..."
REGION_EVENTS = (('p_all_loh', 'loh', None, False), ('p_any_loh', 'not_loh', None, True), ('p_all_hdel', 'hdel', None, False),
                 ('p_any_hdel', 'not_hdel', None, True), ('p_any_subclonal', 'not_subclonal', None, True),
                 ('p_no_change', None, 'state', False), ('p_no_total_change', None, 'total', False))
REGION_ARRAYS = tuple(e[0] for e in REGION_EVENTS)


def _ranks(keys):
    """Equal keys (rows of the last axis) -> equal small integers, over the whole array."""
    flat = keys.reshape(-1, keys.shape[-1])
    _, inv = np.unique(flat, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(keys.shape[:-1])
    if inv.size and inv.max() > 32767:
        raise ValueError('too many distinct labels for int16')
    return inv.astype(np.int16)


def event_tables(cn_classes):
    """State masks and labels of the region events: (masks uint8 (C, 6, S) in MASK_NAMES order, labels int16 (C, 3, S) in
    LABEL_NAMES order).  Masks: is_loh, is_hdel and num_alleles_subclonal > 0 as feature_matrix (bpmodel.pyx:505-507)
    defines them, and their complements.  Labels, each over the tumour clones (state classes differ only in the normal
    row, so equal labels across classes mean equal tumour copies): 'state' the copy numbers themselves, 'total' the
    per-clone totals, 'unphased' the copy numbers up to a swap of the two alleles in every clone at once."""
    cn = np.asarray(cn_classes)
    if cn.ndim != 4 or cn.shape[3] != 2:
        raise ValueError('cn_classes must have shape (num_classes, num_cn_states, num_clones, 2)')
    C, S, M, _ = cn.shape
    nas = (cn[:, :, 1:, :].max(axis=-2) != cn[:, :, 1:, :].min(axis=-2)).sum(axis=-1)
    is_hdel = np.all(cn == 0, axis=(-2, -1))
    is_loh = np.any(cn.sum(axis=-2) == 0, axis=-1)
    sub = nas > 0
    masks = np.stack([is_loh, ~is_loh, is_hdel, ~is_hdel, sub, ~sub], axis=1).astype(np.uint8)
    tum = cn[:, :, 1:, :].astype(np.int64)                                      # (C, S, M - 1, 2)
    flat = tum.reshape(C, S, -1)
    swapped = tum[..., ::-1].reshape(C, S, -1)
    # the lexicographically smaller of the two phasings
    diff = flat != swapped
    first = diff.argmax(axis=-1)[..., None]
    smaller = np.take_along_axis(swapped, first, -1) < np.take_along_axis(flat, first, -1)
    canon = np.where(smaller & diff.any(axis=-1, keepdims=True), swapped, flat)
    labels = np.stack([_ranks(flat), _ranks(tum.sum(axis=-1)), _ranks(canon)], axis=1)
    return np.ascontiguousarray(masks), np.ascontiguousarray(labels)


def chains_from_telomeres(is_telomere):
    """(chain_start, chain_end) model segment indices from the is_telomere flags: a chain ends at a telomere segment and
    at the last segment."""
    tel = np.asarray(is_telomere) != 0
    end = np.flatnonzero(tel)
    if len(tel) and (len(end) == 0 or end[-1] != len(tel) - 1):
        end = np.append(end, len(tel) - 1)
    start = np.concatenate([[0], end[:-1] + 1]).astype(np.int64) if len(end) else end
    return start, end.astype(np.int64)


def region_queries(regions, seg_fwd_remap, seg_is_original, chain_start, chain_end):
    """Experiment-order segment intervals [i, j] (regions: (R, 2) ints, i <= j) as runs of model segments:
    (runs int32 (P, 2), piece_region int (P,), constrain uint8 (N1,)).  The run of [i, j] is seg_fwd_remap[i] ..
    seg_fwd_remap[j] -- the remap is monotone, so the zero-length segments inserted between i and j lie inside it -- split
    at chain ends into pieces (piece_region: the region a piece belongs to; pieces of a region are consecutive).
    constrain is seg_is_original: a state mask binds only real segments, while a label constraint binds every adjacency
    of a run, the ones through a breakend's inserted segment included."""
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    cs, ce = np.asarray(chain_start, dtype=np.int64), np.asarray(chain_end, dtype=np.int64)
    if len(reg) and (reg.min() < 0 or reg.max() >= len(fwd) or (reg[:, 0] > reg[:, 1]).any()):
        raise ValueError('a region needs 0 <= first <= last < number of segments')
    A, B = fwd[reg[:, 0]], fwd[reg[:, 1]]
    ca, cb = np.searchsorted(ce, A, side='left'), np.searchsorted(ce, B, side='left')      # the chains of the two ends
    npieces = cb - ca + 1
    piece_region = np.repeat(np.arange(len(reg)), npieces)
    k = np.arange(len(piece_region)) - np.repeat(np.cumsum(npieces) - npieces, npieces)
    chain = ca[piece_region] + k
    runs = np.stack([np.maximum(A[piece_region], cs[chain]), np.minimum(B[piece_region], ce[chain])], axis=1).astype(np.int32)
    return runs, piece_region, np.ascontiguousarray(np.asarray(seg_is_original) != 0, dtype=np.uint8)


def combine(logp, piece_region, num_regions):
    """log-probability of every region's event from its pieces' (last axis of logp: pieces): their sum.  Chains are
    independent under the structured posterior, a mask event is a conjunction over segments, and a label event is a
    conjunction over adjacencies -- a chain end is not an adjacency."""
    logp = np.asarray(logp, dtype=float)
    out = np.zeros(logp.shape[:-1] + (int(num_regions),))
    with np.errstate(invalid='ignore'):
        np.add.at(out, (Ellipsis, np.asarray(piece_region)), logp)
    return out


def batch_region_events(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, events=REGION_EVENTS):
    """The arrays of `events` (default: the seven of REGION_EVENTS), each (nr, len(regions)), for restarts r0 .. r0+nr-1 of a
    RemixtBatch from one device call.  regions: (first, last) experiment segment indices."""
    masks, labels = event_tables(batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    P, R = len(runs), len(np.asarray(regions).reshape(-1, 2))
    q = np.zeros((len(events), P, 4), dtype=np.int32)
    q[:, :, :2] = runs[None]
    for e, (_, mask, label, _) in enumerate(events):
        q[e, :, 2] = -1 if mask is None else MASK_NAMES.index(mask)
        q[e, :, 3] = -1 if label is None else LABEL_NAMES.index(label)
    if P == 0:
        return dict((ev[0], np.zeros((nr, 0))) for ev in events)
    logp = batch.region_logprob_raw(r0, nr, q.reshape(-1, 4), masks, labels, constrain).reshape(nr, len(events), P)
    out = {}
    for e, (name, _, _, complement) in enumerate(events):
        lp = np.minimum(combine(logp[:, e], piece_region, R), 0.)      # (a sum of rounded logs of 1 can sit an ulp above 0)
        out[name] = -np.expm1(lp) if complement else np.exp(lp)
    return out


def adjacency_regions(seg_fwd_remap, is_telomere):
    """(regions (A, 2), index (A,)): the experiment segment pairs [n, n + 1] that a reference adjacency joins -- no chain
    end between their model segments -- and their n."""
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    ends_before = np.concatenate([[0], np.cumsum(np.asarray(is_telomere) != 0)])      # chain ends among model segments < n
    joined = ends_before[fwd[1:]] == ends_before[fwd[:-1]]
    n = np.flatnonzero(joined)
    return np.stack([n, n + 1], axis=1), n


def batch_change_prob(batch, r0, nr, seg_fwd_remap, seg_is_original, is_telomere):
    """(nr, N - 1): the probability that the copy-number state changes between experiment segments n and n + 1 (anywhere
    along the model segments that join them), NaN where no reference adjacency joins the two."""
    regions, n = adjacency_regions(seg_fwd_remap, is_telomere)
    out = np.full((nr, max(len(seg_fwd_remap) - 1, 0)), np.nan)
    if len(n):
        ev = (('p_change', None, 'state', True),)
        out[:, n] = batch_region_events(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, events=ev)['p_change']
    return out


def add_region_events(res, names, events):
    """Fit result dict `res` gains `region_events`: the region names and the seven arrays of REGION_ARRAYS."""
    out = {'names': list(names)}
    for k in REGION_ARRAYS:
        out[k] = np.asarray(events[k])
    res['region_events'] = out
    return res


def parse_regions(cn_regions):
    """Config value cn_regions, a list of (name, first, last) -> (names, regions int (R, 2))."""
    names = [str(r[0]) for r in cn_regions]
    return names, np.array([[int(r[1]), int(r[2])] for r in cn_regions], dtype=np.int64).reshape(-1, 2)


# ---- distribution of the number of copy-number changes over regions (rmx_region_counts) -----------------
# the arrays of region_change_counts: name -> label
COUNT_LABELS = (('num_changes', 'state'), ('num_total_changes', 'total'))
COUNT_ARRAYS = tuple(c[0] for c in COUNT_LABELS)


def combine_counts(logp, piece_region, num_regions):
    """Distribution of every region's change count from its pieces': logp (..., pieces, bins) log-probabilities ->
    probabilities (..., num_regions, bins).  Chains are independent under the structured posterior and a chain end is not
    an adjacency, so a region's count is the sum of its pieces' counts: the pieces' distributions are convolved, with
    what lands past the last bin added to it (the last bin means bins - 1 changes or more).  A region without pieces has
    no changes."""
    with np.errstate(over='ignore'):
        p = np.exp(np.asarray(logp, dtype=float))
    K = p.shape[-1]
    out = np.zeros(p.shape[:-2] + (int(num_regions), K))
    out[..., 0] = 1.
    for j, reg in enumerate(np.asarray(piece_region)):
        cur = out[..., reg, :].copy()
        new = np.zeros_like(cur)
        for i in range(K):
            for k in range(K):
                new[..., min(i + k, K - 1)] += cur[..., i] * p[..., j, k]
        out[..., reg, :] = new
    return out


def batch_region_change_counts(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, bins=8, labels=('state', 'total')):
    """The distribution of the number of label changes over regions, for restarts r0 .. r0+nr-1 of a RemixtBatch from one
    device call: a dict of (nr, len(regions), bins) arrays of probabilities, `num_changes` for label 'state' and
    `num_total_changes` for 'total' (those of `labels`).  Entry k is the probability of exactly k changes between
    consecutive model segments of the region, the last entry that of bins - 1 or more.  A zero-length segment inserted at
    a shared boundary counts as a segment: a path that takes a third state there changes twice.  regions: (first, last)
    experiment segment indices."""
    bins = int(bins)
    if not 1 <= bins <= 16:
        raise ValueError('bins must be in 1 .. 16')
    names = dict((lb, nm) for nm, lb in COUNT_LABELS)
    _, label_tab = event_tables(batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    P, R = len(runs), len(np.asarray(regions).reshape(-1, 2))
    if P == 0:
        return dict((names[lb], np.zeros((nr, 0, bins))) for lb in labels)
    q = np.zeros((len(labels), P, 4), dtype=np.int32)
    q[:, :, :2] = runs[None]
    q[:, :, 2] = -1
    for e, lb in enumerate(labels):
        q[e, :, 3] = LABEL_NAMES.index(lb)
    logp = batch.region_counts_raw(r0, nr, q.reshape(-1, 4), None, label_tab, constrain, bins).reshape(nr, len(labels), P, bins)
    return dict((names[lb], np.clip(combine_counts(logp[:, e], piece_region, R), 0., 1.)) for e, lb in enumerate(labels))


def add_region_change_counts(res, names, bins, counts):
    """Fit result dict `res` gains `region_change_counts`: the region names, the number of bins and the arrays of
    COUNT_ARRAYS, each (len(names), bins)."""
    out = {'names': list(names), 'bins': int(bins)}
    for k in COUNT_ARRAYS:
        out[k] = np.asarray(counts[k])
    res['region_change_counts'] = out
    return res


def check_region_options(cn_regions, change_bins, call_confidence, region_moments=False):
    """The outputs that are computed over regions need cn_regions: checked before a fit, not after it."""
    if change_bins and cn_regions is None:
        raise ValueError('cn_region_change_bins needs cn_regions')
    if call_confidence and cn_regions is None:
        raise ValueError('cn_call_confidence needs cn_regions')
    if region_moments and cn_regions is None:
        raise ValueError('cn_region_moments needs cn_regions')


def change_bins(config):
    """Config value cn_region_change_bins, checked: 0 (off) or 1 .. 16 with cn_regions set."""
    from . import defaults
    bins = int(defaults.get_param(config, 'cn_region_change_bins') or 0)
    check_region_options(defaults.get_param(config, 'cn_regions'), bins, False)
    if not 0 <= bins <= 16:
        raise ValueError('cn_region_change_bins must be in 0 .. 16')
    return bins


# ---- probability that a copy-number call holds over regions (rmx_call_prob) -----------------------------
# the arrays of call_confidence: name -> the label up to which the path has to agree with the call
CALL_LABELS = (('p_call', 'state'), ('p_call_unphased', 'unphased'), ('p_call_total', 'total'))
CALL_ARRAYS = tuple(c[0] for c in CALL_LABELS)
_CALL_PATH_BYTES = 64 << 20      # the reference paths staged by one device call of batch_cn_logprob


def batch_call_confidence(batch, r0, nr, states, regions, seg_fwd_remap, seg_is_original, is_telomere):
    """The probability, under the structured posterior, that the copy-number path agrees with the call `states` at
    every segment of a region, for restarts r0 .. r0+nr-1 of a RemixtBatch from one device call: a dict of the three
    (nr, len(regions)) arrays of CALL_ARRAYS -- p_call (the same state everywhere), p_call_unphased (the same up to a swap of
    the alleles) and p_call_total (the same per-clone totals).  states: int (nr, N1) state indices in model segment
    order; what they hold at inserted zero-length segments is ignored (those are marginalised), so the output of
    states_in_model_order is valid input.  regions: (first, last) experiment segment indices; a region that spans chain
    ends is the conjunction over its chains, which are independent."""
    _, label_tab = event_tables(batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    P, R = len(runs), len(np.asarray(regions).reshape(-1, 2))
    if P == 0:
        return dict((name, np.zeros((nr, 0))) for name in CALL_ARRAYS)
    q = np.zeros((len(CALL_LABELS), P, 4), dtype=np.int32)
    q[:, :, :2] = runs[None]
    for e, (_, lb) in enumerate(CALL_LABELS):
        q[e, :, 2] = LABEL_NAMES.index(lb)
    paths = np.asarray(states).reshape(nr, 1, -1)
    logp = batch.call_logprob_raw(r0, nr, paths, q.reshape(-1, 4), label_tab, constrain).reshape(nr, len(CALL_LABELS), P)
    # (a sum of rounded logs of 1 can sit an ulp above 0)
    return dict((name, np.exp(np.minimum(combine(logp[:, e], piece_region, R), 0.))) for e, name in enumerate(CALL_ARRAYS))


def batch_cn_logprob(batch, r0, nr, states, seg_is_original, is_telomere):
    """log q of whole copy-number paths under the structured posterior, for restarts r0 .. r0+nr-1 of a RemixtBatch:
    states int (nr, K, N1) state indices in model segment order -> (nr, K).  It is the sum over the chains, which are
    independent, of the log-probability that the path takes exactly these states at every real segment; inserted
    zero-length segments are marginalised (what `states` holds there is ignored).  The paths go to the device in chunks
    over K of at most 64 MiB."""
    st = np.asarray(states)
    if st.ndim != 3 or st.shape[0] != nr:
        raise ValueError('states must have shape (nr, num_paths, num_segments)')
    K, N1 = st.shape[1], st.shape[2]
    cs, ce = chains_from_telomeres(is_telomere)
    constrain = np.ascontiguousarray(np.asarray(seg_is_original) != 0, dtype=np.uint8)
    out = np.zeros((nr, K))
    step = max(1, _CALL_PATH_BYTES // max(1, 2 * nr * N1))
    for k0 in range(0, K, step):
        k1 = min(K, k0 + step)
        q = np.zeros((k1 - k0, len(cs), 4), dtype=np.int32)
        q[:, :, 0], q[:, :, 1], q[:, :, 2] = cs[None], ce[None], -1
        q[:, :, 3] = np.arange(k1 - k0)[:, None]
        logp = batch.call_logprob_raw(r0, nr, st[:, k0:k1], q.reshape(-1, 4), None, constrain)
        out[:, k0:k1] = logp.reshape(nr, k1 - k0, len(cs)).sum(axis=2)
    return out


def add_call_confidence(res, names, conf, logprob):
    """Fit result dict `res` gains `call_confidence`: the region names and the three arrays of CALL_ARRAYS for its own
    `cn`, and stats['cn_logprob']: log q of that `cn`."""
    out = {'names': list(names)}
    for k in CALL_ARRAYS:
        out[k] = np.asarray(conf[k])
    res['call_confidence'] = out
    res['stats']['cn_logprob'] = float(logprob)
    return res


def call_confidence_on(config):
    """Config value cn_call_confidence, checked: it needs cn_regions."""
    from . import defaults
    on = bool(defaults.get_param(config, 'cn_call_confidence'))
    check_region_options(defaults.get_param(config, 'cn_regions'), 0, on)
    return on


# ---- mean and covariance of copy number over regions (rmx_region_moments) -------------------------------
# the fraction features of region_cn_moments: columns of feature_matrix, length-weighted and divided by the region's length
MOMENT_FRACTIONS = ('alleles_subclonal', 'subclonal', 'loh', 'hdel')
MOMENT_ARRAYS = ('length', 'total_cn_mean', 'total_cn_cov', 'fraction_mean', 'fraction_cov')
MOMENT_STATS = ('ploidy_posterior_sd', 'proportion_divergent_posterior_sd')


def moment_features(cn_classes):
    """Feature tables of the region moments, (C, M + 4, S) float64: each clone's total copy number (M rows), then the rows
    of MOMENT_FRACTIONS -- the columns of the same names of feature_matrix."""
    weights, layout = feature_matrix(cn_classes)
    cols = list(range(layout['tot'].start, layout['tot'].stop)) + [layout[k] for k in MOMENT_FRACTIONS]
    return np.ascontiguousarray(weights[:, :, cols].transpose(0, 2, 1))


def moment_shapes(num_regions, M):
    """The shapes of MOMENT_ARRAYS for `num_regions` regions and M clones."""
    nfr = len(MOMENT_FRACTIONS)
    return {'length': (num_regions,), 'total_cn_mean': (num_regions, M), 'total_cn_cov': (num_regions, M, M),
            'fraction_mean': (num_regions, nfr), 'fraction_cov': (num_regions, nfr, nfr)}


def combine_moments(out, piece_region, num_regions):
    """Moments of every region from its pieces': out (..., pieces, per) -> (..., num_regions, per).  The pieces of a region
    are split at chain ends, and chains are independent under the structured posterior, so both the means and the
    covariances of the pieces' sums add.  A region without pieces has all moments 0."""
    out = np.asarray(out, dtype=float)
    res = np.zeros(out.shape[:-2] + (int(num_regions), out.shape[-1]))
    np.add.at(res, (Ellipsis, np.asarray(piece_region), slice(None)), out)
    return res


def _moment_matrices(flat, nf):
    """(..., nf + nf (nf + 1) / 2): the means, then the upper triangle in row-major order -> (mean (..., nf), cov (..., nf, nf)
    symmetric by construction: both halves hold the same number)."""
    flat = np.asarray(flat)
    iu = np.triu_indices(nf)
    cov = np.zeros(flat.shape[:-1] + (nf, nf))
    cov[..., iu[0], iu[1]] = flat[..., nf:]
    cov[..., iu[1], iu[0]] = flat[..., nf:]
    return flat[..., :nf].copy(), cov


def batch_region_cn_moments(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, l1):
    """The exact posterior mean and covariance matrix of the length-weighted mean copy number of regions, and of the
    length fractions of MOMENT_FRACTIONS, for restarts r0 .. r0+nr-1 of a RemixtBatch: a dict of `length` (R,) -- the
    summed segment lengths L of each region --, `total_cn_mean` (nr, R, M) and `total_cn_cov` (nr, R, M, M) of
    sum_n l_n tot_m(c_n) / L over the region's segments, and `fraction_mean` (nr, R, 4) and `fraction_cov` (nr, R, 4, 4) of
    sum_n l_n phi(c_n) / L for phi in MOMENT_FRACTIONS (alleles_subclonal counts 0, 1 or 2 alleles; the others are
    indicators, so their entries are the fraction of the region's length in that state).  l1: the model-order segment
    lengths, 0 at inserted segments, which therefore do not count.  regions: (first, last) experiment segment indices; a
    region that spans chain ends is the sum over its chains, which are independent.  A region of length 0 gives NaN.
    Two queries per region piece -- the M totals and the four fractions -- in one device call when M == 4, in one call
    per group otherwise (a call has one number of features per query)."""
    feats = moment_features(batch.cn_classes)
    M, nfr = feats.shape[1] - len(MOMENT_FRACTIONS), len(MOMENT_FRACTIONS)
    if M > 4:
        raise NotImplementedError('region moments take at most 4 features per query: more than 4 clones are not supported')
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, _ = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    P, R = len(runs), len(np.asarray(regions).reshape(-1, 2))
    w = np.asarray(l1, dtype=float).reshape(1, -1)
    shapes = moment_shapes(R, M)
    if P == 0:
        return dict((k, np.zeros(shapes[k] if k == 'length' else (nr,) + shapes[k])) for k in MOMENT_ARRAYS)
    csum = np.concatenate([[0.], np.cumsum(w[0])])
    length = np.zeros(R)
    np.add.at(length, piece_region, csum[runs[:, 1] + 1] - csum[runs[:, 0]])
    q = np.zeros((2, P, 4), dtype=np.int32)
    q[:, :, :2] = runs[None]
    q[1, :, 2] = M
    if M == nfr:
        both = batch.region_moments_raw(r0, nr, q.reshape(-1, 4), feats, w, nfr).reshape(nr, 2, P, -1)
        tot, frac = both[:, 0], both[:, 1]
    else:
        tot = batch.region_moments_raw(r0, nr, q[0], feats, w, M)
        frac = batch.region_moments_raw(r0, nr, q[1], feats, w, nfr)
    out = {'length': length}
    with np.errstate(invalid='ignore', divide='ignore'):
        for name, flat, nf in (('total_cn', tot, M), ('fraction', frac, nfr)):
            mean, cov = _moment_matrices(combine_moments(flat, piece_region, R), nf)
            out[name + '_mean'] = np.where(length[None, :, None] > 0, mean / length[None, :, None], np.nan)
            out[name + '_cov'] = np.where(length[None, :, None, None] > 0, cov / (length * length)[None, :, None, None], np.nan)
    return out


def moment_stats(total_cn_mean, total_cn_cov, fraction_mean, fraction_cov):
    """The posterior SDs of the two whole-genome statistics of summary_stats from the moments of the whole-genome region
    (total_cn_mean (M,), total_cn_cov (M, M), fraction_mean (4,), fraction_cov (4, 4)), with its conventions: ploidy is the
    sum of the tumour clones' mean totals over M - 1, proportion_divergent the expected alleles_subclonal over 2."""
    cov = np.asarray(total_cn_cov, dtype=float)
    M = cov.shape[-1]
    ploidy_var = cov[1:, 1:].sum() / float((M - 1) ** 2)
    prop_var = np.asarray(fraction_cov, dtype=float)[0, 0] / 4.
    return {'ploidy_posterior_sd': float(np.sqrt(np.maximum(ploidy_var, 0.))), 'proportion_divergent_posterior_sd': float(np.sqrt(np.maximum(prop_var, 0.)))}


def genome_region(regions, num_segments):
    """`regions` with the whole-genome region (0, num_segments - 1) appended: the moments of a fit's regions and of the two
    whole-genome SDs come from one call."""
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([reg, [[0, int(num_segments) - 1]]], axis=0)


def add_region_cn_moments(res, names, moments, stats=None):
    """Fit result dict `res` gains `region_cn_moments`: the region names and the arrays of MOMENT_ARRAYS, one entry per
    name.  moments: those arrays for the named regions, followed (stats None) by the whole-genome region, from which
    stats['ploidy_posterior_sd'] and stats['proportion_divergent_posterior_sd'] are taken; or (stats: the two values) for the
    named regions alone."""
    n = len(names)
    out = {'names': list(names)}
    for k in MOMENT_ARRAYS:
        out[k] = np.asarray(moments[k])[:n].copy()
    res['region_cn_moments'] = out
    if stats is None:
        stats = moment_stats(*[np.asarray(moments[k])[n] for k in MOMENT_ARRAYS[1:]])
        stats = [stats[k] for k in MOMENT_STATS]
    res['stats'].update((k, float(v)) for k, v in zip(MOMENT_STATS, stats))
    return res


def region_moments_on(config):
    """Config value cn_region_moments, checked: it needs cn_regions."""
    from . import defaults
    on = bool(defaults.get_param(config, 'cn_region_moments'))
    check_region_options(defaults.get_param(config, 'cn_regions'), 0, False, on)
    return on


# ---- where a copy-number event begins and ends around an anchor (rmx_region_extent) ---------------------
EXTENT_QUANTILES = (0.05, 0.5, 0.95)
EXTENT_ARRAYS = ('p_event', 'left_q05', 'left_q50', 'left_q95', 'right_q05', 'right_q50', 'right_q95', 'left_censored', 'right_censored')
_EXTENT_MAX_SLOTS = 4096


def parse_event(event):
    """An event by the names of the region tables -> (mask index or -1, label index or -1): a name of MASK_NAMES ('loh': the
    LOH run around the anchor), a name of LABEL_NAMES ('state', 'total': the constant-state / constant-total run around the
    anchor), or a pair (mask name or None, label name or None)."""
    if isinstance(event, str):
        if event in MASK_NAMES:
            return MASK_NAMES.index(event), -1
        if event in LABEL_NAMES:
            return -1, LABEL_NAMES.index(event)
        raise ValueError('unknown event %r: a name of %r or of %r, or a pair of both' % (event, MASK_NAMES, LABEL_NAMES))
    try:
        mask, label = event
    except (TypeError, ValueError):
        raise ValueError('an event is a mask name, a label name or a (mask, label) pair, not %r' % (event,))
    if (mask is not None and mask not in MASK_NAMES) or (label is not None and label not in LABEL_NAMES):
        raise ValueError('unknown event %r: a mask of %r and a label of %r' % (event, MASK_NAMES, LABEL_NAMES))
    return (-1 if mask is None else MASK_NAMES.index(mask)), (-1 if label is None else LABEL_NAMES.index(label))


def parse_window(window):
    """A window as (wl, wr): an int (both sides) or a pair, each >= 0, wl + wr + 1 <= 4096."""
    if np.ndim(window) == 0:
        wl = wr = int(window)
    else:
        wl, wr = (int(w) for w in window)
    if wl < 0 or wr < 0 or wl + wr + 1 > _EXTENT_MAX_SLOTS:
        raise ValueError('a window needs widths >= 0 and at most %d slots' % _EXTENT_MAX_SLOTS)
    return wl, wr


def extent_queries(anchors, event, seg_fwd_remap, seg_is_original):
    """Anchors (experiment segment indices) and an event (parse_event) as the queries of rmx_region_extent:
    (queries int32 (A, 4): model segment of the anchor, mask index or -1, label index or -1, 0; constrain uint8 (N1,)).
    constrain is seg_is_original, as for region_queries: a mask binds only real segments, a label constraint binds every
    adjacency, the ones through an inserted segment included."""
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    anc = np.asarray(anchors, dtype=np.int64).reshape(-1)
    if len(anc) and (anc.min() < 0 or anc.max() >= len(fwd)):
        raise ValueError('an anchor needs 0 <= segment < number of segments')
    mi, li = parse_event(event)
    q = np.zeros((len(anc), 4), dtype=np.int32)
    q[:, 0], q[:, 1], q[:, 2] = fwd[anc], mi, li
    return q, np.ascontiguousarray(np.asarray(seg_is_original) != 0, dtype=np.uint8)


def _boundary(seg, surv, more, forward):
    """One side of extent_summary.  seg: the experiment segments of the side in walking order from the anchor (seg[0]);
    surv: P(E on the run from the anchor to seg[i]) / P(E at the anchor), 1 at i = 0 and not increasing; more: whether the
    chain goes on past seg[-1] (what lies there is censored).  -> (pmf of the boundary over seg, or over seg[:-1] with the
    censored mass when `more`; the quantiles of the boundary in increasing segment order; whether each lies in the censored
    mass).  The boundary is the last segment of the walk the event still reaches: B = seg[i] has mass surv[i] - surv[i + 1]."""
    nxt = np.append(surv[1:], 0.)
    pmf = np.maximum(surv - nxt, 0.)
    censored_mass = 0.
    if more:
        censored_mass, pmf = float(surv[-1]), pmf[:-1]
    quant, cens = [], []
    # walking away from the anchor the boundary's distribution function at seg[i] is 1 - surv[i + 1]; a left boundary is
    # reported in increasing segment order, where the distribution function at seg[i] is surv[i]
    for qv in EXTENT_QUANTILES:
        if forward:
            hit = np.flatnonzero(1. - nxt[:len(pmf)] >= qv)
            i = int(hit[0]) if len(hit) else len(seg) - 1
            c = not len(hit)
        else:
            hit = np.flatnonzero(surv >= qv)      # the farthest segment still reached with probability >= q
            i = int(hit[-1])
            c = bool(more and i == len(seg) - 1)
        quant.append(int(seg[i])); cens.append(c)
    return pmf, censored_mass, quant, cens


def extent_summary(logp, anchor, wl, wr, seg_fwd_remap, is_telomere):
    """What one row of rmx_region_extent says about where the event around `anchor` (an experiment segment index) begins and
    ends.  logp: (wl + wr + 1,) log-probabilities, slot k for model segment seg_fwd_remap[anchor] - wl + k.  A dict of
      p_event: the probability of the event at the anchor alone, exp(slot wl);
      right_segments / left_segments: the experiment segments of the window's original segments of the anchor's chain, from
        the anchor outward (inserted zero-length segments are dropped from the report);
      right_survival / left_survival: for each of those, the probability that the event reaches it, given the event at the
        anchor (1 at the anchor, not increasing outward; NaN everywhere if p_event is 0);
      right_pmf / left_pmf: the joint probability of the event at the anchor and its boundary -- the last segment the event
        still reaches -- at each segment; where the chain goes on past the window the last segment's entry is left out and
        right_censored_mass / left_censored_mass carries the mass at it or beyond (0 otherwise): pmf plus censored mass sum
        to p_event;
      right_quantiles / left_quantiles: the 5 / 50 / 95 % quantiles of each boundary given the event at the anchor, as
        experiment segment indices in increasing order (left <= anchor <= right), -1 if p_event is 0; a quantile that falls
        in the censored mass is the window's end, with right_censored / left_censored (3 bools) True."""
    logp = np.asarray(logp, dtype=float)
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    tel = np.asarray(is_telomere) != 0
    N1 = len(tel)
    if logp.shape != (wl + wr + 1,):
        raise ValueError('logp must have shape (wl + wr + 1,)')
    rev = np.full(N1, -1, dtype=np.int64)
    rev[fwd] = np.arange(len(fwd))
    cs, ce = chains_from_telomeres(tel)
    n0 = int(fwd[anchor])
    c = int(np.searchsorted(ce, n0, side='left'))
    with np.errstate(over='ignore'):
        p = np.minimum(np.exp(logp), 1.)
    p0 = float(p[wl])
    out = {'p_event': p0}
    for side, forward in (('right', True), ('left', False)):
        if forward:
            n = np.arange(n0, min(n0 + wr, int(ce[c])) + 1)
        else:
            n = np.arange(n0, max(n0 - wl, int(cs[c])) - 1, -1)
        n = n[rev[n] >= 0]
        seg = rev[n]
        with np.errstate(invalid='ignore', divide='ignore'):
            surv = np.minimum.accumulate(p[n - n0 + wl]) / p0 if p0 > 0 else np.full(len(n), np.nan)
        # the chain goes on past the window if another original segment of the chain lies beyond the last one reported
        beyond = np.arange(n[-1] + 1, int(ce[c]) + 1) if forward else np.arange(int(cs[c]), n[-1])
        more = bool((rev[beyond] >= 0).any())
        if p0 > 0:
            pmf, cm, quant, cens = _boundary(seg, surv, more, forward)
            pmf, cm = pmf * p0, cm * p0
        else:
            pmf, cm, quant, cens = np.zeros(len(seg) - (1 if more else 0)), 0., [-1] * 3, [False] * 3
        out[side + '_segments'] = seg
        out[side + '_survival'] = surv
        out[side + '_pmf'] = pmf
        out[side + '_censored_mass'] = cm
        out[side + '_quantiles'] = np.array(quant, dtype=np.int64)
        out[side + '_censored'] = np.array(cens, dtype=bool)
    return out


def compact_extents(summaries):
    """The arrays of EXTENT_ARRAYS, each (len(summaries),), from a list of extent_summary dicts: p_event, the six quantiles
    and, per side, whether any of its quantiles lies in the censored mass."""
    out = {'p_event': np.array([s['p_event'] for s in summaries], dtype=float)}
    for side in ('left', 'right'):
        for i, name in enumerate(('q05', 'q50', 'q95')):
            out['%s_%s' % (side, name)] = np.array([s[side + '_quantiles'][i] for s in summaries], dtype=np.int64)
        out[side + '_censored'] = np.array([bool(s[side + '_censored'].any()) for s in summaries], dtype=bool)
    return out


def batch_event_extents(batch, r0, nr, anchors, event, window, seg_fwd_remap, seg_is_original, is_telomere):
    """extent_summary of every anchor (experiment segment indices) for restarts r0 .. r0+nr-1 of a RemixtBatch from one
    device call: a list over restarts of lists over anchors.  event: parse_event; window: parse_window."""
    wl, wr = parse_window(window)
    q, constrain = extent_queries(anchors, event, seg_fwd_remap, seg_is_original)
    if len(q) == 0:
        return [[] for _ in range(nr)]
    masks, labels = event_tables(batch.cn_classes)
    logp = batch.region_extent_raw(r0, nr, q, masks, labels, constrain, wl, wr)
    anc = np.asarray(anchors, dtype=np.int64).reshape(-1)
    return [[extent_summary(logp[i, j], int(a), wl, wr, seg_fwd_remap, is_telomere) for j, a in enumerate(anc)] for i in range(nr)]


def parse_extents(cn_event_extents):
    """Config value cn_event_extents, a list of (name, segment, event) -> (names, anchors int (A,), events: parse_event's
    index pairs).  ValueError for a bad entry."""
    names, anchors, events = [], [], []
    for entry in cn_event_extents:
        try:
            name, seg, event = entry
        except (TypeError, ValueError):
            raise ValueError('cn_event_extents: an entry is (name, segment, event), not %r' % (entry,))
        if int(seg) != seg or int(seg) < 0:
            raise ValueError('cn_event_extents: the segment of %r must be an index >= 0' % (name,))
        names.append(str(name)); anchors.append(int(seg)); events.append(parse_event(event))
    return names, np.array(anchors, dtype=np.int64), events


def event_pair(indices):
    """parse_event's index pair back as a (mask name or None, label name or None) event."""
    mi, li = indices
    return (None if mi < 0 else MASK_NAMES[mi], None if li < 0 else LABEL_NAMES[li])


def extents_on(config, num_segments=None):
    """Config values cn_event_extents / cn_extent_window, checked before any fit: None (off), or (names, anchors, events,
    (wl, wr)).  num_segments: the experiment's number of segments, where known."""
    from . import defaults
    ext = defaults.get_param(config, 'cn_event_extents')
    if ext is None:
        return None
    names, anchors, events = parse_extents(ext)
    window = parse_window(defaults.get_param(config, 'cn_extent_window'))
    if num_segments is not None and len(anchors) and anchors.max() >= num_segments:
        raise ValueError('cn_event_extents: a segment is outside the experiment')
    return names, anchors, events, window


def grouped_event_extents(extent_fn, anchors, events, window):
    """The arrays of EXTENT_ARRAYS over all entries of a parsed cn_event_extents, from one call of
    extent_fn(anchors, event, window) -> list over restarts of lists of extent_summary per distinct event: a list over
    restarts of dicts of (A,) arrays."""
    anchors = np.asarray(anchors, dtype=np.int64)
    out = None
    for ev in sorted(set(events)):
        sel = np.flatnonzero([e == ev for e in events])
        per_restart = extent_fn(anchors[sel], event_pair(ev), window)
        if out is None:
            out = [dict((k, np.zeros(len(anchors), dtype=bool if k.endswith('censored') else (float if k == 'p_event' else np.int64)))
                        for k in EXTENT_ARRAYS) for _ in per_restart]
        for res, summaries in zip(out, per_restart):
            comp = compact_extents(summaries)
            for k in EXTENT_ARRAYS:
                res[k][sel] = comp[k]
    return out if out is not None else []


def add_event_extents(res, names, extents):
    """Fit result dict `res` gains `event_extents`: the entry names and the arrays of EXTENT_ARRAYS, one entry per name."""
    out = {'names': list(names)}
    for k in EXTENT_ARRAYS:
        # (a record carries them as floats)
        out[k] = np.asarray(extents[k]).astype(float if k == 'p_event' else (bool if k.endswith('_censored') else np.int64))
    res['event_extents'] = out
    return res


# ---- the joint law of an event's two ends, and of its length (rmx_region_span) ------------------------------
SPAN_ARRAYS = ('length_q05', 'length_q50', 'length_q95', 'length_censored')
SPAN_EDGE_ARRAYS = ('p_length_le', 'p_length_undetermined')
_SPAN_MAX_ENTRIES = 16384


def parse_span_window(window):
    """A window as (wl, wr): an int (both sides) or a pair, each >= 0, (wl + 1) (wr + 1) <= 16384."""
    if np.ndim(window) == 0:
        wl = wr = int(window)
    else:
        wl, wr = (int(w) for w in window)
    if wl < 0 or wr < 0 or (wl + 1) * (wr + 1) > _SPAN_MAX_ENTRIES:
        raise ValueError('a window needs widths >= 0 and a table of at most %d entries' % _SPAN_MAX_ENTRIES)
    return wl, wr


def _length_cdf(lengths, pmf, closed, p0):
    """length_cdf of span_summary: a function of edges."""
    def length_cdf(edges):
        e = np.asarray(edges, dtype=float).reshape(-1)
        if not p0 > 0:
            return np.full(len(e), np.nan), np.full(len(e), np.nan)
        le = lengths[None, :, :] <= e[:, None, None]
        p_le = (np.where(le & closed[None], pmf[None], 0.)).sum(axis=(1, 2)) / p0
        p_un = (np.where(le & ~closed[None], pmf[None], 0.)).sum(axis=(1, 2)) / p0
        return p_le, p_un
    return length_cdf


def span_summary(logp, anchor, wl, wr, seg_fwd_remap, is_telomere, l1):
    """What one table of rmx_region_span says about the two ends of the event around `anchor` (an experiment segment index)
    together, and about its length.  logp: (wl + 1, wr + 1) log-probabilities, entry (a, c) for the model segments
    [seg_fwd_remap[anchor] - a, seg_fwd_remap[anchor] + c]; l1: the lengths of the model segments.  It follows
    extent_summary: original segments only and in experiment indices (the sub-table of the original segments is taken before
    anything is differenced), and the running minimum is applied along both axes, so that rounding cannot make the table
    rise.  A dict of
      p_event: the probability of the event at the anchor alone, exp(entry (0, 0));
      left_segments / right_segments: as extent_summary, from the anchor outward; they index the rows / columns below;
      left_open / right_open: whether the chain goes on past the window on that side.  The side's last index is then the lump
        "this segment or beyond";
      joint_survival: P(the event reaches left[i] and right[j]) / p_event (NaN everywhere if p_event is 0);
      joint_pmf: P(event at the anchor, left end = left[i], right end = right[j]) = J[i][j] - J[i+1][j] - J[i][j+1] + J[i+1][j+1]
        of the table J, 0 beyond the last index; entries in (-1e-9 p_event, 0) are clipped to 0.  It sums to p_event, and its
        row and column sums are extent_summary's left_pmf and right_pmf followed by their censored masses;
      lengths: the sum of l1 over the model segments from left[i] to right[j]; a lower bound in an open cell;
      length_quantiles: the 5 / 50 / 95 % quantiles of the length given the event, over the closed cells in increasing length;
        a quantile the closed mass never reaches is the table's largest length with length_censored (3 bools) True; -1 if
        p_event is 0;
      length_cdf: a function of edges -> (p_le, p_undetermined), each (len(edges),), given the event: the closed mass with
        length <= edge, and the open mass whose lower bound is <= edge (its length may or may not be); NaN if p_event is 0."""
    logp = np.asarray(logp, dtype=float)
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    tel = np.asarray(is_telomere) != 0
    l1 = np.asarray(l1, dtype=float)
    N1 = len(tel)
    if logp.shape != (wl + 1, wr + 1):
        raise ValueError('logp must have shape (wl + 1, wr + 1)')
    rev = np.full(N1, -1, dtype=np.int64)
    rev[fwd] = np.arange(len(fwd))
    cs, ce = chains_from_telomeres(tel)
    n0 = int(fwd[anchor])
    c = int(np.searchsorted(ce, n0, side='left'))
    with np.errstate(over='ignore'):
        p = np.minimum(np.exp(logp), 1.)
    p0 = float(p[0, 0])
    nr_ = np.arange(n0, min(n0 + wr, int(ce[c])) + 1)
    nl_ = np.arange(n0, max(n0 - wl, int(cs[c])) - 1, -1)
    nr_, nl_ = nr_[rev[nr_] >= 0], nl_[rev[nl_] >= 0]
    right_open = bool((rev[np.arange(nr_[-1] + 1, int(ce[c]) + 1)] >= 0).any())
    left_open = bool((rev[np.arange(int(cs[c]), nl_[-1])] >= 0).any())
    J = p[np.ix_(n0 - nl_, nr_ - n0)]
    J = np.minimum.accumulate(np.minimum.accumulate(J, axis=0), axis=1)
    Jp = np.zeros((len(nl_) + 1, len(nr_) + 1))
    Jp[:-1, :-1] = J
    pmf = Jp[:-1, :-1] - Jp[1:, :-1] - Jp[:-1, 1:] + Jp[1:, 1:]
    pmf[(pmf < 0) & (pmf > -1e-9 * p0)] = 0.
    cum = np.concatenate([[0.], np.cumsum(l1)])
    lengths = cum[nr_ + 1][None, :] - cum[nl_][:, None]
    closed = np.ones(pmf.shape, dtype=bool)
    if left_open:
        closed[-1, :] = False
    if right_open:
        closed[:, -1] = False
    if p0 > 0:
        with np.errstate(invalid='ignore', divide='ignore'):
            surv = J / p0
        order = np.argsort(lengths[closed], kind='stable')
        ls, ms = lengths[closed][order], np.cumsum(pmf[closed][order]) / p0
        quant, cens = [], []
        for qv in EXTENT_QUANTILES:
            hit = np.flatnonzero(ms >= qv)
            quant.append(float(ls[hit[0]]) if len(hit) else float(lengths.max()))
            cens.append(not len(hit))
    else:
        surv = np.full(J.shape, np.nan)
        quant, cens = [-1.] * 3, [False] * 3
    return {'p_event': p0, 'left_segments': rev[nl_], 'right_segments': rev[nr_], 'left_open': left_open, 'right_open': right_open,
            'joint_survival': surv, 'joint_pmf': pmf, 'lengths': lengths, 'length_quantiles': np.array(quant, dtype=float),
            'length_censored': np.array(cens, dtype=bool), 'length_cdf': _length_cdf(lengths, pmf, closed, p0)}


def compact_spans(summaries, edges=()):
    """The arrays of SPAN_ARRAYS, each (len(summaries),), and of SPAN_EDGE_ARRAYS, each (len(summaries), len(edges)), from a list
    of span_summary dicts: the three length quantiles, whether any of them is censored, and length_cdf at `edges`."""
    edges = np.asarray(edges, dtype=float).reshape(-1)
    out = {}
    for i, name in enumerate(SPAN_ARRAYS[:3]):
        out[name] = np.array([s['length_quantiles'][i] for s in summaries], dtype=float)
    out['length_censored'] = np.array([bool(s['length_censored'].any()) for s in summaries], dtype=bool)
    cdf = [s['length_cdf'](edges) for s in summaries]
    out['p_length_le'] = np.array([c[0] for c in cdf], dtype=float).reshape(len(summaries), len(edges))
    out['p_length_undetermined'] = np.array([c[1] for c in cdf], dtype=float).reshape(len(summaries), len(edges))
    return out


def lengths_on(config, num_segments=None):
    """Config values cn_event_lengths / cn_event_length_edges, checked before any fit: None (off), or (names, anchors,
    events, (wl, wr), edges) of the entries of cn_event_extents, which it needs, with a window whose table fits."""
    from . import defaults
    if not defaults.get_param(config, 'cn_event_lengths'):
        return None
    ext = extents_on(config, num_segments)
    if ext is None:
        raise ValueError('cn_event_lengths needs cn_event_extents')
    names, anchors, events, window = ext
    try:
        window = parse_span_window(window)
    except ValueError:
        raise ValueError('cn_event_lengths: cn_extent_window %r gives a table of more than %d entries' % (window, _SPAN_MAX_ENTRIES))
    try:
        edges = tuple(float(x) for x in defaults.get_param(config, 'cn_event_length_edges'))
    except (TypeError, ValueError):
        raise ValueError('cn_event_length_edges: a list of lengths')
    if not all(x > 0 and np.isfinite(x) for x in edges):
        raise ValueError('cn_event_length_edges: every length must be > 0')
    return names, anchors, events, window, edges


def grouped_event_spans(span_fn, anchors, events, window, edges=()):
    """The arrays of SPAN_ARRAYS and SPAN_EDGE_ARRAYS over all entries of a parsed cn_event_extents, from one call of
    span_fn(anchors, event, window) -> list over restarts of lists of span_summary per distinct event: a list over restarts
    of dicts of (A,) and (A, len(edges)) arrays."""
    anchors = np.asarray(anchors, dtype=np.int64)
    out = None
    for ev in sorted(set(events)):
        sel = np.flatnonzero([e == ev for e in events])
        per_restart = span_fn(anchors[sel], event_pair(ev), window)
        if out is None:
            out = [dict([(k, np.zeros(len(anchors), dtype=bool if k == 'length_censored' else float)) for k in SPAN_ARRAYS] +
                        [(k, np.zeros((len(anchors), len(edges)))) for k in SPAN_EDGE_ARRAYS]) for _ in per_restart]
        for res, summaries in zip(out, per_restart):
            comp = compact_spans(summaries, edges)
            for k in SPAN_ARRAYS + SPAN_EDGE_ARRAYS:
                res[k][sel] = comp[k]
    return out if out is not None else []


def add_event_lengths(res, names, lengths):
    """Fit result dict `res` gains `event_lengths`: the entry names, the arrays of SPAN_ARRAYS, one entry per name, and the
    two tables of SPAN_EDGE_ARRAYS, (entries, edges)."""
    out = {'names': list(names)}
    for k in SPAN_ARRAYS + SPAN_EDGE_ARRAYS:
        # (a record carries them as floats)
        out[k] = np.asarray(lengths[k]).astype(bool if k == 'length_censored' else float)
    res['event_lengths'] = out
    return res


def batch_event_spans(batch, r0, nr, anchors, event, window, seg_fwd_remap, seg_is_original, is_telomere, l1):
    """span_summary of every anchor (experiment segment indices) for restarts r0 .. r0+nr-1 of a RemixtBatch from one device
    call: a list over restarts of lists over anchors.  event: parse_event; window: parse_span_window."""
    wl, wr = parse_span_window(window)
    q, constrain = extent_queries(anchors, event, seg_fwd_remap, seg_is_original)
    if len(q) == 0:
        return [[] for _ in range(nr)]
    masks, labels = event_tables(batch.cn_classes)
    logp = batch.region_span_raw(r0, nr, q, masks, labels, constrain, wl, wr)
    anc = np.asarray(anchors, dtype=np.int64).reshape(-1)
    return [[span_summary(logp[i, j], int(a), wl, wr, seg_fwd_remap, is_telomere, l1) for j, a in enumerate(anc)] for i in range(nr)]


# ---- joint events at several regions of a chain (rmx_region_pattern) ------------------------------------
# the arrays of focal_events: name -> (the mask the region lies in, the mask its flanks lie in)
FOCAL_EVENTS = (('p_focal_loh', 'loh', 'not_loh'), ('p_focal_hdel', 'hdel', 'not_hdel'), ('p_focal_subclonal', 'subclonal', 'not_subclonal'))
FOCAL_ARRAYS = tuple(e[0] for e in FOCAL_EVENTS)
# the arrays a fit result gains with config cn_breakend_changes: p_change (K, 2), the others (K,)
BREAKEND_ARRAYS = ('p_change', 'p_change_both', 'p_change_neither', 'p_change_only_first', 'p_change_only_second')


def pattern_queries(patterns, seg_fwd_remap, seg_is_original, chain_start, chain_end):
    """Patterns -- each a list of parts (first, last, event): an experiment-order segment interval and an event as
    parse_event takes it -- as the queries of rmx_region_pattern:
    (queries int32 (Q, 4), pieces int32 (P, 4), query_pattern int (Q,), constrain uint8 (N1,)).
    A part's run is seg_fwd_remap[first] .. seg_fwd_remap[last], as in region_queries, split at chain ends.  The parts of one
    pattern are grouped by chain into one query per chain (query_pattern: the pattern a query belongs to; combine() adds
    the chains' log-probabilities, chains being independent under the structured posterior), sorted, and parts that overlap
    or share a segment are merged when they carry the same event -- their conjunction is the event over the union.
    ValueError for parts of one pattern that overlap with different events.  Parts that only touch stay apart: nothing
    binds at the adjacency between them.  constrain is seg_is_original."""
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    cs, ce = np.asarray(chain_start, dtype=np.int64), np.asarray(chain_end, dtype=np.int64)
    queries, pieces, query_pattern = [], [], []
    for p, parts in enumerate(patterns):
        by_chain = {}
        for part in parts:
            try:
                first, last, event = part
            except (TypeError, ValueError):
                raise ValueError('a part of a pattern is (first, last, event), not %r' % (part,))
            first, last = int(first), int(last)
            if not 0 <= first <= last < len(fwd):
                raise ValueError('a part needs 0 <= first <= last < number of segments')
            mi, li = parse_event(event)
            A, B = int(fwd[first]), int(fwd[last])
            ca, cb = int(np.searchsorted(ce, A, side='left')), int(np.searchsorted(ce, B, side='left'))
            for c in range(ca, cb + 1):
                by_chain.setdefault(c, []).append((max(A, int(cs[c])), min(B, int(ce[c])), mi, li))
        for c in sorted(by_chain):
            merged = []
            for a, b, mi, li in sorted(by_chain[c]):
                if merged and a <= merged[-1][1]:
                    if (mi, li) != tuple(merged[-1][2:]):
                        raise ValueError('pattern %d: parts with different events overlap at model segment %d' % (p, a))
                    merged[-1][1] = max(merged[-1][1], b)
                else:
                    merged.append([a, b, mi, li])
            queries.append((len(pieces), len(merged), 0, 0))
            query_pattern.append(p)
            pieces.extend(tuple(m) for m in merged)
    return (np.array(queries, dtype=np.int32).reshape(-1, 4), np.array(pieces, dtype=np.int32).reshape(-1, 4),
            np.array(query_pattern, dtype=np.int64), np.ascontiguousarray(np.asarray(seg_is_original) != 0, dtype=np.uint8))


def batch_event_joint(batch, r0, nr, patterns, seg_fwd_remap, seg_is_original, is_telomere):
    """The joint probability of every pattern (pattern_queries) for restarts r0 .. r0+nr-1 of a RemixtBatch, from one
    rmx_region_pattern call and one rmx_region_prob call: a dict of `log_p_joint` and `p_joint` (nr, len(patterns)), `p_parts`
    -- a list over patterns of (nr, parts) arrays, each part of the pattern alone -- and `lift` (nr, len(patterns)) =
    p_joint / prod p_parts (NaN where a part has probability 0).  P(A | B) is p_joint of (A, B) over p_joint of (B,)."""
    patterns = [list(p) for p in patterns]
    masks, labels = event_tables(batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    q, pieces, query_pattern, constrain = pattern_queries(patterns, seg_fwd_remap, seg_is_original, cs, ce)
    P = len(patterns)
    out = {'log_p_joint': np.zeros((nr, P)), 'p_joint': np.ones((nr, P)), 'p_parts': [np.zeros((nr, len(p))) for p in patterns], 'lift': np.ones((nr, P))}
    if len(q) == 0:
        return out
    logp = batch.region_pattern_raw(r0, nr, q, pieces, masks, labels, constrain)
    lj = np.minimum(combine(logp, query_pattern, P), 0.)      # (a sum of rounded logs of 1 can sit an ulp above 0)
    # every part alone: one run per part and chain
    parts = [(p, k, part) for p, pat in enumerate(patterns) for k, part in enumerate(pat)]
    runs, run_part, _ = region_queries([(pt[0], pt[1]) for _, _, pt in parts], seg_fwd_remap, seg_is_original, cs, ce)
    ev = np.array([parse_event(pt[2]) for _, _, pt in parts], dtype=np.int32).reshape(-1, 2)
    rq = np.concatenate([runs, ev[run_part]], axis=1).astype(np.int32)
    lpart = np.minimum(combine(batch.region_logprob_raw(r0, nr, rq, masks, labels, constrain), run_part, len(parts)), 0.)
    for i, (p, k, _) in enumerate(parts):
        out['p_parts'][p][:, k] = np.exp(lpart[:, i])
    out['log_p_joint'], out['p_joint'] = lj, np.exp(lj)
    with np.errstate(divide='ignore', invalid='ignore'):
        for p in range(P):
            prod = out['p_parts'][p].prod(axis=1)
            out['lift'][:, p] = np.where(prod > 0., out['p_joint'][:, p] / prod, np.nan)
    return out


def focal_patterns(regions, flank, mask, flank_mask, seg_fwd_remap, chain_start, chain_end):
    """One pattern per region ((first, last) experiment segment indices): the region in `mask` and the `flank` segments on
    each side of it in `flank_mask`.  A flank stops at the end of the chain the region's end lies in (and at the ends of the
    genome); a side without segments drops out."""
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    cs, ce = np.asarray(chain_start, dtype=np.int64), np.asarray(chain_end, dtype=np.int64)
    flank = int(flank)
    if flank < 0:
        raise ValueError('flank must be >= 0')
    reg = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    if len(reg) and (reg.min() < 0 or reg.max() >= len(fwd) or (reg[:, 0] > reg[:, 1]).any()):
        raise ValueError('a region needs 0 <= first <= last < number of segments')
    out = []
    for first, last in reg:
        first, last = int(first), int(last)
        c0, c1 = int(np.searchsorted(ce, fwd[first], side='left')), int(np.searchsorted(ce, fwd[last], side='left'))
        # the experiment segments of the two chains: those whose model segment lies in them
        lo = int(np.searchsorted(fwd, cs[c0], side='left'))
        hi = int(np.searchsorted(fwd, ce[c1], side='right')) - 1
        pat = []
        if flank and first - 1 >= lo:
            pat.append((max(first - flank, lo), first - 1, flank_mask))
        pat.append((first, last, mask))
        if flank and last + 1 <= hi:
            pat.append((last + 1, min(last + flank, hi), flank_mask))
        out.append(pat)
    return out


def batch_focal_events(batch, r0, nr, regions, flank, seg_fwd_remap, seg_is_original, is_telomere):
    """The arrays of FOCAL_ARRAYS, each (nr, len(regions)), for restarts r0 .. r0+nr-1 of a RemixtBatch from one
    rmx_region_pattern call: p_focal_loh = P(every original segment of the region in LOH and none of the `flank` original
    segments on each side of it, inside the chain), p_focal_hdel and p_focal_subclonal likewise."""
    masks, labels = event_tables(batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    R = len(np.asarray(regions, dtype=np.int64).reshape(-1, 2))
    patterns = [pat for _, mask, fm in FOCAL_EVENTS for pat in focal_patterns(regions, flank, mask, fm, seg_fwd_remap, cs, ce)]
    q, pieces, query_pattern, constrain = pattern_queries(patterns, seg_fwd_remap, seg_is_original, cs, ce)
    if R == 0:
        return dict((name, np.zeros((nr, 0))) for name in FOCAL_ARRAYS)
    logp = batch.region_pattern_raw(r0, nr, q, pieces, masks, labels, constrain)
    p = np.exp(np.minimum(combine(logp, query_pattern, len(patterns)), 0.)).reshape(nr, len(FOCAL_EVENTS), R)
    return dict((name, p[:, e]) for e, name in enumerate(FOCAL_ARRAYS))


def breakend_adjacencies(breakpoint_idx, num_breakpoints):
    """int (K, 2): for every breakpoint k its two model adjacencies (n, n + 1), by their n with breakpoint_idx[n] == k in
    ascending order; -1 where the model holds fewer than two."""
    bidx = np.asarray(breakpoint_idx, dtype=np.int64)
    adj = np.full((int(num_breakpoints), 2), -1, dtype=np.int64)
    seen = np.zeros(int(num_breakpoints), dtype=np.int64)
    for n in np.flatnonzero(bidx >= 0):
        k = int(bidx[n])
        if k < len(adj) and seen[k] < 2:
            adj[k, seen[k]] = n
            seen[k] += 1
    adj[seen < 2] = -1
    return adj


def batch_breakend_changes(batch, r0, nr, breakpoint_idx, num_breakpoints, is_telomere, seg_is_original=None, label='state'):
    """Whether the copy-number state changes at the two breakends of every breakpoint, jointly, for restarts r0 .. r0+nr-1 of a
    RemixtBatch from one rmx_region_prob and one rmx_region_pattern call.  The breakends of breakpoint k are its two model
    adjacencies (breakend_adjacencies: `first` is the one with the smaller model segment index).  A dict of
      p_change (nr, K, 2)        the probability of a change of `label` across each breakend's adjacency,
      p_change_both, p_change_neither, p_change_only_first, p_change_only_second (nr, K): the 2 x 2 table of the two,
      log_p_same (nr, K, 2), log_p_same_both (nr, K): the raw log-probabilities of no change at each and at both.
    The table comes by inclusion-exclusion from P(no change at i), P(no change at j) and P(no change at i and at j); the
    last is a two-piece pattern on one chain -- one three-segment piece where the adjacencies share a segment -- and the
    product of the two where they lie in different chains (chains are independent).  Rounding-level negatives are clipped
    to 0 in the four derived columns only.  NaN for a breakpoint without two adjacencies in the model."""
    K = int(num_breakpoints)
    adj = breakend_adjacencies(breakpoint_idx, K)
    ok = np.flatnonzero(adj[:, 0] >= 0)
    names = ('p_change_both', 'p_change_neither', 'p_change_only_first', 'p_change_only_second')
    out = dict((k, np.full((nr, K), np.nan)) for k in names + ('log_p_same_both',))
    out['p_change'] = np.full((nr, K, 2), np.nan)
    out['log_p_same'] = np.full((nr, K, 2), np.nan)
    if len(ok) == 0:
        return out
    masks, labels = event_tables(batch.cn_classes)
    li = LABEL_NAMES.index(label)
    constrain = None if seg_is_original is None else np.ascontiguousarray(np.asarray(seg_is_original) != 0, dtype=np.uint8)
    i, j = adj[ok, 0], adj[ok, 1]
    ends_before = np.concatenate([[0], np.cumsum(np.asarray(is_telomere) != 0)])      # chain ends among model segments < n
    same_chain = ends_before[i] == ends_before[j]
    # no change at one adjacency: the label event over [n, n + 1]
    single = np.zeros((2 * len(ok), 4), dtype=np.int32)
    single[:, 0] = np.concatenate([i, j]); single[:, 1] = single[:, 0] + 1; single[:, 2] = -1; single[:, 3] = li
    ls = np.minimum(batch.region_logprob_raw(r0, nr, single, masks, labels, constrain), 0.).reshape(nr, 2, len(ok))
    la, lb = ls[:, 0], ls[:, 1]
    lab = la + lb                                                                      # (different chains: independent)
    sel = np.flatnonzero(same_chain)
    if len(sel):
        pieces, queries = [], []
        for t in sel:
            if j[t] == i[t] + 1:       # the adjacencies share segment i + 1: one piece binds both
                queries.append((len(pieces), 1, 0, 0))
                pieces.append((i[t], i[t] + 2, -1, li))
            else:
                queries.append((len(pieces), 2, 0, 0))
                pieces.extend([(i[t], i[t] + 1, -1, li), (j[t], j[t] + 1, -1, li)])
        lj = batch.region_pattern_raw(r0, nr, np.array(queries, dtype=np.int32), np.array(pieces, dtype=np.int32), masks, labels, constrain)
        lab[:, sel] = np.minimum(lj, 0.)
    pa, pb, pab = np.exp(la), np.exp(lb), np.exp(lab)
    out['log_p_same'][:, ok, 0], out['log_p_same'][:, ok, 1], out['log_p_same_both'][:, ok] = la, lb, lab
    out['p_change'][:, ok, 0], out['p_change'][:, ok, 1] = -np.expm1(la), -np.expm1(lb)
    out['p_change_both'][:, ok] = np.maximum(1. - pa - pb + pab, 0.)
    out['p_change_neither'][:, ok] = pab
    out['p_change_only_first'][:, ok] = np.maximum(pb - pab, 0.)
    out['p_change_only_second'][:, ok] = np.maximum(pa - pab, 0.)
    return out


def add_breakend_changes(res, changes):
    """Fit result dict `res` gains the five arrays of BREAKEND_ARRAYS (config cn_breakend_changes), breakpoints in the order of
    the experiment's `breakpoints` (the model's)."""
    for k in BREAKEND_ARRAYS:
        res[k] = np.asarray(changes[k], dtype=float)
    return res


# ---- the most probable configuration of a region, and its probability (rmx_region_decode) ----------------
# the arrays of region_calls that go into fit results, records and stores (config cn_region_calls)
REGION_CALL_ARRAYS = ('log_prob', 'log_prob_call', 'n_differ')


def parse_call_event(event):
    """event of region_call: None, or (mask name or None, label name or None) over MASK_NAMES / LABEL_NAMES -> the
    (mask index or -1, label index or -1) of a region query."""
    if event is None:
        return -1, -1
    mask, label = event
    if mask is not None and mask not in MASK_NAMES:
        raise ValueError('unknown mask %r: one of %s' % (mask, ', '.join(MASK_NAMES)))
    if label is not None and label not in LABEL_NAMES:
        raise ValueError('unknown label %r: one of %s' % (label, ', '.join(LABEL_NAMES)))
    return (-1 if mask is None else MASK_NAMES.index(mask)), (-1 if label is None else LABEL_NAMES.index(label))


def batch_region_calls(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, event=None, cn=None):
    """The most probable copy-number configuration of every region under the structured posterior, and its probability,
    for restarts r0 .. r0+nr-1 of a RemixtBatch from one device call per kernel (rmx_region_decode; rmx_region_prob with
    an event; rmx_call_prob with a call).  regions: (first, last) or (name, first, last) experiment segment indices, split
    at chain ends into pieces as region_queries does it, with constrain = seg_is_original: a mask binds real segments
    only, a label every adjacency of a run.  event: None, or (mask name or None, label name or None): the configuration is
    then the most probable one in which the event holds.  A dict of
      cn                    a list over restarts of lists over regions of int arrays (segments of the region, M, 2): the
                            copy numbers of the region's segments through the state tables, its pieces in different chains
                            concatenated (-1 everywhere where the event is impossible);
      log_prob              (nr, R) the log-probability of that configuration of the region's model segments -- the zero-length
                            segments inserted inside it included --, summed over the pieces: chains are independent;
      log_p_event           (nr, R) log P(event) over the same pieces, 0 without an event;
      log_prob_given_event  (nr, R) log_prob - log_p_event, at most 0;
    and, with a call cn -- int (nr, N1) state indices in model segment order, as states_in_model_order gives them --,
      n_differ              int (nr, R) the number of the region's segments where the configuration differs from the call
                            (-1 where the event is impossible);
      log_prob_call         (nr, R) the log-probability that the path takes the call's states at every segment of the region
                            (batch_call_confidence's p_call as a logarithm; inserted segments are marginalised there, so it
                            can exceed log_prob where a region holds some)."""
    mi, li = parse_call_event(event)
    reg = np.array([[int(r[-2]), int(r[-1])] for r in regions], dtype=np.int64).reshape(-1, 2)
    masks, labels = event_tables(batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(reg, seg_fwd_remap, seg_is_original, cs, ce)
    P, R = len(runs), len(reg)
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    classes, seg_class = np.asarray(batch.cn_classes), np.asarray(batch.seg_class)
    out = {'cn': [[] for _ in range(nr)], 'log_prob': np.zeros((nr, R)), 'log_p_event': np.zeros((nr, R)), 'log_prob_given_event': np.zeros((nr, R))}
    if cn is not None:
        out['n_differ'] = np.zeros((nr, R), dtype=np.int64)
        out['log_prob_call'] = np.zeros((nr, R))
    if P == 0:
        return out
    q = np.zeros((P, 4), dtype=np.int32)
    q[:, :2], q[:, 2], q[:, 3] = runs, mi, li
    logp, states = batch.region_decode_raw(r0, nr, q, masks, labels, constrain)
    with np.errstate(invalid='ignore'):
        out['log_prob'] = combine(logp, piece_region, R)
        if event is not None:
            out['log_p_event'] = np.minimum(combine(batch.region_logprob_raw(r0, nr, q, masks, labels, constrain), piece_region, R), 0.)
        # (-inf - -inf: an impossible event has no conditional; a maximum is not above the sum, up to rounding)
        given = out['log_prob'] - out['log_p_event']
    out['log_prob_given_event'] = np.where(np.isnan(given), np.nan, np.minimum(given, 0.))
    call = None
    if cn is not None:
        call = np.asarray(cn).reshape(nr, -1)
        qc = q.copy()
        qc[:, 2], qc[:, 3] = LABEL_NAMES.index('state'), 0
        lpc = batch.call_logprob_raw(r0, nr, call[:, None], qc, labels, constrain)
        out['log_prob_call'] = np.minimum(combine(lpc, piece_region, R), 0.)
    # states of a region's pieces -> model segment order -> the region's own segments
    full = np.full(len(seg_class), -1, dtype=np.int64)
    for r in range(nr):
        for k in range(R):
            seg = fwd[reg[k, 0]:reg[k, 1] + 1]
            full[seg] = -1
            ok = True
            for p in np.flatnonzero(piece_region == k):
                a, b = int(runs[p, 0]), int(runs[p, 1])
                full[a:b + 1] = states[r, p, :b - a + 1]
                ok = ok and np.isfinite(logp[r, p])
            st = full[seg]
            ok = ok and (st >= 0).all()
            out['cn'][r].append(classes[seg_class[seg], st] if ok else np.full((len(seg),) + classes.shape[2:], -1, dtype=classes.dtype))
            if call is not None:
                out['n_differ'][r, k] = int((st != call[r, seg]).sum()) if ok else -1
    return out


def add_region_calls(res, names, calls):
    """Fit result dict `res` gains `region_calls` (config cn_region_calls): the region names and the three arrays of
    REGION_CALL_ARRAYS, (len(names),) each: the log-probability of the region's most probable configuration, that of the
    result's own call over the region, and the number of segments where the two differ.  (The configurations themselves
    come from region_call.)"""
    out = {'names': list(names)}
    for k in REGION_CALL_ARRAYS:
        out[k] = np.asarray(calls[k], dtype=float)
    res['region_calls'] = out
    return res


def region_calls_on(config):
    """Config value cn_region_calls, checked: it needs cn_regions."""
    from . import defaults
    on = bool(defaults.get_param(config, 'cn_region_calls'))
    if on and defaults.get_param(config, 'cn_regions') is None:
        raise ValueError('cn_region_calls needs cn_regions')
    return on


# ---- the K most probable configurations of a region (rmx_region_kbest) -----------------------------------
def combine_kbest(logp, piece_region, num_regions, k):
    """The k best configurations of every region from its pieces' k-best lists.  logp (..., P, K): per piece the
    log-probabilities of its ranks, descending, -inf for an empty rank.  A region cut at chain ends is a product of independent
    pieces, so its k best configurations are the k largest sums of one entry per piece: merged piece by piece over the at
    most k x K candidates of a step, sums taken in piece order, ties to the lower tuple of ranks (in lexicographic order).
    (values (..., num_regions, k), -inf where fewer than k combinations are possible; choice int (..., num_regions, k, P): the
    rank taken of every piece of the region, -1 for the other pieces and for an empty rank).  A NaN in a piece makes every
    value of its region NaN."""
    logp = np.asarray(logp, dtype=float)
    piece_region = np.asarray(piece_region, dtype=np.int64)
    lead, (P, K), R, k = logp.shape[:-2], logp.shape[-2:], int(num_regions), int(k)
    if k < 1:
        raise ValueError('k must be at least 1')
    flat = logp.reshape((-1, P, K))
    values = np.full((flat.shape[0], R, k), -np.inf)
    choice = np.full((flat.shape[0], R, k, P), -1, dtype=np.int64)
    for i in range(flat.shape[0]):
        for reg in range(R):
            pieces = np.flatnonzero(piece_region == reg)
            if np.isnan(flat[i, pieces]).any():
                values[i, reg] = np.nan
                continue
            cur = [(0., ())]      # (sum, ranks of the pieces so far), best first
            for p in pieces:
                cand = [(v + w, t + (j,)) for v, t in cur for j, w in enumerate(flat[i, p]) if w > -np.inf]
                cand.sort(key=lambda c: (-c[0], c[1]))
                cur = cand[:k]
            if len(pieces) == 0:
                cur = []
            for rank, (v, t) in enumerate(cur):
                values[i, reg, rank] = v
                choice[i, reg, rank, pieces] = t
    return values.reshape(lead + (R, k)), choice.reshape(lead + (R, k, P))


def batch_region_alternatives(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, k=4, event=None, cn=None):
    """The k most probable copy-number configurations of every region under the structured posterior, for restarts
    r0 .. r0+nr-1 of a RemixtBatch from one rmx_region_kbest call (and one rmx_region_prob call with an event).  regions, event
    and the pieces as batch_region_calls; cn: None, or the restarts' calls as int (nr, N1) state indices in model segment order.
    A list over restarts of lists over regions of dicts:
      cn                    a list over the found ranks of int arrays (segments of the region, M, 2): the copy numbers of the
                            region's original segments through the state tables, best first;
      log_prob              (k,) the log-probabilities of the configurations of the region's model segments, -inf past the found ranks;
      log_p_event           log P(event) over the same pieces, 0 without an event;
      log_prob_given_event  (k,) log_prob - log_p_event;
      coverage              the sum over the ranks of exp(log_prob_given_event): the share of the event's mass the list explains;
      n_differ              int (k,) the number of the region's segments where a rank differs from the call (-1 past the found
                            ranks and without a call);
      rank_of_call          the first rank whose cn equals the call on the region, -1 if none;
      duplicate_of          int (k,) the first earlier rank with the same cn, else -1.
    Two state paths that differ only inside an inserted zero-length segment are distinct paths with the same copy numbers on
    the region's segments: both are kept, the later one marked in duplicate_of, and their probabilities are not added up (the
    k best of the summed-out law is another question, which this list does not answer)."""
    mi, li = parse_call_event(event)
    k = int(k)
    reg = np.array([[int(r[-2]), int(r[-1])] for r in regions], dtype=np.int64).reshape(-1, 2)
    masks, labels = event_tables(batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(reg, seg_fwd_remap, seg_is_original, cs, ce)
    P, R = len(runs), len(reg)
    if P == 0:
        return [[] for _ in range(nr)]
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    classes, seg_class = np.asarray(batch.cn_classes), np.asarray(batch.seg_class)
    q = np.zeros((P, 4), dtype=np.int32)
    q[:, :2], q[:, 2], q[:, 3] = runs, mi, li
    logp, states = batch.region_kbest_raw(r0, nr, q, k, masks, labels, constrain)
    values, choice = combine_kbest(logp, piece_region, R, k)
    log_p_event = np.zeros((nr, R))
    if event is not None:
        with np.errstate(invalid='ignore'):
            log_p_event = np.minimum(combine(batch.region_logprob_raw(r0, nr, q, masks, labels, constrain), piece_region, R), 0.)
    call = None if cn is None else np.asarray(cn).reshape(nr, -1)
    out = []
    full = np.full(len(seg_class), -1, dtype=np.int64)
    for r in range(nr):
        row = []
        for g in range(R):
            seg = fwd[reg[g, 0]:reg[g, 1] + 1]
            pieces = np.flatnonzero(piece_region == g)
            found = int(np.isfinite(values[r, g]).sum())
            paths = []
            for rank in range(found):
                for p in pieces:
                    a, b = int(runs[p, 0]), int(runs[p, 1])
                    full[a:b + 1] = states[r, p, choice[r, g, rank, p], :b - a + 1]
                paths.append(full[seg].copy())
            with np.errstate(invalid='ignore'):
                given = values[r, g] - log_p_event[r, g]
            n_differ = np.full(k, -1, dtype=np.int64)
            duplicate_of = np.full(k, -1, dtype=np.int64)
            rank_of_call = -1
            for rank, st in enumerate(paths):
                same = [j for j in range(rank) if np.array_equal(paths[j], st)]
                duplicate_of[rank] = same[0] if same else -1
                if call is not None:
                    n_differ[rank] = int((st != call[r, seg]).sum())
                    if rank_of_call < 0 and n_differ[rank] == 0:
                        rank_of_call = rank
            row.append({'cn': [classes[seg_class[seg], st] for st in paths], 'log_prob': values[r, g].copy(), 'log_p_event': float(log_p_event[r, g]),
                        'log_prob_given_event': given, 'coverage': float(np.exp(given[:found]).sum()), 'n_differ': n_differ,
                        'rank_of_call': rank_of_call, 'duplicate_of': duplicate_of})
        out.append(row)
    return out


# ---- distribution of a region's peak and lowest copy number (rmx_region_extremes) ------------------------
LEVEL_QUANTITIES = ('total', 'major', 'minor')
LEVEL_ORIENTATIONS = ('peak', 'floor')
EXTREME_QUANTILES = (0.05, 0.5, 0.95)
# the arrays of region_cn_extremes that go into fit results, records and stores (config cn_region_extremes): (regions, M - 1, bins) each
EXTREME_ARRAYS = ('peak_total_pmf', 'floor_total_pmf')
EXTREME_BINS = 16


def _level_quantity(cn_classes, quantity):
    """(C, S, M - 1): the quantity of every tumour clone."""
    tum = np.asarray(cn_classes)[:, :, 1:, :].astype(np.int64)
    if quantity == 'total':
        return tum.sum(axis=-1)
    if quantity == 'major':
        return tum.max(axis=-1)
    if quantity == 'minor':
        return tum.min(axis=-1)
    raise ValueError('unknown quantity %r: one of %s' % (quantity, ', '.join(LEVEL_QUANTITIES)))


def level_name(orientation, quantity, clone):
    """The name of a level table: '<peak|floor>_<total|major|minor>_<tumour clone 1 .. M-1, or any>'."""
    if orientation not in LEVEL_ORIENTATIONS:
        raise ValueError('unknown orientation %r: one of %s' % (orientation, ', '.join(LEVEL_ORIENTATIONS)))
    if quantity not in LEVEL_QUANTITIES:
        raise ValueError('unknown quantity %r: one of %s' % (quantity, ', '.join(LEVEL_QUANTITIES)))
    return '%s_%s_%s' % (orientation, quantity, clone)


def level_tables(cn_classes, ncol, first_level=0):
    """Level tables of the region extremes: (levels int16 (C, T, S), names), T = 2 * 3 * M tables named by level_name, the
    orientations outermost, then the quantities, then the tumour clones 1 .. M-1 and 'any'.  The quantities of a clone are
    its total, major (the larger allele) and minor copy number; 'any' is the maximum over the tumour clones under 'peak' and
    the minimum under 'floor'.  With q the quantity and w = clip(q - first_level, 0, ncol - 1),
      peak   the level is w: column j of rmx_region_extremes is "q <= first_level + j throughout", and because of the clip the
             last column is the mask-only event (the last bin means first_level + ncol - 1 or more);
      floor  the level is ncol - 1 - w: column j is "q >= first_level + ncol - 1 - j throughout" (the bin of w = 0 means
             first_level or less)."""
    cn = np.asarray(cn_classes)
    if cn.ndim != 4 or cn.shape[3] != 2 or cn.shape[2] < 2:
        raise ValueError('cn_classes must have shape (num_classes, num_cn_states, num_clones >= 2, 2)')
    ncol, first_level = int(ncol), int(first_level)
    if not 1 <= ncol <= 16:
        raise ValueError('ncol must be in 1 .. 16')
    if first_level < 0:
        raise ValueError('first_level must not be negative')
    M = cn.shape[2]
    tabs, names = [], []
    for orient in LEVEL_ORIENTATIONS:
        for quantity in LEVEL_QUANTITIES:
            q = _level_quantity(cn, quantity)
            cols = [q[:, :, m] for m in range(M - 1)] + [q.max(axis=-1) if orient == 'peak' else q.min(axis=-1)]
            for clone, v in zip(list(range(1, M)) + ['any'], cols):
                w = np.clip(v - first_level, 0, ncol - 1)
                tabs.append(w if orient == 'peak' else ncol - 1 - w)
                names.append(level_name(orient, quantity, clone))
    return np.ascontiguousarray(np.stack(tabs, axis=1).astype(np.int16)), names


def combine_columns(logp, piece_region, num_regions):
    """Every region's columns from its pieces': logp (..., pieces, ncol) -> (..., num_regions, ncol), the pieces' logs added
    per column.  Chains are independent under the structured posterior and "in the mask and at or below the threshold at
    every segment" is a conjunction over segments, so column j of a region split at chain ends is the product of its pieces'
    column j."""
    return np.moveaxis(combine(np.moveaxis(np.asarray(logp, dtype=float), -1, -2), piece_region, num_regions), -1, -2)


def _quantile_bins(cdf):
    """cdf (..., bins), non-decreasing with last entry 1 -> int (..., 3): the first bin at which it reaches each of
    EXTREME_QUANTILES (the last bin where rounding keeps it below)."""
    out = np.zeros(cdf.shape[:-1] + (len(EXTREME_QUANTILES),), dtype=np.int64)
    for i, qv in enumerate(EXTREME_QUANTILES):
        reached = cdf >= qv
        out[..., i] = np.where(reached.any(axis=-1), reached.argmax(axis=-1), cdf.shape[-1] - 1)
    return out


def extremes_summary(peak_logcdf, floor_logsurv, first_level=0):
    """The arrays of region_cn_extremes from the two families of columns (..., bins): peak_logcdf[..., j] = log P(peak <=
    first_level + j) (the last one the mask-only event), floor_logsurv[..., k] = log P(lowest >= first_level + k) (the first
    one the mask-only event).  pmfs are differences of the exponentials, clipped to [0, 1]: a CDF that dips by an ulp gives
    0, not a negative number.  Quantiles are copy numbers; a saturated bin is reported as its edge (first_level + bins - 1
    for a peak of that or more, first_level for a lowest value of that or less)."""
    with np.errstate(over='ignore'):
        pc = np.clip(np.exp(np.minimum(np.asarray(peak_logcdf, dtype=float), 0.)), 0., 1.)
        fs = np.clip(np.exp(np.minimum(np.asarray(floor_logsurv, dtype=float), 0.)), 0., 1.)
    bins = pc.shape[-1]
    zero = np.zeros(pc.shape[:-1] + (1,))
    out = {'bins': bins, 'first_level': int(first_level), 'peak_cdf': pc, 'floor_cdf': fs,
           'peak_pmf': np.clip(np.diff(np.concatenate([zero, pc], axis=-1), axis=-1), 0., 1.),
           'floor_pmf': np.clip(-np.diff(np.concatenate([fs, zero], axis=-1), axis=-1), 0., 1.)}
    # the lowest value's own CDF, P(lowest <= first_level + k) = 1 - P(lowest >= first_level + k + 1)
    low = 1. - np.concatenate([fs[..., 1:], zero], axis=-1)
    for name, cdf in (('peak', pc), ('floor', low)):
        qb = _quantile_bins(cdf) + int(first_level)
        for i, qv in enumerate(EXTREME_QUANTILES):
            out['%s_q%02d' % (name, int(round(qv * 100)))] = qb[..., i]
    return out


def _extreme_columns(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, levels, bins):
    """F (nr, T, R, bins): the columns of every region under each of the T level tables `levels` (C, T, S), no mask, from one device
    call: one query per region piece and table, the pieces of a region joined per column."""
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    P, R, T = len(runs), len(np.asarray(regions).reshape(-1, 2)), levels.shape[1]
    if P == 0:
        return np.zeros((nr, T, 0, bins))
    q = np.zeros((T, P, 4), dtype=np.int32)
    q[:, :, :2] = runs[None]
    q[:, :, 2] = -1
    q[:, :, 3] = np.arange(T)[:, None]
    logp = batch.region_extremes_raw(r0, nr, q.reshape(-1, 4), None, levels, constrain, bins).reshape(nr, T, P, bins)
    return combine_columns(logp, piece_region, R)


def batch_region_cn_extremes(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, quantity='total', clone='any', bins=16, first_level=0):
    """The exact posterior distribution of the highest and of the lowest copy number over regions, for restarts r0 ..
    r0+nr-1 of a RemixtBatch from one device call (rmx_region_extremes).  quantity: 'total', 'major' or 'minor'; clone: a
    tumour clone 1 .. M-1, or 'any' (the peak is then the highest over the tumour clones, the lowest value the lowest); the
    window is first_level .. first_level + bins - 1, bins in 1 .. 16.  The extremes run over the region's real segments:
    a zero-length segment inserted at a breakend does not count.  regions: (first, last) experiment segment indices.
    A dict of `bins`, `first_level` and, per restart and region,
      peak_cdf   (nr, R, bins)  P(peak <= first_level + k); the last entry is 1: that bin means first_level + bins - 1 or more
      peak_pmf   (nr, R, bins)  its differences, clipped to [0, 1]
      floor_cdf  (nr, R, bins)  P(lowest >= first_level + k); the first entry is 1: that bin means first_level or less
      floor_pmf  (nr, R, bins)  P(lowest == first_level + k), from its differences
      peak_q05, peak_q50, peak_q95, floor_q05, floor_q50, floor_q95   int (nr, R): quantiles as copy numbers, a saturated
                 bin reported as its edge."""
    bins = int(bins)
    if not 1 <= bins <= 16:
        raise ValueError('bins must be in 1 .. 16')
    levels, names = level_tables(batch.cn_classes, bins, first_level)
    M = np.asarray(batch.cn_classes).shape[2]
    if clone != 'any' and not (isinstance(clone, (int, np.integer)) and 1 <= clone < M):
        raise ValueError('clone must be a tumour clone 1 .. %d or \'any\'' % (M - 1))
    pick = [names.index(level_name(o, quantity, clone)) for o in LEVEL_ORIENTATIONS]
    F = _extreme_columns(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, levels[:, pick], bins)
    # floor column j is "lowest >= first_level + bins - 1 - j": reversed, entry k is "lowest >= first_level + k"
    return extremes_summary(F[:, 0], F[:, 1, :, ::-1], first_level)


def amplification_prob(extremes, threshold):
    """P(peak >= threshold) of a batch_region_cn_extremes result: 1 - P(peak <= threshold - 1).  The threshold has to lie in
    the window's resolved part, first_level + 1 .. first_level + bins - 1 (or at most 0: certain)."""
    k = int(threshold) - int(extremes['first_level'])
    cdf = np.asarray(extremes['peak_cdf'])
    if int(threshold) <= 0:
        return np.ones(cdf.shape[:-1])
    if not 1 <= k <= cdf.shape[-1] - 1:
        raise ValueError('threshold outside first_level + 1 .. first_level + bins - 1: slide the window with first_level')
    return np.clip(1. - cdf[..., k - 1], 0., 1.)


def add_region_cn_extremes(res, names, extremes):
    """Fit result dict `res` gains `region_cn_extremes` (config cn_region_extremes): the region names, the number of bins and
    the arrays of EXTREME_ARRAYS, (len(names), M - 1, bins) each, one row per tumour clone: the distributions of the peak and
    of the lowest total copy number of the clone over the region, from 0 (the last bin: bins - 1 or more)."""
    out = {'names': list(names), 'bins': int(np.asarray(extremes[EXTREME_ARRAYS[0]]).shape[-1])}
    for k in EXTREME_ARRAYS:
        out[k] = np.asarray(extremes[k], dtype=float)
    res['region_cn_extremes'] = out
    return res


def batch_clone_extremes(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, bins=EXTREME_BINS):
    """The arrays of EXTREME_ARRAYS, (nr, R, M - 1, bins) each, from one device call: batch_region_cn_extremes' peak_pmf and
    floor_pmf of the total copy number of every tumour clone, window 0 .. bins - 1."""
    levels, names = level_tables(batch.cn_classes, bins, 0)
    M = np.asarray(batch.cn_classes).shape[2]
    pick = [names.index(level_name(o, 'total', m)) for o in LEVEL_ORIENTATIONS for m in range(1, M)]
    F = _extreme_columns(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, levels[:, pick], bins)
    F = F.reshape(nr, 2, M - 1, F.shape[2], bins)
    s = extremes_summary(F[:, 0], F[:, 1, ..., ::-1], 0)
    return {'peak_total_pmf': np.moveaxis(s['peak_pmf'], 1, 2), 'floor_total_pmf': np.moveaxis(s['floor_pmf'], 1, 2)}


def region_extremes_on(config):
    """Config value cn_region_extremes, checked: it needs cn_regions."""
    from . import defaults
    on = bool(defaults.get_param(config, 'cn_region_extremes'))
    if on and defaults.get_param(config, 'cn_regions') is None:
        raise ValueError('cn_region_extremes needs cn_regions')
    return on


# ---- overlap between two restarts' structured posteriors (rmx_restart_overlap) ----
OVERLAP_MODES = (('log_overlap', 0), ('log_coincidence', 1))


def clone_permutations(num_clones):
    """The (M - 1)! orders of the tumour clones as clone maps, identity first: tuples p of length M with p[0] == 0 (the normal
    clone stays) -- clone m of restart A is compared with clone p[m] of restart B."""
    import itertools
    return [(0,) + p for p in itertools.permutations(range(1, int(num_clones)))]


def state_permutation_tables(cn_classes, perms):
    """int16 (P, C, S): for every clone map of `perms` and every state class, the state index of B that a state index of A is
    compared with -- the table entry whose clone p[m] carries the copy numbers of A's clone m.  A state table holds one
    representative of {state, both alleles swapped in every clone} (cn_model.create_cn_states), so the image is the entry equal
    to the permuted copy numbers or to their allele swap; a table without such an entry is a ValueError."""
    cn = np.asarray(cn_classes, dtype=np.int64)
    C_, S, M = cn.shape[:3]
    out = np.zeros((len(perms), C_, S), dtype=np.int16)
    for c in range(C_):
        index = dict((cn[c, s].tobytes(), s) for s in range(S))
        for i, p in enumerate(perms):
            p = np.asarray(p, dtype=np.int64)
            if sorted(p.tolist()) != list(range(M)) or p[0] != 0:
                raise ValueError('a clone map is a permutation of the clones that keeps the normal clone')
            target = np.zeros_like(cn[c])
            target[:, p] = cn[c]
            for s in range(S):
                t = index.get(target[s].tobytes())
                if t is None:
                    t = index.get(np.ascontiguousarray(target[s, :, ::-1]).tobytes())
                if t is None:
                    raise ValueError('state table %d has no entry for state %d under the clone map %s' % (c, s, tuple(p.tolist())))
                out[i, c, s] = t
    return out


def batch_restart_overlap(batches, offsets, pairs, regions, seg_fwd_remap, seg_is_original, is_telomere, perm_tables, mode):
    """log Z (npairs, len(regions), nmaps) of rmx_restart_overlap's `mode` for pairs of restarts over experiment-order
    regions, under every state permutation of perm_tables (nmaps, C, S).  The restarts are those of `batches` in order,
    batch g holding restarts offsets[g] .. offsets[g + 1] - 1; a pair may straddle two batches.  Chains are independent
    under the structured posterior, so a region's log Z is the sum over its pieces (region_queries, combine).  One device
    call per pair of batches that the pairs touch."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    offsets = np.asarray(offsets, dtype=np.int64)
    if len(pairs) and (pairs.min() < 0 or pairs.max() >= offsets[-1]):
        raise ValueError('a pair names a restart outside the set')
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, _ = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    P, R, nmaps = len(runs), len(np.asarray(regions).reshape(-1, 2)), len(perm_tables)
    out = np.zeros((len(pairs), R, nmaps))
    if P == 0 or len(pairs) == 0:
        return out
    q = np.zeros((nmaps, P, 4), dtype=np.int32)
    q[:, :, :2] = runs[None]
    q[:, :, 2] = np.arange(nmaps)[:, None]
    group = np.searchsorted(offsets, pairs, side='right') - 1      # the batch of either side
    for ga, gb in sorted(set(map(tuple, group.tolist()))):
        sel = np.flatnonzero((group[:, 0] == ga) & (group[:, 1] == gb))
        local = pairs[sel] - offsets[[ga, gb]][None]
        logz = batches[ga].restart_overlap_raw(batches[gb], local, q.reshape(-1, 4), perm_tables, mode).reshape(len(sel), nmaps, P)
        out[sel] = np.moveaxis(combine(logz, piece_region, R), 1, 2)
    return out


def cluster_restarts(distance, threshold):
    """Single-linkage clusters of restarts: i and j share a cluster when a chain of restarts joins them whose consecutive
    distances are all <= threshold.  distance: symmetric (R, R) (NaN: no link).  Returns int labels (R,), numbered in the order
    of each cluster's first member."""
    d = np.asarray(distance, dtype=float)
    R = d.shape[0]
    if d.shape != (R, R):
        raise ValueError('distance must be a square matrix')
    with np.errstate(invalid='ignore'):
        link = (d <= threshold) | (d.T <= threshold)
    labels = np.full(R, -1, dtype=np.int64)
    k = 0
    for i in range(R):
        if labels[i] >= 0:
            continue
        labels[i] = k
        todo = [i]
        while todo:
            j = todo.pop()
            for m in np.flatnonzero(link[j] & (labels < 0)):
                labels[m] = k
                todo.append(int(m))
        k += 1
    return labels


def pair_matrix(pairs, values, num_restarts, diagonal=0.):
    """Symmetric (R, R) matrix of a per-pair value (NaN where no pair was computed; `diagonal` on the diagonal)."""
    out = np.full((num_restarts, num_restarts), np.nan)
    np.fill_diagonal(out, diagonal)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out[pr[:, 0], pr[:, 1]] = values
    out[pr[:, 1], pr[:, 0]] = values
    return out


def overlap_summary(pairs, clone_maps, log_overlap, log_coincidence, self_log_coincidence, num_real_segments):
    """What .restart_overlap returns, from the raw sums: `pairs` (npairs, 2), `clone_maps`, `log_overlap` and `log_coincidence`
    (npairs, nreg + 1, nmaps; the whole genome is the last region), `clone_map` (npairs,): the map with the largest
    whole-genome log overlap, `hellinger` (npairs, nreg): the Hellinger distance sqrt(1 - BC) of every region at that map,
    `distance_rate` (npairs, nmaps): -log BC of the genome per real segment -- BC of a whole genome multiplies over tens of
    thousands of segments and is 0 for any two distinct fits, the rate is the number to cluster on --, and
    `self_log_coincidence` (R, nreg + 1): the log collision probability of every restart's own region posterior."""
    lo = np.asarray(log_overlap, dtype=float)
    npairs = lo.shape[0]
    best = np.zeros(npairs, dtype=np.int64)
    if npairs:
        with np.errstate(invalid='ignore'):
            best = np.argmax(np.where(np.isnan(lo[:, -1, :]), -np.inf, lo[:, -1, :]), axis=1)
    at = lo[np.arange(npairs), :-1, best] if npairs else np.zeros((0, lo.shape[1] - 1))
    with np.errstate(invalid='ignore'):
        hell = np.sqrt(np.maximum(-np.expm1(np.minimum(at, 0.)), 0.))
    return {'pairs': np.asarray(pairs, dtype=np.int64).reshape(-1, 2), 'clone_maps': [tuple(int(v) for v in p) for p in clone_maps],
            'log_overlap': lo, 'log_coincidence': np.asarray(log_coincidence, dtype=float), 'clone_map': best, 'hellinger': hell,
            'distance_rate': -lo[:, -1, :] / float(num_real_segments), 'self_log_coincidence': np.asarray(self_log_coincidence, dtype=float)}


def restart_overlap(batches, counts, model, regions=None, pairs=None, clone_maps='all'):
    """The exact overlap between the restarts of `batches` (RemixtBatch objects of one problem on one device; batch g holds
    counts[g] restarts; `model`: any of their BreakpointModels, for the segment maps): overlap_summary of the Bhattacharyya
    overlap and the coincidence probability of every pair (default: all i < j across the batches) over `regions`
    ((first, last) experiment segments; the whole genome is always appended) under every clone map (default 'all':
    clone_permutations)."""
    if any(b is None or not hasattr(b, 'restart_overlap_raw') for b in batches):
        raise NotImplementedError('restart_overlap needs the device batches of the HIP library')
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    R = int(offsets[-1])
    cn_classes = np.asarray(batches[0].cn_classes)
    maps = clone_permutations(cn_classes.shape[2]) if isinstance(clone_maps, str) and clone_maps == 'all' else [tuple(p) for p in clone_maps]
    tables = state_permutation_tables(cn_classes, maps)
    if pairs is None:
        pairs = [(i, j) for i in range(R) for j in range(i + 1, R)]
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    reg = genome_region([] if regions is None else regions, len(model.seg_fwd_remap))
    args = (reg, model.seg_fwd_remap, model.seg_is_original, model.is_telomere)
    raw = dict((name, batch_restart_overlap(batches, offsets, pairs, *args, tables, mode)) for name, mode in OVERLAP_MODES)
    own = np.stack([np.arange(R), np.arange(R)], axis=1)
    self_lc = batch_restart_overlap(batches, offsets, own, *args, tables[:1], 1)[:, :, 0]
    return overlap_summary(pairs, maps, raw['log_overlap'], raw['log_coincidence'], self_lc, int(np.count_nonzero(model.seg_is_original)))


# ---- per-segment posteriors given that an event holds (rmx_region_conditional) ----------------------------
# the arrays of unpack a conditional summary holds (the row entropy is not computed given an event)
CONDITIONAL_ARRAYS = ('total_cn_mean', 'total_cn_sd', 'expected_alleles_subclonal', 'p_subclonal', 'p_loh', 'p_hdel', 'cn_posterior_max', 'cn_mpm')
_CONDITIONAL_MAX_SLOTS = 16384
_CONDITIONAL_MAX_Q = 64


def conditional_event(event, cn_classes):
    """The evidence of a conditional summary as tables and indices: (masks (C, nmask, S), labels (C, nlabel, S), mask index or
    -1, label index or -1).  event: as parse_event takes it, over the tables of event_tables, or a boolean (C, S) table of the
    states the evidence allows (one mask of its own, no label)."""
    if not isinstance(event, (str, tuple, list)) and np.ndim(event) == 2:
        table = np.asarray(event)
        cn = np.asarray(cn_classes)
        if table.shape != cn.shape[:2]:
            raise ValueError('a mask table must have shape (num_classes, num_cn_states)')
        return np.ascontiguousarray((table != 0)[:, None, :], dtype=np.uint8), None, 0, -1
    mi, li = parse_event(event)
    masks, labels = event_tables(cn_classes)
    return masks, labels, mi, li


def conditional_queries(regions, window, seg_fwd_remap, seg_is_original, chain_start, chain_end):
    """Regions ((first, last) experiment segment indices) and a window as the runs and windows of rmx_region_conditional:
    (runs int32 (P, 2), windows int32 (P, 2), piece_region (P,), constrain uint8 (N1,)).  The runs are region_queries': a
    region that spans chains is one piece per chain.  window: 'chain' -- every piece's whole chain -- or the number of model
    segments on either side of the piece, cut at its chain's ends."""
    runs, piece_region, constrain = region_queries(regions, seg_fwd_remap, seg_is_original, chain_start, chain_end)
    cs, ce = np.asarray(chain_start, dtype=np.int64), np.asarray(chain_end, dtype=np.int64)
    chain = np.searchsorted(ce, runs[:, 0], side='left')
    if isinstance(window, str):
        if window != 'chain':
            raise ValueError("a window is 'chain' or a number of segments, not %r" % (window,))
        lo, hi = cs[chain], ce[chain]
    else:
        if np.ndim(window) != 0 or int(window) != window or int(window) < 0:
            raise ValueError("a window is 'chain' or a number of segments >= 0, not %r" % (window,))
        lo, hi = np.maximum(runs[:, 0] - int(window), cs[chain]), np.minimum(runs[:, 1] + int(window), ce[chain])
    windows = np.stack([lo, hi], axis=1).astype(np.int32).reshape(-1, 2)
    if len(windows) and (windows[:, 1] - windows[:, 0] + 1).max() > _CONDITIONAL_MAX_SLOTS:
        raise ValueError('a window holds at most %d model segments' % _CONDITIONAL_MAX_SLOTS)
    return runs, windows, piece_region, constrain


def conditional_unpack(logp, out, windows, piece_region, num_regions, layout, cn_classes, seg_class, seg_fwd_remap, with_prob):
    """One restart's rows of rmx_region_conditional (logp (P,), out (P, nslot, Q + 3)) as one dict per region: `log_evidence`,
    the sum over the region's pieces -- chains are independent under the structured posterior, so every chain's window is
    conditioned on its own piece --, and the arrays of unpack without the entropy, in experiment segment order (inserted
    segments dropped), NaN outside the windows (cn_mpm: -1) and everywhere where the evidence cannot happen."""
    N1, Q = len(seg_class), layout['Q']
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    log_ev = combine(np.asarray(logp, dtype=float), piece_region, num_regions)
    res = []
    for R in range(int(num_regions)):
        proj = np.full((N1, Q), np.nan)
        stats = np.full((N1, 3), np.nan)
        amax = np.zeros(N1, dtype=np.int64)
        for p in np.flatnonzero(np.asarray(piece_region) == R):
            lo, hi = int(windows[p, 0]), int(windows[p, 1])
            rows = np.asarray(out[p, :hi - lo + 1])
            proj[lo:hi + 1] = rows[:, :Q]
            stats[lo:hi + 1, 0], stats[lo:hi + 1, 2] = rows[:, Q], rows[:, Q + 2]
            amax[lo:hi + 1] = np.where(np.isnan(rows[:, Q + 1]), 0, rows[:, Q + 1]).astype(np.int64)
        s = unpack(proj, stats, amax, layout, cn_classes, seg_class)
        del s['cn_posterior_entropy']
        if not with_prob:
            del s['cn_posterior_prob']
        s['cn_mpm'] = np.where(np.isnan(stats[:, 0])[:, None, None], -1, s['cn_mpm'])
        s = dict((k, v[fwd]) for k, v in s.items())
        s['log_evidence'] = float(log_ev[R])
        res.append(s)
    return res


def batch_conditional_summary(batch, r0, nr, regions, event, window, seg_fwd_remap, seg_is_original, is_telomere, marginals=False, states=None):
    """Exact per-segment summaries given that an event holds over a region, for restarts r0 .. r0+nr-1 of a RemixtBatch from
    one device call: a list over restarts of lists over regions of conditional_unpack dicts.  regions: (first, last)
    experiment segment indices; event: conditional_event; window: conditional_queries; marginals: the one-hot columns of
    feature_matrix too (cn_marginals), where they fit 64 weight columns; states: int16 (nr, N1) decoded states in model order
    for cn_posterior_prob given the event, or None (the key is then left out)."""
    weights, layout = feature_matrix(batch.cn_classes, marginals)
    if layout['Q'] > _CONDITIONAL_MAX_Q:
        raise ValueError('a conditional summary takes at most %d weight columns, %d asked for (marginals=%r)' % (_CONDITIONAL_MAX_Q, layout['Q'], marginals))
    masks, labels, mi, li = conditional_event(event, batch.cn_classes)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, windows, piece_region, constrain = conditional_queries(regions, window, seg_fwd_remap, seg_is_original, cs, ce)
    R = len(np.asarray(regions).reshape(-1, 2))
    if len(runs) == 0:
        return [[] for _ in range(nr)]
    q = np.zeros((len(runs), 4), dtype=np.int32)
    q[:, :2], q[:, 2], q[:, 3] = runs, mi, li
    logp, out = batch.region_conditional_raw(r0, nr, q, windows, masks, labels, constrain, weights, states)
    return [conditional_unpack(logp[i], out[i], windows, piece_region, R, layout, batch.cn_classes, batch.seg_class, seg_fwd_remap, states is not None)
            for i in range(nr)]


def evidence_shift(conditional, unconditional, l=None):
    """What the evidence changes: for one region's conditional summary (conditional_unpack) and the unconditional summary of
    the same restart (unpack, experiment order), the differences conditional - unconditional of the floating-point arrays
    both hold, NaN outside the window; `cn_mpm_changed`, whether the marginal arg-max moved (False outside the window);
    `log_evidence`; and with segment lengths l (experiment order) `ploidy_before` and `ploidy_after`, summary_stats'
    ploidy_posterior_mean over the segments of the window alone."""
    out = {'log_evidence': conditional['log_evidence']}
    for k, v in conditional.items():
        if k in unconditional and np.asarray(v).dtype.kind == 'f' and np.ndim(v) >= 1:
            out[k] = np.asarray(v) - np.asarray(unconditional[k])
    inside = ~np.isnan(np.asarray(conditional['cn_posterior_max']))
    if 'cn_mpm' in unconditional:
        out['cn_mpm_changed'] = inside & np.any(np.asarray(conditional['cn_mpm']) != np.asarray(unconditional['cn_mpm']), axis=(1, 2))
    if l is not None:
        lw = np.asarray(l, dtype=float)[inside]
        for name, s in (('ploidy_before', unconditional), ('ploidy_after', conditional)):
            part = {'total_cn_mean': np.asarray(s['total_cn_mean'])[inside], 'expected_alleles_subclonal': np.asarray(s['expected_alleles_subclonal'])[inside]}
            out[name] = summary_stats(part, lw)['ploidy_posterior_mean'] if inside.any() and lw.sum() > 0 else float('nan')
    return out


# ---- joint posterior of copy number at two loci of a chain (rmx_locus_joint) ------------------------------
JOINT_ARRAYS = ('joint', 'marginal_a', 'marginal_b', 'p_equal', 'p_a_higher', 'p_b_higher', 'difference_pmf', 'mean_difference', 'correlation',
                'mutual_information', 'p_saturated')
DEPENDENCE_ARRAYS = ('mutual_information', 'correlation', 'p_equal')
_LOCUS_MAX_SLOTS = 4096
_LOCUS_HOST_BYTES = 256 << 20      # the tables one device call of batch_locus_dependence brings back


def locus_level_tables(cn_classes, bins, first_level=0):
    """Level tables of the locus joints: (levels int16 (C, T, S), names).  First the 3 * M 'peak' tables of level_tables,
    named 'peak_<quantity>_<clone>' -- clip(q - first_level, 0, bins - 1) of a clone's (or the tumour clones' highest) total,
    major or minor copy number, the last bin meaning first_level + bins - 1 or more --, then one 0/1 table per mask of
    event_tables, named as in MASK_NAMES: level 1 where the event holds."""
    levels, names = level_tables(cn_classes, bins, first_level)
    half = len(names) // 2
    masks, _ = event_tables(cn_classes)
    tabs = np.concatenate([levels[:, :half], masks.astype(np.int16)], axis=1)
    return np.ascontiguousarray(tabs), names[:half] + list(MASK_NAMES)


def locus_feature_name(feature, num_clones):
    """The table name of a feature: (quantity, clone) with quantity in LEVEL_QUANTITIES and clone 1 .. M-1 or 'any', or a name
    of MASK_NAMES."""
    if isinstance(feature, str):
        if feature not in MASK_NAMES:
            raise ValueError('unknown feature %r: a (quantity, clone) pair or one of %s' % (feature, ', '.join(MASK_NAMES)))
        return feature
    try:
        quantity, clone = feature
    except (TypeError, ValueError):
        raise ValueError('a feature is a (quantity, clone) pair or one of %s' % ', '.join(MASK_NAMES))
    if clone != 'any' and not (isinstance(clone, (int, np.integer)) and 1 <= clone < num_clones):
        raise ValueError('clone must be a tumour clone 1 .. %d or \'any\'' % (num_clones - 1))
    return level_name('peak', quantity, clone)


def locus_queries(pairs, seg_fwd_remap, chain_start, chain_end):
    """Pairs of experiment segments (P, 2), in any order, as model segments: (segs int32 (P, 2) ordered left, right; swapped
    bool (P,), whether the pair's first locus is the right one; cross bool (P,), whether the two lie in different chains)."""
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    if len(pr) and (pr.min() < 0 or pr.max() >= len(fwd)):
        raise ValueError('a locus needs 0 <= segment < number of segments')
    seg = fwd[pr]
    swapped = seg[:, 0] > seg[:, 1]
    segs = np.where(swapped[:, None], seg[:, ::-1], seg).astype(np.int32)
    ce = np.asarray(chain_end, dtype=np.int64)
    cross = np.searchsorted(ce, segs[:, 0], side='left') != np.searchsorted(ce, segs[:, 1], side='left')
    return segs, swapped, cross


def joint_summary(log_joint, first_level=0):
    """What a table of two levels says, log_joint (..., bins, bins) with locus a along axis -2 and locus b along axis -1: a dict of
      joint             (..., bins, bins)    exp(log_joint)
      marginal_a, marginal_b  (..., bins)    its row and column sums
      p_equal, p_a_higher, p_b_higher (...)  the mass on, below and above the diagonal
      difference_pmf    (..., 2 bins - 1)    of level(a) - level(b), entry d + bins - 1
      mean_difference   (...)
      correlation       (...)                of the two levels; NaN where a marginal is degenerate
      mutual_information (...)               in nats, clipped at 0
      p_saturated       (...)                the mass with either level in the last, "or more" bin, where differences are not resolved.
    Correlation and mutual information are those of the table divided by its sum (it is 1 for tables that cover every state).
    A table with a NaN gives NaN.  first_level is carried for the caller: differences do not depend on it."""
    lj = np.asarray(log_joint, dtype=float)
    bins = lj.shape[-1]
    if lj.shape[-2] != bins:
        raise ValueError('log_joint must have shape (..., bins, bins)')
    with np.errstate(over='ignore', invalid='ignore'):
        J = np.exp(lj)
    ma, mb = J.sum(axis=-1), J.sum(axis=-2)
    lev = np.arange(bins)
    d = lev[:, None] - lev[None, :]
    out = {'joint': J, 'marginal_a': ma, 'marginal_b': mb,
           'p_equal': np.where(d == 0, J, 0.).sum(axis=(-2, -1)), 'p_a_higher': np.where(d > 0, J, 0.).sum(axis=(-2, -1)),
           'p_b_higher': np.where(d < 0, J, 0.).sum(axis=(-2, -1))}
    pmf = np.zeros(J.shape[:-2] + (2 * bins - 1,))
    for k in range(-(bins - 1), bins):
        pmf[..., k + bins - 1] = np.where(d == k, J, 0.).sum(axis=(-2, -1))
    out['difference_pmf'] = pmf
    out['mean_difference'] = (pmf * np.arange(-(bins - 1), bins)).sum(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        tot = J.sum(axis=(-2, -1))
        P = J / tot[..., None, None]
        pa, pb = P.sum(axis=-1), P.sum(axis=-2)
        ea, eb = (pa * lev).sum(axis=-1), (pb * lev).sum(axis=-1)
        va, vb = (pa * lev ** 2).sum(axis=-1) - ea ** 2, (pb * lev ** 2).sum(axis=-1) - eb ** 2
        cov = (P * (lev[:, None] * lev[None, :])).sum(axis=(-2, -1)) - ea * eb
        degenerate = (pa.max(axis=-1) >= 1.) | (pb.max(axis=-1) >= 1.) | ~(va > 0) | ~(vb > 0)
        corr = np.where(degenerate, np.nan, cov / np.sqrt(np.where(degenerate, 1., va * vb)))
        out['correlation'] = np.where(np.isnan(tot), np.nan, np.clip(corr, -1., 1.))
        # (the logarithms apart: the product of two marginals near 1e-200 is 0 in double, their cell is not)
        lp, la, lb = (np.log(np.where(x > 0, x, 1.)) for x in (P, pa, pb))
        mi = np.where(P > 0, P * (lp - la[..., :, None] - lb[..., None, :]), 0.).sum(axis=(-2, -1))
        out['mutual_information'] = np.where(np.isnan(tot) | ~(tot > 0), np.nan, np.maximum(mi, 0.))
    last = (lev[:, None] == bins - 1) | (lev[None, :] == bins - 1)
    out['p_saturated'] = np.where(last, J, 0.).sum(axis=(-2, -1))
    return out


def _locus_tables(batch, feature, other, bins, first_level):
    bins = int(bins)
    if not 1 <= bins <= 16:
        raise ValueError('bins must be in 1 .. 16')
    levels, names = locus_level_tables(batch.cn_classes, bins, first_level)
    M = np.asarray(batch.cn_classes).shape[2]
    fi = names.index(locus_feature_name(feature, M))
    oi = fi if other is None else names.index(locus_feature_name(other, M))
    return bins, levels, fi, oi


def batch_locus_joint(batch, r0, nr, pairs, seg_fwd_remap, seg_is_original, is_telomere, feature=('total', 1), other=None, bins=8, first_level=0):
    """The exact joint posterior of `feature` at the first and `other` at the second locus of every pair, for restarts r0 ..
    r0+nr-1 of a RemixtBatch from one device call (rmx_locus_joint).  pairs: (first, second) experiment segment indices in
    any order; a pair whose first locus is the right one is asked left to right with the tables exchanged and comes back
    transposed, so that axis -2 is always the pair's first locus.  other None: the same feature.  A pair in two chains is the
    outer product of the two marginals, which (a, a) and (t, t) queries of the same call give: chains are independent under the
    structured posterior, and the mutual information of such a pair is 0.  A dict of `log_joint` (nr, P, bins, bins), the
    arrays of joint_summary, `bins` and `first_level`."""
    bins, levels, fi, oi = _locus_tables(batch, feature, other, bins, first_level)
    cs, ce = chains_from_telomeres(is_telomere)
    segs, swapped, cross = locus_queries(pairs, seg_fwd_remap, cs, ce)
    P = len(segs)
    same = np.flatnonzero(~cross)
    far = np.flatnonzero(cross)
    q = np.zeros((len(same) + 2 * len(far), 4), dtype=np.int32)
    # one chain: left, right, the left locus's table, the right locus's
    q[:len(same), :2] = segs[same]
    q[:len(same), 2] = np.where(swapped[same], oi, fi)
    q[:len(same), 3] = np.where(swapped[same], fi, oi)
    # two chains: the first locus alone, then the second
    first = np.where(swapped[far], segs[far, 1], segs[far, 0])
    second = np.where(swapped[far], segs[far, 0], segs[far, 1])
    q[len(same):len(same) + len(far)] = np.stack([first, first, np.full(len(far), fi), np.full(len(far), fi)], axis=1)
    q[len(same) + len(far):] = np.stack([second, second, np.full(len(far), oi), np.full(len(far), oi)], axis=1)
    lj = np.zeros((nr, P, bins, bins))
    if P:
        raw = batch.locus_joint_raw(r0, nr, q, levels, bins, bins, 0)
        t = raw[:, :len(same)]
        lj[:, same] = np.where(swapped[same][None, :, None, None], np.swapaxes(t, -1, -2), t)
        diag = np.arange(bins)
        ma = raw[:, len(same):len(same) + len(far)][..., diag, diag]
        mb = raw[:, len(same) + len(far):][..., diag, diag]
        with np.errstate(invalid='ignore'):
            lj[:, far] = ma[..., :, None] + mb[..., None, :]
    out = {'log_joint': lj, 'bins': bins, 'first_level': int(first_level)}
    out.update(joint_summary(lj, first_level))
    return out


def locus_windows(anchors, window, seg_fwd_remap, chain_start, chain_end):
    """The neighbourhoods of batch_locus_dependence: segment int (A, 2 window + 1), the experiment segments window .. 1 to the
    left of every anchor, the anchor, and 1 .. window to its right, -1 outside the anchor's chain."""
    an = np.asarray(anchors, dtype=np.int64).reshape(-1)
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    window = int(window)
    if window < 0:
        raise ValueError('window must not be negative')
    if len(an) and (an.min() < 0 or an.max() >= len(fwd)):
        raise ValueError('an anchor needs 0 <= segment < number of segments')
    ce = np.asarray(chain_end, dtype=np.int64)
    seg = an[:, None] + np.arange(-window, window + 1)[None, :]
    inside = (seg >= 0) & (seg < len(fwd))
    chain = np.searchsorted(ce, fwd[np.clip(seg, 0, len(fwd) - 1)], side='left')
    inside &= chain == chain[:, window:window + 1]
    return np.where(inside, seg, -1)


def batch_locus_dependence(batch, r0, nr, anchors, seg_fwd_remap, seg_is_original, is_telomere, window=32, feature=('total', 1), other=None, bins=8,
                           first_level=0):
    """The dependence profile of anchors: for every anchor (an experiment segment) and each of the `window` experiment segments
    on either side inside its chain, joint_summary's mutual_information, correlation and p_equal of `feature` at the anchor
    and `other` at the neighbour.  A dict of `segment` (A, 2 window + 1), experiment indices with -1 outside the chain, the
    three arrays (nr, A, 2 window + 1), NaN there, `bins` and `first_level`.  The left half and the anchor itself come from one
    profile query per anchor (rmx_locus_joint with nslot >= 1: the walk from the anchor leftwards emits the table at every
    step), from which the slots of zero-length segments inserted at shared boundaries are dropped through seg_is_original;
    the right half from one pair query per neighbour."""
    bins, levels, fi, oi = _locus_tables(batch, feature, other, bins, first_level)
    cs, ce = chains_from_telomeres(is_telomere)
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    orig = np.asarray(seg_is_original) != 0
    segment = locus_windows(anchors, window, fwd, cs, ce)
    A, W = segment.shape[0], int(window)
    out = {'segment': segment, 'bins': bins, 'first_level': int(first_level)}
    res = dict((k, np.full((nr, A, 2 * W + 1), np.nan)) for k in DEPENDENCE_ARRAYS)
    if A:
        T = fwd[segment[:, W]]
        leftmost = np.where(segment[:, :W + 1] >= 0, segment[:, :W + 1], np.iinfo(np.int64).max).min(axis=1)
        L = fwd[leftmost]
        nslot = int((T - L).max()) + 1
        if nslot > _LOCUS_MAX_SLOTS:
            raise ValueError('the left half of a window spans more than %d model segments' % _LOCUS_MAX_SLOTS)
        step = max(1, _LOCUS_HOST_BYTES // (max(nr, 1) * nslot * bins * bins * 8))
        for a0 in range(0, A, step):
            sl = slice(a0, min(a0 + step, A))
            n = sl.stop - sl.start
            # the anchor is the walk's start t: its table is the column one, the neighbour's the row one
            q = np.stack([L[sl], T[sl], np.full(n, oi), np.full(n, fi)], axis=1).astype(np.int32)
            prof = batch.locus_joint_raw(r0, nr, q, levels, bins, bins, nslot)                      # (nr, n, nslot, bins, bins)
            tables = np.full((nr, n, 2 * W + 1, bins, bins), np.nan)
            for i in range(n):
                # slot k is model segment T - k: the real ones, in order, are the anchor and its neighbours leftwards
                ks = np.flatnonzero(orig[T[a0 + i] - np.arange(T[a0 + i] - L[a0 + i] + 1)])
                tables[:, i, W - np.arange(len(ks))] = np.swapaxes(prof[:, i, ks], -1, -2)
            right = [(i, k) for i in range(n) for k in range(W + 1, 2 * W + 1) if segment[a0 + i, k] >= 0]
            if right:
                q = np.array([[T[a0 + i], fwd[segment[a0 + i, k]], fi, oi] for i, k in right], dtype=np.int32)
                pair = batch.locus_joint_raw(r0, nr, q, levels, bins, bins, 0)
                ii, kk = np.array(right).T
                tables[:, ii, kk] = pair
            with np.errstate(invalid='ignore'):
                s = joint_summary(tables, first_level)
            for k in DEPENDENCE_ARRAYS:
                res[k][:, sl] = s[k]
    out.update(res)
    return out


# ---- posterior of regular path events: automaton queries over regions (rmx_region_automaton) ---------------
# delta int (Q, A): delta[q, x] the state after reading symbol x in state q; start the start state; alphabet = A; value an int
# per state (the count the state stands for, say) or None.  THE DEVICE READS A REGION FROM ITS LAST SEGMENT TO ITS FIRST: the
# builders below are symmetric under reversal, reverse_automaton turns a left-to-right automaton into one for that order.
Automaton = collections.namedtuple('Automaton', 'delta start alphabet value')
_AUTOMATON_MAX = 16


def _event_table(cn_classes, event):
    """A boolean (C, S) table: a mask name of MASK_NAMES, or the table itself."""
    cn = np.asarray(cn_classes)
    if isinstance(event, str):
        if event not in MASK_NAMES:
            raise ValueError('unknown event %r: one of %s, or a boolean (classes, states) table' % (event, ', '.join(MASK_NAMES)))
        return event_tables(cn)[0][:, MASK_NAMES.index(event)] != 0
    tab = np.asarray(event)
    if tab.shape != cn.shape[:2]:
        raise ValueError('an event table must have shape (num_classes, num_cn_states)')
    return tab != 0


def symbols_from(cn_classes, parts):
    """A symbol table int16 (C, S) from at most 15 parts, each a mask name of MASK_NAMES or a boolean (classes, states)
    table: the symbol of a state is 1 + the index of the first part that holds there, 0 if none holds."""
    parts = list(parts)
    if len(parts) > _AUTOMATON_MAX - 1:
        raise ValueError('at most %d parts' % (_AUTOMATON_MAX - 1))
    cn = np.asarray(cn_classes)
    sym = np.zeros(cn.shape[:2], dtype=np.int16)
    for i in reversed(range(len(parts))):
        sym[_event_table(cn, parts[i])] = i + 1
    return sym


def level_mask(cn_classes, quantity, clone, lo, hi):
    """A boolean (C, S) table: lo <= quantity <= hi, quantity 'total', 'major' or 'minor' of tumour clone 1 .. M-1, or with
    clone 'any' the highest over the tumour clones."""
    q = _level_quantity(cn_classes, quantity)
    M = np.asarray(cn_classes).shape[2]
    if clone != 'any' and not (isinstance(clone, (int, np.integer)) and 1 <= clone < M):
        raise ValueError('clone must be a tumour clone 1 .. %d or \'any\'' % (M - 1))
    v = q.max(axis=-1) if clone == 'any' else q[:, :, clone - 1]
    return (v >= lo) & (v <= hi)


def automaton_runs(bins):
    """The number of maximal runs of symbol 1 among the read segments (alphabet 2).  State 2 c + e: c runs so far, saturating
    at bins - 1 (the last count means bins - 1 or more), e whether the last read segment was in the event.  Q = 2 bins,
    bins <= 8; value is c."""
    bins = int(bins)
    if not 1 <= bins <= 8:
        raise ValueError('bins must be in 1 .. 8')
    delta = np.zeros((2 * bins, 2), dtype=np.uint8)
    for c in range(bins):
        for e in (0, 1):
            delta[2 * c + e, 0] = 2 * c
            delta[2 * c + e, 1] = 2 * c + 1 if e else 2 * min(c + 1, bins - 1) + 1
    return Automaton(delta, 0, 2, tuple(c for c in range(bins) for _ in (0, 1)))


def automaton_run_of(k):
    """Whether some run of symbol 1 spans at least k read segments (alphabet 2).  The state is the length of the current run,
    state k absorbing: P(state k) is the answer.  Q = k + 1, 1 <= k <= 15; value is the state itself."""
    k = int(k)
    if not 1 <= k <= 15:
        raise ValueError('k must be in 1 .. 15')
    delta = np.zeros((k + 1, 2), dtype=np.uint8)
    for q in range(k + 1):
        delta[q, 0] = k if q == k else 0
        delta[q, 1] = min(q + 1, k)
    return Automaton(delta, 0, 2, tuple(range(k + 1)))


def automaton_switches(bins):
    """The number of switches between two levels (alphabet 3: symbols 1 and 2 are the levels, symbol 0 is ignored).  State 0:
    neither level read yet; state 1 + 2 c + (v - 1): c switches so far, saturating at bins - 1, the level read last v.
    Q = 1 + 2 bins, bins <= 7; value is c."""
    bins = int(bins)
    if not 1 <= bins <= 7:
        raise ValueError('bins must be in 1 .. 7')
    delta = np.zeros((1 + 2 * bins, 3), dtype=np.uint8)
    delta[0] = (0, 1, 2)
    for c in range(bins):
        for v in (1, 2):
            q = 1 + 2 * c + (v - 1)
            delta[q, 0] = q
            delta[q, v] = q
            delta[q, 3 - v] = 1 + 2 * min(c + 1, bins - 1) + (2 - v)
    return Automaton(delta, 0, 3, (0,) + tuple(c for c in range(bins) for _ in (0, 1)))


def _check_automaton(automaton):
    delta = np.asarray(automaton.delta)
    if delta.ndim != 2 or not (1 <= delta.shape[0] <= _AUTOMATON_MAX and 1 <= delta.shape[1] <= _AUTOMATON_MAX):
        raise ValueError('delta must have shape (Q, A) with Q and A in 1 .. %d' % _AUTOMATON_MAX)
    Q = delta.shape[0]
    if delta.min() < 0 or delta.max() >= Q or not 0 <= int(automaton.start) < Q:
        raise ValueError('delta and start must hold states in [0, Q)')
    return delta.astype(np.uint8), int(automaton.start)


def reverse_automaton(delta, start, accept):
    """For users who think left to right: a deterministic automaton (delta (Q, A), start, accept: the accepting states, as
    indices or a boolean (Q,)) that reads a region first segment to last -> (Automaton, accept' boolean) that accepts the
    same regions read last segment to first, by the subset construction of the reversed language: a state is the set of
    original states from which the symbols read so far lead to acceptance.  ValueError above 16 states."""
    delta = np.asarray(delta, dtype=np.int64)
    Q, A = delta.shape
    acc = np.zeros(Q, dtype=bool)
    acc[np.asarray(accept)] = True
    first = frozenset(np.flatnonzero(acc).tolist())
    index, rows, todo = {first: 0}, [], [first]
    while todo:
        cur = todo.pop(0)
        row = []
        for x in range(A):
            nxt = frozenset(q for q in range(Q) if int(delta[q, x]) in cur)
            if nxt not in index:
                if len(index) >= _AUTOMATON_MAX:
                    raise ValueError('the reversed automaton has more than %d states' % _AUTOMATON_MAX)
                index[nxt] = len(index)
                todo.append(nxt)
            row.append(index[nxt])
        rows.append(row)
    sets = sorted(index, key=index.get)
    return (Automaton(np.array(rows, dtype=np.uint8), 0, A, None), np.array([int(start) in s for s in sets], dtype=bool))


def _one_chain_queries(regions, seg_fwd_remap, seg_is_original, is_telomere, what):
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    R = len(np.asarray(regions).reshape(-1, 2))
    split = np.flatnonzero(np.bincount(piece_region, minlength=R) > 1)
    if len(split):
        reg = np.asarray(regions).reshape(-1, 2)[split[0]]
        raise ValueError('%s: region %d (%d, %d) lies in two chains: the automaton\'s state does not cross a chain end' % (what, split[0], reg[0], reg[1]))
    return runs, constrain, R


def batch_region_automaton(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, automaton, symbols, accept=None):
    """The exact distribution of the final state of `automaton` (an Automaton) over regions, for restarts r0 .. r0+nr-1 of a
    RemixtBatch from one device call (rmx_region_automaton).  regions: (first, last) experiment segment indices, each inside
    one chain (ValueError otherwise).  symbols: an int (classes, states) table with entries in [0, alphabet), as symbols_from
    gives.  The automaton reads a region FROM ITS LAST SEGMENT TO ITS FIRST; zero-length segments inserted at shared
    boundaries are not read.  A dict of `log_final` and `final` (nr, R, Q), and with accept (state indices or a boolean (Q,))
    `p_accept` (nr, R)."""
    delta, start = _check_automaton(automaton)
    sym = np.asarray(symbols)
    if sym.shape != np.asarray(batch.cn_classes).shape[:2]:
        raise ValueError('symbols must have shape (num_classes, num_cn_states)')
    runs, constrain, R = _one_chain_queries(regions, seg_fwd_remap, seg_is_original, is_telomere, 'region_automaton')
    Q = delta.shape[0]
    lf = np.zeros((nr, R, Q))
    if R:
        q = np.zeros((R, 4), dtype=np.int32)
        q[:, :2] = runs
        lf = batch.region_automaton_raw(r0, nr, q, sym[:, None, :], delta[None], np.array([start]), constrain)
    with np.errstate(over='ignore'):
        out = {'log_final': lf, 'final': np.exp(lf)}
    if accept is not None:
        acc = np.zeros(Q, dtype=bool)
        acc[np.asarray(accept)] = True
        out['p_accept'] = np.clip(out['final'][..., acc].sum(axis=-1), 0., 1.)
    return out


def _piece_final(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, automaton, event):
    """(final (nr, P, Q) probabilities of every region piece, piece_region, R): one query per piece of a region split at chain ends."""
    delta, start = _check_automaton(automaton)
    sym = symbols_from(batch.cn_classes, [event])
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, constrain = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    P, R = len(runs), len(np.asarray(regions).reshape(-1, 2))
    if P == 0:
        return np.zeros((nr, 0, delta.shape[0])), piece_region, R
    q = np.zeros((P, 4), dtype=np.int32)
    q[:, :2] = runs
    with np.errstate(over='ignore'):
        return np.exp(batch.region_automaton_raw(r0, nr, q, sym[:, None, :], delta[None], np.array([start]), constrain)), piece_region, R


def batch_event_runs(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, event, bins=8):
    """How many separate events a region holds: the distribution of the number of maximal runs of real segments in `event` (a
    mask name of MASK_NAMES or a boolean (classes, states) table), for restarts r0 .. r0+nr-1 of a RemixtBatch from one
    device call.  A dict of `num_events` (nr, R, bins) -- entry k the probability of exactly k runs, the last that of
    bins - 1 or more -- and `p_any` (nr, R), the probability of at least one.  A run cannot cross a chromosome end, so the
    pieces of a region split at chain ends are asked one by one and their counts add (combine_counts); zero-length segments
    inserted at shared boundaries neither start, extend nor end a run."""
    au = automaton_runs(bins)
    bins = len(au.value) // 2
    final, piece_region, R = _piece_final(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, au, event)
    pmf = final.reshape(final.shape[:2] + (bins, 2)).sum(axis=-1)
    with np.errstate(divide='ignore'):
        counts = np.clip(combine_counts(np.log(pmf), piece_region, R), 0., 1.)
    return {'num_events': counts, 'p_any': np.clip(1. - counts[..., 0], 0., 1.)}


def batch_event_run_of(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, event, k):
    """Whether `event` (as batch_event_runs) is supported by at least k consecutive real segments somewhere in a region: a dict
    of `p_run` (nr, R).  Pieces of a region split at chain ends are joined as 1 - prod (1 - p): chains are independent and a
    run cannot cross a chromosome end."""
    au = automaton_run_of(k)
    final, piece_region, R = _piece_final(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, au, event)
    miss = np.ones((nr, R))
    for j, reg in enumerate(np.asarray(piece_region)):
        miss[:, reg] *= np.clip(1. - final[:, j, -1], 0., 1.)
    return {'p_run': 1. - miss}


# ---- entropy of the path posterior over regions (rmx_path_entropy) ---------------------------------------------
PATH_ENTROPY_ARRAYS = ('path_entropy', 'inserted_slack', 'marginal_entropy_sum', 'total_correlation', 'perplexity', 'entropy_per_segment')


def _prefix(a):
    """Prefix sums along the last axis with a leading zero: sum a[..., i:j] = p[..., j] - p[..., i]."""
    a = np.asarray(a, dtype=float)
    return np.concatenate([np.zeros(a.shape[:-1] + (1,)), np.cumsum(a, axis=-1)], axis=-1)


def entropy_runs(marginal, step, runs, seg_is_original):
    """The entropy (nats) of the path posterior over runs of model segments from the two arrays of path_entropy_raw
    (marginal, step: (..., N1); marginal[n] = H(post_n), step[n] = H(c_n | c_n+1)).  runs int (P, 2): segments a <= b of one
    chain each, b a real segment.  A dict of arrays (..., P):
      path_entropy          H(c_a .. c_b) = marginal[b] + sum step[a .. b-1]: the chain is Markov, so the chain rule stops after
                            one condition.  The path is over the model run, inserted zero-length segments included
      marginal_entropy_sum  sum marginal[a .. b]
      inserted_slack        sum of step[m] over the inserted segments m of the run.  H(real segments of the run) lies in
                            [path_entropy - inserted_slack, path_entropy]: H(c_I | c_R) = sum_m H(c_m | c_{I > m}, c_R) over
                            the inserted m in descending order, and every term is <= H(c_m | c_m+1) because c_m+1 is among its
                            conditions and dropping conditions raises an entropy
    and `num_segments` int (P,), the real segments of each run.  Everything is a difference of prefix sums."""
    marg, st = np.asarray(marginal, dtype=float), np.asarray(step, dtype=float)
    r = np.asarray(runs, dtype=np.int64).reshape(-1, 2)
    real = np.asarray(seg_is_original) != 0
    a, b = r[:, 0], r[:, 1]
    if len(r) and (a.min() < 0 or b.max() >= marg.shape[-1] or (a > b).any()):
        raise ValueError('a run needs 0 <= first <= last < number of model segments')
    ps, pm, pi = _prefix(st), _prefix(marg), _prefix(np.where(real, 0., st))
    nreal = np.concatenate([[0], np.cumsum(real)]).astype(np.int64)
    return {'path_entropy': marg[..., b] + (ps[..., b] - ps[..., a]),
            'marginal_entropy_sum': pm[..., b + 1] - pm[..., a],
            'inserted_slack': pi[..., b] - pi[..., a],
            'num_segments': nreal[b + 1] - nreal[a]}


def batch_path_entropy(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere):
    """How uncertain regions are, for restarts r0 .. r0+nr-1 of a RemixtBatch from one device call over all segments
    (path_entropy_raw); everything else is prefix sums here.  regions: (first, last) experiment segment indices; None: one
    region, the genome.  A dict of arrays with a leading restart axis, nats:
      segment_entropy (nr, N)      H of every experiment segment's marginal
      step_entropy (nr, N - 1)     the model steps from seg_fwd_remap[i] up to but not including seg_fwd_remap[i + 1] added up:
                                   the entropy of segment i and the inserted segments behind it given segment i + 1; NaN where
                                   no reference adjacency joins i and i + 1
      adjacent_information (nr, N - 1)  I(c_i; c_i+1) = H(c_i) - H(c_i | c_i+1) where no inserted segment separates the two; NaN
                                   otherwise, and where no reference adjacency joins them
    and per region, (nr, R): path_entropy (pieces in different chains add: chains are independent), inserted_slack,
    marginal_entropy_sum, total_correlation = marginal_entropy_sum - path_entropy, perplexity = exp(path_entropy) and
    entropy_per_segment = path_entropy over the number of real segments (entropy_runs)."""
    fwd = np.asarray(seg_fwd_remap, dtype=np.int64)
    N = len(fwd)
    marg, step = batch.path_entropy_raw(r0, nr)
    marg, step = np.asarray(marg, dtype=float), np.asarray(step, dtype=float)
    out = {'segment_entropy': marg[:, fwd]}
    ps = _prefix(step)
    _, joined = adjacency_regions(fwd, is_telomere)
    se = np.full((nr, max(N - 1, 0)), np.nan)
    ai = np.full((nr, max(N - 1, 0)), np.nan)
    if len(joined):
        se[:, joined] = ps[:, fwd[joined + 1]] - ps[:, fwd[joined]]
        direct = joined[fwd[joined + 1] == fwd[joined] + 1]
        ai[:, direct] = marg[:, fwd[direct]] - step[:, fwd[direct]]
    out['step_entropy'], out['adjacent_information'] = se, ai
    reg = genome_region(np.zeros((0, 2), dtype=np.int64), N) if regions is None else np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    R = len(reg)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, _ = region_queries(reg, fwd, seg_is_original, cs, ce)
    pieces = entropy_runs(marg, step, runs, seg_is_original)
    for k in ('path_entropy', 'inserted_slack', 'marginal_entropy_sum'):
        out[k] = combine(pieces[k], piece_region, R)
    nreal = np.zeros(R)
    np.add.at(nreal, np.asarray(piece_region), pieces['num_segments'])
    out['total_correlation'] = out['marginal_entropy_sum'] - out['path_entropy']
    with np.errstate(over='ignore'):                       # (a genome's perplexity is beyond the doubles: inf)
        out['perplexity'] = np.exp(out['path_entropy'])
    with np.errstate(invalid='ignore', divide='ignore'):
        out['entropy_per_segment'] = out['path_entropy'] / nreal
    return out


# ---- posterior of length-weighted event occupancy over regions (rmx_region_sums) -------------------------------
# how much of a region is in an event: the distribution of sum_n w_n level(c_n) over the region's segments, with non-negative
# integer weights w_n and levels.  EXACT for integer weights (weights='segments', or lengths that are multiples of the unit); for
# real lengths the floor and the ceil weights give two distributions that BRACKET the true one, rigorously: for every path,
# unit * (floor sum) <= true weighted sum <= unit * (ceil sum).  The bracket is as wide as the number of real segments whose
# length is no multiple of the unit: an arm-sized region of thousands of unequal segments gets a loose bracket.
SUMS_MAX_BINS = 64
OCCUPANCY_WEIGHTS = ('length', 'segments')


def sums_max_bins(num_states):
    """The most bins rmx_region_sums takes at num_states copy-number states (rmxh::sums_max_bins, from the kernel's LDS plan):
    64 up to 304 states, 32 up to 608, 16 up to 1024, 0 beyond."""
    S = int(num_states)
    if S < 1 or S > 1024:
        return 0
    SR = (S + 15) // 16 * 16
    for bins in (64, 32, 16):
        if SR * (128 * {64: 4, 32: 2, 16: 1}[bins] + 12) + 64 <= 160 * 1024:
            return bins
    return 0


def _integer_weights(lengths, unit):
    """(floor(l / unit), ceil(l / unit)) as int64.  A ratio within a few ulps of an integer is that integer (1000 / (2500 / 45)
    is 18): unit * floor <= l <= unit * ceil then holds up to the rounding of the product."""
    ratio = lengths / unit
    near = np.round(ratio)
    whole = np.abs(ratio - near) <= 8 * np.finfo(float).eps * np.maximum(near, 1.)
    wf, wc = np.where(whole, near, np.floor(ratio)), np.where(whole, near, np.ceil(ratio))
    return wf.astype(np.int64), wc.astype(np.int64)


def quantise_lengths(lengths, bins, vmax=1, unit=None):
    """Integer weights for real segment lengths: (unit, w_floor, w_ceil, exact) with w_floor = floor(l / unit) and
    w_ceil = ceil(l / unit), int64.  For every choice of levels in 0 .. vmax, unit * sum w_floor level <= sum l level <=
    unit * sum w_ceil level: the two integer sums bracket the true one.  unit None: the smallest unit for which
    sum ceil(l_n / unit) * vmax <= bins - 1, so that nothing saturates; if even one unit per segment of positive length does
    not fit, the smallest unit for which the FLOOR sum fits (the ceil side then saturates, and its last bin says so).
    exact: the two weight vectors are equal -- every length is a multiple of the unit, and the distribution is exact."""
    l = np.asarray(lengths, dtype=float).reshape(-1)
    bins, vmax = int(bins), max(int(vmax), 1)
    if bins < 1:
        raise ValueError('bins must be at least 1')
    if len(l) and not (np.isfinite(l).all() and l.min() >= 0):
        raise ValueError('lengths must be finite and >= 0')
    cap = (bins - 1) // vmax                   # the most weight units a region may hold
    if unit is not None:
        unit = float(unit)
        if not unit > 0:
            raise ValueError('unit must be positive')
    elif not (l > 0).any():
        unit = 1.
    else:
        pos = l[l > 0]
        ceil_fits = len(pos) <= cap

        def fits(u):
            wf, wc = _integer_weights(pos, u)
            return (wc if ceil_fits else wf).sum() <= cap
        # the sums only change at u = l_n / k, so the smallest unit that fits is one of those.  (The floor sum fits only PAST such
        # a point, where no smallest unit exists: a part in 1e12 above it.)  The largest candidate fits: every ceil is 1 there,
        # every floor 0
        cand = np.unique((pos[:, None] / np.arange(1, max(cap, 1) + 2)[None, :]).reshape(-1))
        if not ceil_fits:
            cand = cand * (1 + 1e-12)
        lo, hi = 0, len(cand) - 1
        while lo < hi:
            mid = (lo + hi) // 2
            if fits(cand[mid]):
                hi = mid
            else:
                lo = mid + 1
        unit = float(cand[lo])
    wf, wc = _integer_weights(l, unit)
    return unit, wf, wc, bool(np.array_equal(wf, wc))


def _sum_levels(cn_classes, event):
    """An int (C, S) level table: a mask name of MASK_NAMES or a boolean (classes, states) table (level 1 where the event holds),
    or a (quantity, clone) feature as locus_joint takes it (the level is that copy number)."""
    cn = np.asarray(cn_classes)
    if isinstance(event, tuple) and len(event) == 2 and isinstance(event[0], str):
        quantity, clone = event
        q = _level_quantity(cn, quantity)
        M = cn.shape[2]
        if clone != 'any' and not (isinstance(clone, (int, np.integer)) and 1 <= clone < M):
            raise ValueError('clone must be a tumour clone 1 .. %d or \'any\'' % (M - 1))
        return (q.max(axis=-1) if clone == 'any' else q[:, :, clone - 1]).astype(np.int64)
    return _event_table(cn, event).astype(np.int64)


def _check_levels(batch, levels):
    lv = np.asarray(levels)
    if lv.shape != np.asarray(batch.cn_classes).shape[:2]:
        raise ValueError('levels must have shape (num_classes, num_cn_states)')
    if lv.size and (lv.min() < 0 or lv.max() > 32767):
        raise ValueError('levels must lie in 0 .. 32767')
    return lv.astype(np.int16)


def _sum_bins(batch, bins):
    most = sums_max_bins(batch.num_cn_states)
    bins = most if bins is None else int(bins)
    if not 1 <= bins <= SUMS_MAX_BINS:
        raise ValueError('bins must be in 1 .. %d' % SUMS_MAX_BINS)
    if bins > most:
        raise ValueError('at %d states a region sum holds at most %d bins' % (batch.num_cn_states, most))
    return bins


def _piece_sums(batch, r0, nr, runs, piece_region, R, levels, piece_weights, bins):
    """One device call for several weightings of the same pieces: piece_weights a list over weightings of lists over pieces of
    int weight vectors (one entry per model segment of the piece) -> a list over weightings of probabilities (nr, R, bins),
    the pieces of a region convolved (combine_counts)."""
    P = len(runs)
    if P == 0:
        empty = np.zeros((nr, R, bins))
        empty[..., 0] = 1.
        return [empty.copy() for _ in piece_weights]
    pool = np.concatenate([np.asarray(w, dtype=np.int64) for ws in piece_weights for w in ws])
    if pool.min() < 0 or pool.max() >= 2 ** 31:
        raise ValueError('weights must lie in 0 .. 2^31 - 1')
    q = np.zeros((len(piece_weights) * P, 4), dtype=np.int32)
    at = 0
    for k, ws in enumerate(piece_weights):
        for j, w in enumerate(ws):
            if len(w) != runs[j][1] - runs[j][0] + 1:
                raise ValueError('a piece needs one weight per model segment')
            q[k * P + j] = (runs[j][0], runs[j][1], 0, at)
            at += len(w)
    logp = batch.region_sums_raw(r0, nr, q, levels[:, None, :], pool.astype(np.int32), bins)
    return [np.clip(combine_counts(logp[:, k * P:(k + 1) * P], piece_region, R), 0., 1.) for k in range(len(piece_weights))]


def batch_region_sums(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, levels, weights, bins=None):
    """The exact posterior distribution of sum_n weights[n] levels(c_n) over the model segments of regions, for restarts r0 ..
    r0+nr-1 of a RemixtBatch from one device call (rmx_region_sums).  regions: (first, last) experiment segment indices;
    levels: an int (classes, states) table, every entry >= 0; weights: int (num model segments,), every entry >= 0, PER MODEL
    SEGMENT (0: the segment does not count -- give the inserted zero-length segments 0); bins None: the most the batch's state
    count allows (sums_max_bins).  Exact for these integer weights.  Pieces of a region in several chains are joined with
    combine_counts: chains are independent, sums add, and the last bin absorbs.  A dict of `bins`, `pmf` (nr, R, bins) --
    entry k the probability that the sum is k, the last entry that of bins - 1 or more --, `mean` (nr, R) of the sum capped at
    bins - 1, and `p_saturated` (nr, R), the last bin."""
    bins = _sum_bins(batch, bins)
    lv = _check_levels(batch, levels)
    w = np.asarray(weights)
    if w.shape != (batch.num_segments,) or (w.size and w.min() < 0) or not np.issubdtype(w.dtype, np.integer):
        raise ValueError('weights must be non-negative integers, one per model segment')
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, _ = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    R = len(np.asarray(regions).reshape(-1, 2))
    pmf, = _piece_sums(batch, r0, nr, runs, piece_region, R, lv, [[w[a:b + 1] for a, b in runs]], bins)
    return {'bins': bins, 'pmf': pmf, 'mean': (pmf * np.arange(bins)).sum(axis=-1), 'p_saturated': pmf[..., -1]}


def batch_event_occupancy(batch, r0, nr, regions, seg_fwd_remap, seg_is_original, is_telomere, l1, event, weights='length', bins=None, unit=None):
    """How much of a region is in an event: the posterior distribution of the weighted occupancy sum_n w_n level(c_n) over the
    real segments of regions, for restarts r0 .. r0+nr-1 of a RemixtBatch from ONE device call that holds both the floor and
    the ceil queries (rmx_region_sums).  regions: (first, last) experiment segment indices; l1: the model segments' lengths.
    event: a mask name of MASK_NAMES or a boolean (classes, states) table (level_mask) -- level 1 where the event holds --, or a
    (quantity, clone) feature as locus_joint takes it (the level is that copy number: 'the segments carry at least twelve
    copies between them').  weights 'segments': every real segment weighs 1, and the result is EXACT.  weights 'length': a
    real segment weighs its length in units of `unit` (None: per region, quantise_lengths' choice for `bins` and the
    table's highest level); the result is exact where every length of the region is a multiple of the unit (`exact`), and
    otherwise a RIGOROUS BRACKET: for every path unit * (floor sum) <= true weighted sum <= unit * (ceil sum), so pmf_floor
    and pmf_ceil are the distributions of a lower and of an upper bound of the true sum, not approximations of its
    distribution.  The bracket is as wide as the number of real segments whose length is no multiple of the unit: arm-sized
    regions of thousands of unequal segments get a loose bracket.  Inserted zero-length segments weigh 0.  bins None: the
    most the batch's state count allows (sums_max_bins).  A dict of
      bins; unit (R,); length (R,), the summed length of the region's real segments (their number under 'segments'); exact (R,)
      pmf_floor, pmf_ceil (nr, R, bins)   entry k: P(the integer sum is k), the last entry that of bins - 1 or more
      mean_floor, mean_ceil (nr, R)       unit * the mean of the integer sums: a lower and an upper bound of the mean weighted
                                          occupancy.  The floor sum capped at bins - 1 is still a lower bound; where the ceil
                                          sum can pass the last bin and that bin has mass, its mean bounds nothing: mean_ceil
                                          is inf there
      p_saturated (nr, R)                 the last bin of pmf_ceil: the mass whose ceil sum is not resolved.
    occupancy_at_least turns it into bounds of P(weighted fraction >= f)."""
    if weights not in OCCUPANCY_WEIGHTS:
        raise ValueError('weights must be one of %s' % ', '.join(OCCUPANCY_WEIGHTS))
    bins = _sum_bins(batch, bins)
    lv = _check_levels(batch, _sum_levels(batch.cn_classes, event))
    vmax = int(lv.max()) if lv.size else 1
    real = np.asarray(seg_is_original) != 0
    seg_len = np.where(real, np.asarray(l1, dtype=float), 0.) if weights == 'length' else real.astype(float)
    cs, ce = chains_from_telomeres(is_telomere)
    runs, piece_region, _ = region_queries(regions, seg_fwd_remap, seg_is_original, cs, ce)
    R = len(np.asarray(regions).reshape(-1, 2))
    units, length, exact, capped = np.ones(R), np.zeros(R), np.ones(R, dtype=bool), np.zeros(R, dtype=bool)
    wfloor, wceil = [None] * len(runs), [None] * len(runs)
    for reg in range(R):
        pieces = np.flatnonzero(np.asarray(piece_region) == reg)
        ls = [seg_len[runs[j][0]:runs[j][1] + 1] for j in pieces]
        whole = np.concatenate(ls) if ls else np.zeros(0)
        length[reg] = whole.sum()
        u, wf, wc, ex = quantise_lengths(whole, bins, vmax, 1. if weights == 'segments' else unit)
        units[reg], exact[reg] = u, ex
        capped[reg] = int(wc.sum()) * vmax > bins - 1          # the ceil sum can pass the last bin
        at = 0
        for j, x in zip(pieces, ls):
            wfloor[j], wceil[j] = wf[at:at + len(x)], wc[at:at + len(x)]
            at += len(x)
    lo, hi = _piece_sums(batch, r0, nr, runs, piece_region, R, lv, [wfloor, wceil], bins)
    k = np.arange(bins)
    mean_ceil = np.where(capped[None, :] & (hi[..., -1] > 0), np.inf, (hi * k).sum(axis=-1) * units)
    return {'bins': bins, 'unit': units, 'length': length, 'exact': exact, 'pmf_floor': lo, 'pmf_ceil': hi,
            'mean_floor': (lo * k).sum(axis=-1) * units, 'mean_ceil': mean_ceil, 'p_saturated': hi[..., -1]}


def occupancy_at_least(out, fraction):
    """(lower, upper), each (..., R): bounds of P(the weighted occupancy is at least `fraction` of the region's length) from a
    batch_event_occupancy dict (for a 0/1 event: 'at least half of the arm is in LOH').  With the threshold
    t = ceil(fraction * length / unit) in integer units, lower = P(floor sum >= t) and upper = P(ceil sum >= t): the floor sum
    is an integer below the true sum in units and the ceil sum one above it (a ratio within a few ulps of an integer counts as
    that integer, as in quantise_lengths).  The two coincide where `exact`.  A threshold past
    the last bin is not resolved: lower is 0 there and upper the last bin of pmf_ceil."""
    bins = int(out['bins'])
    with np.errstate(invalid='ignore'):
        ratio = float(fraction) * np.asarray(out['length'], dtype=float) / np.asarray(out['unit'], dtype=float)
    near = np.round(ratio)            # (quantise_lengths' rule: a ratio within a few ulps of an integer is that integer, not the next)
    with np.errstate(invalid='ignore'):
        t = np.where(np.abs(ratio - near) <= 8 * np.finfo(float).eps * np.maximum(near, 1.), near, np.ceil(ratio))
    t = np.clip(np.where(np.isfinite(t), t, 0), 0, bins).astype(np.int64)
    k = np.arange(bins)
    tail = k[None, :] >= t[:, None]                                    # (R, bins)
    lower = np.where(tail, np.asarray(out['pmf_floor']), 0.).sum(axis=-1)
    upper = np.where(np.minimum(t, bins - 1)[:, None] <= k[None, :], np.asarray(out['pmf_ceil']), 0.).sum(axis=-1)
    return np.clip(lower, 0., 1.), np.clip(upper, 0., 1.)
