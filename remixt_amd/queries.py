"""The posterior queries of a fit, each described once.

A query is one entry of QUERIES: its name, what it needs of the device batch, a plain function that makes the
posteriors.batch_* call for a range of restarts, and how its result is taken apart and put together along the restart axis.
The four classes that answer queries -- cn_model.BreakpointModel (one restart), restarts.RestartSet (the restarts of one
batch), restarts.RestartGroups (several batches) and restarts.DatasetGroups (several datasets) -- get their methods from
this table through the class decorator `answers`: one generic body per level below, no code per (query, level).

Adding a query: its posteriors.batch_* function, and its entry here, in a later tuple such as AUTOMATON_QUERIES (QUERIES and LATER_QUERIES are closed lists).

(posteriors imports nothing of this package when it loads, and this module imports posteriors alone, so cn_model and
restarts load it at import time without a cycle.  sample_cn, restart_overlap and ploidy_posterior_sd are no entries: the
first seeds per restart, the second spans batches, the third is a statistic of one model.)"""
import collections
import inspect

import numpy as np

from . import posteriors


class Restarts(collections.namedtuple('Restarts', 'batch r0 nr models')):
    """What an entry's function gets first: restarts r0 .. r0+nr-1 of a device batch and their BreakpointModels."""
    __slots__ = ()

    @property
    def model(self):
        return self.models[0]

    @property
    def at(self):
        """The leading arguments of a posteriors.batch_* call."""
        return self.batch, self.r0, self.nr

    @property
    def maps(self):
        """The segment maps, which the restarts of a batch share."""
        m = self.models[0]
        return m.seg_fwd_remap, m.seg_is_original, m.is_telomere


# name: the method's.  needs: the RemixtBatch method without which `lacks` is the NotImplementedError.  call(q, ...): the batch
# call for the Restarts q; the rest of its `def` line is the public signature, and a `cn` there arrives as state indices in model
# segment order, (nr, N1).  cn: None, or how the per-restart parameter `cn` is read -- 'call': paths in experiment order, None =
# the decoded paths; 'path': None stays None, and `lacks_cn` are the words for a path given without a batch.  The result has a
# leading restart axis: a list over restarts, a bare array, or a dict of arrays except the keys in `shared` (the same for all
# restarts), `extend` (lists over restarts) and `each` (lists of arrays with a restart axis).  many: the model level also
# takes K calls, (K, N, M, 2).  finish(out, model, args, restart_axis): the last step at every level but the datasets'.
# flat: the datasets' results are strung together, not listed per dataset.  doc: the model level's help; result: what the
# restart levels return, in words.
Query = collections.namedtuple('Query', 'name needs lacks call doc result cn lacks_cn shared extend each many finish flat')


def _query(needs, lacks, result, cn=None, lacks_cn=None, shared=(), extend=(), each=(), many=False, finish=None, flat=False):
    def entry(call):
        return Query(call.__name__, needs, lacks, call, inspect.cleandoc(call.__doc__), result, cn, lacks_cn, shared, extend, each, many, finish, flat)
    return entry


@_query('posterior_summary_raw', 'has no posterior summary', 'a list of dicts of arrays in experiment segment order', cn='path',
        lacks_cn='posterior summaries', flat=True)
def posterior_summary(q, cn=None, marginals=False):
    """Exact per-segment summaries of the posterior marginals of the last variational update, in experiment segment
    order (as optimal_cn): the arrays of posteriors.unpack -- total_cn_mean / total_cn_sd (N, M), p_subclonal, p_loh,
    p_hdel, expected_alleles_subclonal, cn_posterior_max, cn_posterior_entropy, cn_mpm, and cn_marginals with
    marginals=True.  cn: an already decoded path ([N][M][2], model segment order, e.g. what infer_cn fills); it
    supplies cn_posterior_prob, the marginal probability of its state at every segment."""
    out = posteriors.batch_summaries(*q.at, states=cn, marginals=marginals)
    return [dict((k, v[m.seg_fwd_remap]) for k, v in s.items()) for s, m in zip(out, q.models)]


@_query('region_logprob_raw', 'has no region event probabilities', 'a dict of arrays (restarts, len(regions))')
def region_events(q, regions):
    """Exact probabilities, under the structured posterior of the last variational update, of copy-number events over
    regions: regions is a list of (first, last) experiment segment indices; a dict of arrays (len(regions),):
    p_all_loh, p_any_loh, p_all_hdel, p_any_hdel, p_any_subclonal (over the region's segments), p_no_change (the same
    copy-number state along the whole region) and p_no_total_change (the same per-clone totals).  A region that spans
    chain ends is the conjunction over its chains."""
    return posteriors.batch_region_events(*q.at, regions, *q.maps)


@_query('region_counts_raw', 'has no region change counts', 'a dict of arrays (restarts, len(regions), bins)')
def region_change_counts(q, regions, bins=8):
    """Exact posterior distribution of the number of copy-number changes inside regions ((first, last) experiment
    segment indices): a dict of arrays (len(regions), bins), `num_changes` (changes of the copy-number state) and
    `num_total_changes` (changes of the per-clone totals).  Entry k is the probability of exactly k changes, the
    last entry that of bins - 1 or more.  Changes are counted between consecutive model segments: a path that takes a
    third state in a zero-length segment inserted at a shared boundary changes twice there."""
    return posteriors.batch_region_change_counts(*q.at, regions, *q.maps, bins=bins)


@_query('region_extremes_raw', 'has no region extremes', '`bins`, `first_level` and arrays (restarts, len(regions), ...)',
        shared=('bins', 'first_level'))
def region_cn_extremes(q, regions, quantity='total', clone='any', bins=16, first_level=0):
    """Exact posterior distribution, under the structured posterior of the last variational update, of the highest and of
    the lowest copy number inside regions ((first, last) experiment segment indices): is the region amplified, how high
    does it go, how deep is its deepest loss.  quantity: 'total', 'major' or 'minor'; clone: a tumour clone 1 .. M-1 or
    'any'; the window of copy numbers is first_level .. first_level + bins - 1.  A dict of `bins`, `first_level`, arrays
    (len(regions), bins) `peak_cdf`, `peak_pmf`, `floor_cdf` (P(lowest >= k)) and `floor_pmf`, and int arrays
    (len(regions),) `peak_q05/q50/q95` and `floor_q05/q50/q95` (posteriors.batch_region_cn_extremes;
    posteriors.amplification_prob gives P(peak >= threshold))."""
    return posteriors.batch_region_cn_extremes(*q.at, regions, *q.maps, quantity=quantity, clone=clone, bins=bins, first_level=first_level)


@_query('region_extremes_raw', 'has no region extremes', 'arrays (restarts, len(regions), M - 1, bins)')
def region_clone_extremes(q, regions, bins=16):
    """The distributions of the peak and of the lowest total copy number of every tumour clone over regions, from one
    device call: a dict of `peak_total_pmf` and `floor_total_pmf`, (len(regions), M - 1, bins) each, window 0 .. bins - 1
    (what config cn_region_extremes adds to a fit result)."""
    return posteriors.batch_clone_extremes(*q.at, regions, *q.maps, bins=bins)


@_query('region_moments_raw', 'has no region moments', 'a dict of `length` (len(regions),) and arrays (restarts, len(regions), ...)',
        shared=('length',))
def region_cn_moments(q, regions):
    """Exact posterior mean and covariance, under the structured posterior of the last variational update, of copy
    number over regions ((first, last) experiment segment indices): a dict of `length` (R,), `total_cn_mean` (R, M) and
    `total_cn_cov` (R, M, M) -- the length-weighted mean total copy number of each clone over the region, with the
    covariance matrix that the correlation between neighbouring segments gives it -- and `fraction_mean` (R, 4) and
    `fraction_cov` (R, 4, 4) of the length fractions of posteriors.MOMENT_FRACTIONS.  Zero-length segments inserted at
    shared boundaries have no weight; a region of length 0 gives NaN."""
    return posteriors.batch_region_cn_moments(*q.at, regions, *q.maps, q.model.l1)


@_query('region_extent_raw', 'has no event extents', 'a list over restarts of lists of posteriors.extent_summary dicts, one per anchor')
def event_extent(q, anchors, event, window=64):
    """Where a copy-number event begins and ends around anchor segments, exactly, under the structured posterior of the
    last variational update: anchors are experiment segment indices, event a mask name of posteriors.MASK_NAMES ('loh':
    the LOH run around the anchor), a label name of posteriors.LABEL_NAMES ('state' / 'total': the constant-state /
    constant-total run around it) or a (mask, label) pair, window the number of model segments walked on each side (an
    int or a (left, right) pair).  A list with one posteriors.extent_summary dict per anchor: p_event, the survival
    curves of both ends, the boundary pmfs with their censored mass, and the 5 / 50 / 95 % quantiles of each boundary as
    experiment segment indices."""
    return posteriors.batch_event_extents(*q.at, anchors, event, window, *q.maps)


@_query('region_conditional_raw', 'has no conditional summaries', 'a list over restarts of lists over regions', cn='path',
        lacks_cn='conditional summaries')
def conditional_summary(q, regions, event, window='chain', cn=None, marginals=False):
    """"Suppose it is so: what follows?"  Exact per-segment posterior summaries given that a copy-number event holds over a
    region, under the structured posterior of the last variational update: regions is a list of (first, last) experiment
    segment indices, each an evidence of its own; event a mask name of posteriors.MASK_NAMES ('hdel': every segment of the
    region is homozygously deleted), a label name of posteriors.LABEL_NAMES, a (mask, label) pair, or a boolean
    (classes, states) table of the states the evidence allows; window 'chain' (the whole chain of the region) or the number
    of model segments on either side.  One dict per region: `log_evidence`, the log-probability of the event, and the
    arrays of posterior_summary without the entropy, in experiment segment order, NaN outside the window.  cn: a decoded
    path ([N][M][2], model segment order), which supplies cn_posterior_prob given the event.
    posteriors.evidence_shift compares a dict with posterior_summary()."""
    return posteriors.batch_conditional_summary(*q.at, regions, event, window, *q.maps, marginals=marginals, states=cn)


@_query('region_span_raw', 'has no event spans', 'a list over restarts of lists of posteriors.span_summary dicts, one per anchor')
def event_span(q, anchors, event, window=64):
    """The joint law of where a copy-number event begins and ends around anchor segments, and so of its length, exactly,
    under the structured posterior of the last variational update; anchors, event and window as event_extent (the
    window's table may hold at most 16 384 entries).  A list with one posteriors.span_summary dict per anchor: p_event,
    the joint survival function and pmf of (left end, right end), the length of every cell in the units of the segment
    lengths, the 5 / 50 / 95 % quantiles of the length and its distribution function."""
    return posteriors.batch_event_spans(*q.at, anchors, event, window, *q.maps, q.model.l1)


@_query('region_pattern_raw', 'has no region event patterns',
        'a dict of arrays (restarts, len(patterns)) and `p_parts`, a list over patterns of (restarts, parts) arrays', each=('p_parts',))
def event_joint(q, patterns):
    """The exact joint probability, under the structured posterior of the last variational update, of copy-number events
    at several regions: patterns is a list of patterns, each a list of parts (first, last, event) -- experiment segment
    indices and an event as event_extent takes it.  A dict of `log_p_joint`, `p_joint` and `lift` (len(patterns),) and
    `p_parts`, a list of (parts,) arrays: each part alone; lift = p_joint / prod p_parts.  Parts in different chains are
    independent; inside one chain nothing binds between the parts."""
    return posteriors.batch_event_joint(*q.at, patterns, *q.maps)


@_query('region_pattern_raw', 'has no region event patterns', 'a dict of arrays (restarts, len(regions))')
def focal_events(q, regions, flank=1):
    """Exact probabilities of focal events over regions ((first, last) experiment segment indices): a dict of arrays
    (len(regions),), p_focal_loh -- every segment of the region in LOH and none of the `flank` segments on each side of
    it, inside the chain --, p_focal_hdel and p_focal_subclonal likewise.  A side without segments drops out."""
    return posteriors.batch_focal_events(*q.at, regions, flank, *q.maps)


def _by_breakpoint(out, model, args, restart_axis):
    """breakend_changes(arrays=False): the arrays over breakpoints as a dict breakpoint -> its entries."""
    if args['arrays']:
        return out
    return dict((bp, dict((k, v[:, i] if restart_axis else v[i]) for k, v in out.items())) for i, bp in enumerate(model.breakpoints))


@_query('region_pattern_raw', 'has no region event patterns',
        'keyed by the breakpoints, a dict breakpoint -> dict of arrays with a leading restart axis; arrays=True: the dict of arrays '
        '(restarts, K, 2) and (restarts, K)', finish=_by_breakpoint)
def breakend_changes(q, arrays=False):
    """Whether the copy-number state changes at the two breakends of every breakpoint, jointly and exactly
    (posteriors.batch_breakend_changes): keyed like breakpoint_prob(), a dict breakpoint -> dict of p_change (2,),
    p_change_both, p_change_neither, p_change_only_first, p_change_only_second, log_p_same (2,) and log_p_same_both;
    arrays=True: the dict of arrays over breakpoints instead, (K, 2) and (K,)."""
    m = q.model
    return posteriors.batch_breakend_changes(*q.at, m.breakpoint_idx, m.num_breakpoints, m.is_telomere, m.seg_is_original)


@_query('region_decode_raw', 'has no region decode', '`cn` a list over restarts of lists over regions, the arrays (restarts, len(regions))',
        cn='call', extend=('cn',))
def region_call(q, regions, event=None, cn=None):
    """The most probable copy-number configuration of every region under the structured posterior of the last
    variational update, and its probability (posteriors.batch_region_calls): regions is a list of (first, last)
    experiment segment indices; event None, or (mask name or None, label name or None) -- the most probable
    configuration in which the event holds, e.g. ('hdel', None).  A dict of `cn`, a list over regions of (segments, M, 2)
    arrays, and arrays (len(regions),): log_prob, log_p_event, log_prob_given_event, and against the call cn ((N, M, 2)
    in experiment order; None: the decoded path) n_differ and log_prob_call."""
    return posteriors.batch_region_calls(*q.at, regions, *q.maps, event=event, cn=cn)


@_query('region_kbest_raw', 'has no region alternatives', 'a list over restarts of lists over regions of dicts', cn='call')
def region_alternatives(q, regions, k=4, event=None, cn=None):
    """The k most probable copy-number configurations of every region under the structured posterior of the last
    variational update (posteriors.batch_region_alternatives): what else could be there besides region_call's answer, and
    how much of the mass the list explains.  regions, event and cn as region_call; 1 <= k <= 8.  A list over regions of
    dicts: cn (a list over the found ranks of (segments, M, 2) arrays), log_prob (k,), log_p_event, log_prob_given_event
    (k,), coverage, n_differ (k,), rank_of_call and duplicate_of (k,)."""
    return posteriors.batch_region_alternatives(*q.at, regions, *q.maps, k=k, event=event, cn=cn)


@_query('call_logprob_raw', 'has no call probabilities', 'a dict of arrays (restarts, len(regions))', cn='call')
def call_confidence(q, regions, cn=None):
    """Exact probabilities, under the structured posterior of the last variational update, that the copy-number path
    agrees with a call over regions ((first, last) experiment segment indices): a dict of arrays (len(regions),),
    p_call (the path equals the call at every segment of the region), p_call_unphased (up to a swap of the two alleles)
    and p_call_total (the per-clone totals).  cn: the call, (N, M, 2) in experiment segment order as optimal_cn returns
    it; None: the decoded path.  Zero-length segments inserted at shared boundaries are marginalised."""
    return posteriors.batch_call_confidence(*q.at, cn, regions, *q.maps)


@_query('call_logprob_raw', 'has no call probabilities', '(restarts,)', cn='call', many=True)
def cn_logprob(q, cn=None):
    """log q(cn) under the structured posterior of the last variational update: the exact log-probability of a whole
    copy-number path, a float -- or (K,) for cn of shape (K, N, M, 2).  cn in experiment segment order as optimal_cn
    returns it; None: the decoded path.  Zero-length segments inserted at shared boundaries are marginalised.  -inf
    also where a state's forward entry underflowed in the sweep."""
    # (one path per restart, (nr, N1), or the model level's K paths, (1, K, N1))
    out = posteriors.batch_cn_logprob(*q.at, cn if cn.ndim == 3 else cn[:, None], q.model.seg_is_original, q.model.is_telomere)
    return out if cn.ndim == 3 else out[:, 0]


@_query('region_logprob_raw', 'has no region event probabilities', '(restarts, N - 1)')
def cn_change_prob(q):
    """(N - 1,): the posterior probability that the copy-number state changes between experiment segments n and n + 1
    (1 - p_no_change of the region [n, n + 1]); NaN where no reference adjacency joins them."""
    return posteriors.batch_change_prob(*q.at, *q.maps)


QUERIES = (posterior_summary, region_events, region_change_counts, region_cn_extremes, region_clone_extremes, region_cn_moments,
           event_extent, conditional_summary, event_span, event_joint, focal_events, breakend_changes, region_call,
           region_alternatives, call_confidence, cn_logprob, cn_change_prob)


@_query('locus_joint_raw', 'has no locus joints', '`bins`, `first_level` and arrays (restarts, len(pairs), ...)', shared=('bins', 'first_level'))
def locus_joint(q, pairs, feature=('total', 1), other=None, bins=8, first_level=0):
    """The exact joint posterior of copy number at two loci, under the structured posterior of the last variational update:
    is the gene above the arm it sits on, do the two sides of a rearrangement carry the same total, are both genes in LOH.
    pairs is a list of (first, second) experiment segment indices in any order; feature what is read at the first locus and
    other at the second (None: the same) -- (quantity, clone) with quantity 'total', 'major' or 'minor' and clone a tumour
    clone 1 .. M-1 or 'any', in the window first_level .. first_level + bins - 1 (the last bin meaning "or more"), or a mask
    name of posteriors.MASK_NAMES (level 1: the event holds).  A dict of `bins`, `first_level`, `log_joint` (len(pairs), bins,
    bins) with the first locus along axis -2, and the arrays of posteriors.joint_summary: joint, marginal_a, marginal_b,
    p_equal, p_a_higher, p_b_higher, difference_pmf, mean_difference, correlation, mutual_information and p_saturated.  Two
    loci in different chains are independent: their table is the product of the marginals."""
    return posteriors.batch_locus_joint(*q.at, pairs, *q.maps, feature=feature, other=other, bins=bins, first_level=first_level)


@_query('locus_joint_raw', 'has no locus joints', '`bins`, `first_level`, `segment` (len(anchors), 2 window + 1) and arrays (restarts, len(anchors), 2 window + 1)',
        shared=('bins', 'first_level', 'segment'))
def locus_dependence(q, anchors, window=32, feature=('total', 1), other=None, bins=8, first_level=0):
    """How far along the chain knowing one segment tells anything about another: for every anchor (an experiment segment index)
    and each of the `window` experiment segments on either side of it inside its chain, the mutual information (nats), the
    correlation and the probability of equality between `feature` at the anchor and `other` at the neighbour (feature, other,
    bins and first_level as locus_joint).  A dict of `bins`, `first_level`, `segment` (len(anchors), 2 window + 1) -- the
    neighbours' experiment indices, the anchor in the middle, -1 outside the chain -- and `mutual_information`, `correlation`
    and `p_equal` of that shape, NaN outside the chain."""
    return posteriors.batch_locus_dependence(*q.at, anchors, *q.maps, window=window, feature=feature, other=other, bins=bins, first_level=first_level)


# (QUERIES is a closed list: tests compare its names with theirs.  Later entries go here; BY_NAME and `answers` run over both)
LATER_QUERIES = (locus_joint, locus_dependence)


@_query('region_automaton_raw', 'has no region automata', 'a dict of arrays (restarts, len(regions), ...)')
def region_automaton(q, regions, automaton, symbols, accept=None):
    """The exact posterior, under the structured posterior of the last variational update, of a regular property of regions
    ((first, last) experiment segment indices, each inside one chain): automaton is a posteriors.Automaton with at most 16
    states over at most 16 symbols -- posteriors.automaton_runs, automaton_run_of, automaton_switches, or
    posteriors.reverse_automaton of a left-to-right one --, symbols an int (classes, states) table as posteriors.symbols_from
    gives.  The automaton reads a region FROM ITS LAST SEGMENT TO ITS FIRST, one symbol per real segment.  A dict of `log_final`
    and `final` (len(regions), Q), the distribution of the automaton's final state, and with accept (state indices or a
    boolean per state) `p_accept` (len(regions),)."""
    return posteriors.batch_region_automaton(*q.at, regions, *q.maps, automaton=automaton, symbols=symbols, accept=accept)


@_query('region_automaton_raw', 'has no region automata', 'a dict of arrays (restarts, len(regions), ...)')
def event_runs(q, regions, event, bins=8):
    """How many separate events regions hold ((first, last) experiment segment indices): three distinct homozygous deletions
    or one.  event is a mask name of posteriors.MASK_NAMES or a boolean (classes, states) table (posteriors.level_mask).  A
    dict of `num_events` (len(regions), bins) -- entry k the exact posterior probability of exactly k maximal runs of real
    segments in the event, the last entry that of bins - 1 or more -- and `p_any` (len(regions),).  A run does not cross a
    chromosome end."""
    return posteriors.batch_event_runs(*q.at, regions, *q.maps, event=event, bins=bins)


@_query('region_automaton_raw', 'has no region automata', 'a dict of arrays (restarts, len(regions))')
def event_run_of(q, regions, event, k):
    """Whether an event (as event_runs) is supported by at least k consecutive real segments somewhere in a region: a dict of
    `p_run` (len(regions),), the exact posterior probability.  A one-segment blip is not a call."""
    return posteriors.batch_event_run_of(*q.at, regions, *q.maps, event=event, k=k)


# (LATER_QUERIES is compared with a closed list too; the automaton queries have a tuple of their own)
AUTOMATON_QUERIES = (region_automaton, event_runs, event_run_of)
ALL_QUERIES = QUERIES + LATER_QUERIES + AUTOMATON_QUERIES
BY_NAME = dict((e.name, e) for e in ALL_QUERIES)


@_query('path_entropy_raw', 'has no path entropy', 'a dict of arrays with a leading restart axis')
def path_entropy(q, regions=None):
    """How uncertain regions are at all: the exact Shannon entropy, in nats, of the copy-number path posterior of the last
    variational update over regions ((first, last) experiment segment indices; None: one region, the genome).  A dict of
    `segment_entropy` (N,), the entropy of every segment's marginal; `step_entropy` (N - 1,), H(c_n | c_n+1) between experiment
    segments n and n + 1, and `adjacent_information` (N - 1,), their mutual information, both NaN where no reference adjacency
    joins them; and per region `path_entropy`, the entropy of the joint configuration of the region (chains add),
    `inserted_slack` (the entropy of the real segments alone lies in [path_entropy - inserted_slack, path_entropy]: the
    zero-length segments inserted at breakends are part of the path), `marginal_entropy_sum`, `total_correlation` (what the sum
    of the marginal entropies overstates), `perplexity` = exp(path_entropy), the effective number of configurations, and
    `entropy_per_segment` (posteriors.batch_path_entropy)."""
    return posteriors.batch_path_entropy(*q.at, regions, *q.maps)


# (ALL_QUERIES and BY_NAME are compared with closed lists as well: `entry` looks a name up in every tuple, `answers` installs them all)
ENTROPY_QUERIES = (path_entropy,)


@_query('region_sums_raw', 'has no region sums', '`bins` and arrays (restarts, len(regions), ...)', shared=('bins', 'unit', 'length', 'exact'))
def region_sums(q, regions, levels, weights, bins=None):
    """The exact posterior distribution, under the structured posterior of the last variational update, of the additive
    functional sum_n weights[n] levels(c_n) over regions ((first, last) experiment segment indices): levels an int
    (classes, states) table with entries >= 0, weights non-negative integers PER MODEL SEGMENT (0: the segment does not count;
    give the inserted zero-length segments 0), bins None: the most the state count allows (posteriors.sums_max_bins).  Exact
    for these integer weights.  A dict of `bins`, `pmf` (len(regions), bins) -- entry k the probability that the sum is k,
    the last entry that of bins - 1 or more --, `mean` and `p_saturated` (len(regions),).  Pieces of a region in several
    chains add."""
    return posteriors.batch_region_sums(*q.at, regions, *q.maps, levels=levels, weights=weights, bins=bins)


@_query('region_sums_raw', 'has no region sums', '`bins`, `unit`, `length`, `exact` (len(regions),) and arrays (restarts, len(regions), ...)',
        shared=('bins', 'unit', 'length', 'exact'))
def event_occupancy(q, regions, event, weights='length', bins=None, unit=None):
    """How much of a region is in an event -- 'at least half of 17p is in LOH', 'the gene's segments carry at least twelve
    copies between them', 'how many of these segments are subclonal' -- as a distribution, not a mean and an SD: regions is a
    list of (first, last) experiment segment indices; event a mask name of posteriors.MASK_NAMES, a boolean
    (classes, states) table (posteriors.level_mask), or a (quantity, clone) feature as locus_joint takes it (the level is that
    copy number).  weights 'segments': every real segment weighs 1 and the distribution is EXACT.  weights 'length': a real
    segment weighs its length in units of `unit` (None: chosen per region so that nothing saturates); exact where every
    length is a multiple of the unit (`exact`), otherwise a RIGOROUS BRACKET and no approximation: for every path
    unit * (floor sum) <= true weighted sum <= unit * (ceil sum).  The bracket is as wide as the number of real segments whose
    length is no multiple of the unit, so arm-sized regions of thousands of unequal segments get a loose bracket.  A dict of
    `bins`, `unit`, `length`, `exact` (len(regions),), `pmf_floor` and `pmf_ceil` (len(regions), bins; the last entry means
    bins - 1 units or more), `mean_floor`, `mean_ceil` and `p_saturated` (len(regions),); posteriors.occupancy_at_least gives
    the bounds of P(weighted fraction >= f) (posteriors.batch_event_occupancy)."""
    return posteriors.batch_event_occupancy(*q.at, regions, *q.maps, q.model.l1, event, weights=weights, bins=bins, unit=unit)


# (the closed lists above stay what they are: `entry` looks a name up in every tuple, `answers` installs them all)
SUM_QUERIES = (region_sums, event_occupancy)


def entry(name):
    """The table's entry of a query by its name, whichever tuple holds it."""
    for e in ALL_QUERIES + ENTROPY_QUERIES + SUM_QUERIES:
        if e.name == name:
            return e
    raise KeyError(name)


# ---- a result along the restart axis ----------------------------------------------------------------------------------------
def _join(parts, shared=(), extend=(), each=()):
    """One query's results from several groups of restarts, as of all their restarts in order.  Lists over restarts are
    strung together, bare arrays concatenated.  Of dicts, the arrays are concatenated along the restart axis, except the keys
    named in `shared` (the same in every part: the first part's), in `extend` (lists over restarts: strung together) and in
    `each` (lists of arrays with a restart axis: concatenated entry by entry)."""
    if isinstance(parts[0], np.ndarray):
        return np.concatenate(parts)
    if not isinstance(parts[0], dict):
        return [x for part in parts for x in part]

    def one(k):
        values = [part[k] for part in parts]
        if k in shared:
            return values[0]
        if k in extend:
            return [x for v in values for x in v]
        if k in each:
            return [np.concatenate(v) for v in zip(*values)]
        return np.concatenate(values)
    return dict((k, one(k)) for k in parts[0])


def _only(entry, out):
    """The single restart's entry of a result of one restart: exactly the restart axis goes."""
    if isinstance(out, np.ndarray) and out.ndim == 1:
        return float(out[0])                                         # (cn_logprob of one path)
    if not isinstance(out, dict):
        return out[0]
    return dict((k, v if k in entry.shared else [x[0] for x in v] if k in entry.each else v[0]) for k, v in out.items())


# ---- the four levels --------------------------------------------------------------------------------------------------------
def _lacking(entry, model):
    return NotImplementedError('kernel module %s %s' % (getattr(model._kernel_module(), '__name__', '?'), entry.lacks))


def _model_level(self, entry, args):
    """BreakpointModel: restart self.model._r of its batch alone, the restart axis stripped."""
    b = getattr(self.model, '_batch', None)
    if b is None or not hasattr(b, entry.needs):
        raise _lacking(entry, self)
    if entry.cn == 'call':
        several = args['cn'] is not None and np.ndim(args['cn']) == 4
        if several and not entry.many:
            raise ValueError('%s takes one call of shape (num_segments, num_clones, 2)' % entry.name)
        states = self._call_states(args['cn'])
        args['cn'] = states[None] if several else states
    elif entry.cn and args['cn'] is not None:
        args['cn'] = posteriors.cn_to_states(args['cn'], b.cn_classes, b.seg_class)[None]      # (a path in MODEL segment order)
    out = _only(entry, entry.call(Restarts(b, self.model._r, 1, [self]), **args))
    return entry.finish(out, self, args, False) if entry.finish else out


def _set_level(self, entry, args, finish=True):
    """RestartSet: all restarts of its batch from one call."""
    b = self.batch
    if b is None or not hasattr(b, entry.needs):
        if entry.cn == 'path' and args['cn'] is not None:
            raise NotImplementedError('%s against a decoded path need the batched kernel module' % entry.lacks_cn)
        raise _lacking(entry, self.models[0])
    if entry.cn == 'call' or (entry.cn and args['cn'] is not None):
        args['cn'] = self._call_states(args['cn'])
    out = entry.call(Restarts(b, 0, len(self.models), self.models), **args)
    return entry.finish(out, self.models[0], args, True) if entry.finish and finish else out


def _groups_level(self, entry, args, finish=True):
    """RestartGroups: its sets side by side, each with its slice of `cn`, joined in restart order."""
    def one(rs):
        own = dict(args, cn=self._own(rs, args['cn'])) if entry.cn else dict(args)
        return _set_level(rs, entry, own, finish=False)
    out = _join(self._map(one), entry.shared, entry.extend, entry.each)
    return entry.finish(out, self.models[0], args, True) if entry.finish and finish else out


def _datasets_level(self, entry, args):
    """DatasetGroups: every dataset's RestartGroups with its entry of `cn`: a list, one result per dataset."""
    def one(part):
        own = dict(args, cn=self._own(part, args['cn'])) if entry.cn else dict(args)
        return _groups_level(part, entry, own)
    out = self._map(one)
    return _join(out) if entry.flat else out


_CN_WORDS = {None: '', 'call': "  cn: the restarts' calls in experiment order (the `cn` of results()); None: the decoded paths.",
             'path': "  cn: the restarts' decoded paths in experiment order (the `cn` of results()), or None."}
# level: (its body, its help from an entry)
LEVELS = {
    'model': (_model_level, lambda e: e.doc),
    'set': (_set_level, lambda e: 'BreakpointModel.%s of every restart from one device call per kernel: %s.%s' % (e.name, e.result, _CN_WORDS[e.cn])),
    'groups': (_groups_level, lambda e: 'RestartSet.%s over the groups, restarts in order%s: %s.' % (e.name, ' (cn: of all restarts)' if e.cn else '', e.result)),
    'datasets': (_datasets_level, lambda e: 'RestartGroups.%s of every dataset%s: %s.' % (
        e.name, " (cn: per dataset, a list of its restarts' paths)" if e.cn else '',
        'dataset after dataset, ' + e.result if e.flat else 'a list, per dataset ' + e.result)),
}


def _method(cls, entry, body, doc):
    params = list(inspect.signature(entry.call).parameters.values())
    signature = inspect.Signature([inspect.Parameter('self', inspect.Parameter.POSITIONAL_OR_KEYWORD)] + params[1:])

    def method(self, *args, **kwargs):
        bound = signature.bind(self, *args, **kwargs)
        bound.apply_defaults()
        given = dict(bound.arguments)
        del given['self']
        return body(self, entry, given)
    method.__name__ = entry.name
    method.__qualname__ = '%s.%s' % (cls.__qualname__, entry.name)
    method.__module__ = cls.__module__
    method.__doc__ = doc
    method.__signature__ = signature
    return method


def answers(level):
    """Class decorator: every query of the table as a method of the class, with the body and the help of `level`."""
    body, doc = LEVELS[level]

    def install(cls):
        for e in ALL_QUERIES + ENTROPY_QUERIES + SUM_QUERIES:
            setattr(cls, e.name, _method(cls, e, body, doc(e)))
        return cls
    return install
