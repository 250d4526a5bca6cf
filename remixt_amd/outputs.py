"""The optional outputs of a fit, each described once, in record order.

An output is switched on by config keys (remixt_amd/defaults.py).  `resolve` checks a config against the whole table before
any fit and returns the selection: output name -> what its check returns, None where it is off.  Everything that depends
on which outputs are on walks OUTPUTS with that selection: restarts.add_optional_outputs (compute), the result record of
restarts._record_sections (section) and analysis.pipeline.store_fit_results (store)."""
import collections

import numpy as np

from . import defaults, posteriors, sampling

# name: the selection's key.  keys: the config keys it reads.  switch: the keyword of restarts._record_sections it answers
# to; as_switch(value): that keyword's value, value None (off) included.  resolve(config, num_segments) -> value, None = off (a ValueError for a bad
# combination).  compute(rs, results, experiment, init_ids, sel): query every restart of rs -- anything with the query
# methods of restarts.RestartSet -- and add the output to results[r]; sel: the whole selection (the outputs over regions
# read the regions).  section(sw, N, M, K) -> its section of the float record (record_section) under the record switches
# sw, None where they leave it out.  store(put, fit_results): put(key, table) what a result holds of it.
Output = collections.namedtuple('Output', 'name keys switch as_switch resolve compute section store')

Section = collections.namedtuple('Section', 'length pack unpack')      # pack(res, stats, view), unpack(view, res, stats)


def record_section(fields, group=None, head=(), tail=(), add=None):
    """One optional section of a float record: the stats `head`, the arrays `fields` ((name, shape), read from res, or
    from res[group]) and the stats `tail`.  Unpacking puts the arrays into res, or hands them, with the tail values, to
    add(res, arrays, *tail values)."""
    sizes = [int(np.prod(shape)) for _, shape in fields]

    def pack(res, stats, view):
        src = res if group is None else res[group]
        view[:len(head)] = [stats[k] for k in head]
        o = len(head)
        for (k, _), n in zip(fields, sizes):
            view[o:o + n] = np.asarray(src[k]).ravel(); o += n
        view[o:] = [stats[k] for k in tail]

    def unpack(view, res, stats):
        stats.update((k, float(v)) for k, v in zip(head, view))
        o = len(head); arrays = {}
        for (k, shape), n in zip(fields, sizes):
            arrays[k] = view[o:o + n].reshape(shape).copy(); o += n
        if add is None:
            res.update(arrays)
        else:
            add(res, arrays, *view[o:])
    return Section(len(head) + sum(sizes) + len(tail), pack, unpack)


def _get(config, key):
    return defaults.get_param(config, key)


def _is_on(value):
    return value is not None


def _names(value):
    """(the names lead the parsed regions and the parsed extents)"""
    return None if value is None else value[0]


def _flag(key):
    return lambda config, n: True if _get(config, key) else None


def _series_or_frame(v):
    import pandas as pd
    v = np.asarray(v)
    return pd.Series(v) if v.ndim == 1 else pd.DataFrame(v if v.ndim == 2 else v.reshape(len(v), -1))


def _store(arrays, group=None, prefix='', names=None):
    """store(): the named arrays of fit_results[group] (None: of fit_results itself) under prefix + name, a Series or
    (trailing axes side by side) a DataFrame each, behind the group's names under `names`."""
    def store(put, res):
        import pandas as pd
        if (arrays[0] if group is None else group) in res:
            src = res if group is None else res[group]
            if names is not None:
                put(names, pd.Series(list(src['names'])))
            for k in arrays:
                put(prefix + k, _series_or_frame(src[k]))
    return store


def _per_restart(arrays, r, shared=()):
    return dict((k, v if k in shared else v[r]) for k, v in arrays.items())


# ---- compute: the queries of every restart, scattered to results[r] ---------------------------------------------------------
def _samples(rs, results, experiment, init_ids, sel):
    num_samples, seed = sel['samples']
    for res, smp in zip(results, rs.sample_cn(num_samples, seed, init_ids=list(init_ids))):
        sampling.add_sample_summary(res, smp, experiment.l)


def _posterior_summary(rs, results, experiment, init_ids, sel):
    """(cn_posterior_prob is taken at results[r]['cn'])"""
    for res, s in zip(results, rs.posterior_summary(cn=[res['cn'] for res in results])):
        posteriors.add_posterior_summary(res, s, experiment.l)


def _regional(query, add, shared=()):
    """compute() of an output over the regions: query(rs, regions, results, sel) -> arrays with a leading restart axis (the keys
    in `shared`: without one), add(res, names, restart r's arrays, sel)."""
    def compute(rs, results, experiment, init_ids, sel):
        names, regions = sel['region_events']
        out = query(rs, regions, results, sel)
        for r, res in enumerate(results):
            add(res, names, _per_restart(out, r, shared), sel)
    return compute


def _call_confidence(rs, results, experiment, init_ids, sel):
    """(each restart for its own `cn`)"""
    names, regions = sel['region_events']
    cn = [res['cn'] for res in results]
    conf = rs.call_confidence(regions, cn=cn)
    logprob = rs.cn_logprob(cn=cn)
    for r, res in enumerate(results):
        posteriors.add_call_confidence(res, names, _per_restart(conf, r), logprob[r])


def _event_extents(rs, results, experiment, init_ids, sel):
    names, anchors, events, window = sel['event_extents']
    for res, ext in zip(results, posteriors.grouped_event_extents(rs.event_extent, anchors, events, window)):
        posteriors.add_event_extents(res, names, ext)


def _event_lengths(rs, results, experiment, init_ids, sel):
    names, anchors, events, window, edges = sel['event_lengths']
    for res, ln in zip(results, posteriors.grouped_event_spans(rs.event_span, anchors, events, window, edges)):
        posteriors.add_event_lengths(res, names, ln)


def _breakend_changes(rs, results, experiment, init_ids, sel):
    ch = rs.breakend_changes(arrays=True)
    for r, res in enumerate(results):
        posteriors.add_breakend_changes(res, _per_restart(ch, r))


# ---- section: what a float record carries of an output (restarts._record_sections has the layout in words) -------------------
def _over_regions(switch, fields, group, tail=(), add=None):
    """section(): one over the regions, on with `switch` (None: with the regions themselves).  fields(nreg, M, sw)."""
    def section(sw, N, M, K):
        names = sw['region_names']
        if names is None or not (switch is None or sw[switch]):
            return None
        return record_section(fields(len(names), M, sw), group, tail=tail, add=lambda res, a, *t: add(res, names, sw, a, *t))
    return section


def _samples_section(sw, N, M, K):
    if sw['cn_samples']:
        return record_section([('cn_sample_agreement', (N, M)), ('cn_state_agreement', (N,))], head=sampling.SUMMARY_STATS)


def _posterior_section(sw, N, M, K):
    if sw['cn_posterior']:
        return record_section([(k, (N, M) if k.startswith('total_cn') else (N,)) for k in posteriors.COMPACT_ARRAYS], head=posteriors.SUMMARY_STATS)


def _extents_section(sw, N, M, K):
    names = sw['extent_names']
    if names is not None:
        return record_section([(k, (len(names),)) for k in posteriors.EXTENT_ARRAYS], 'event_extents',
                              add=lambda res, a: posteriors.add_event_extents(res, names, a))


def _lengths_section(sw, N, M, K):
    names, edges = sw['extent_names'], sw['length_edges']
    if names is not None and edges is not None:
        nent = len(names)
        return record_section([(k, (nent,)) for k in posteriors.SPAN_ARRAYS] + [(k, (nent, int(edges))) for k in posteriors.SPAN_EDGE_ARRAYS],
                              'event_lengths', add=lambda res, a: posteriors.add_event_lengths(res, names, a))


def _breakend_section(sw, N, M, K):
    if sw['breakend_changes']:
        return record_section([(k, (K, 2) if k == 'p_change' else (K,)) for k in posteriors.BREAKEND_ARRAYS])


def _moment_fields(nreg, M, sw):
    shapes = posteriors.moment_shapes(nreg, M)
    return [(k, shapes[k]) for k in posteriors.MOMENT_ARRAYS]


OUTPUTS = (
    Output('samples', ('num_cn_samples', 'cn_sample_seed'), 'cn_samples', _is_on,
           lambda config, n: (_get(config, 'num_cn_samples'), _get(config, 'cn_sample_seed')) if _get(config, 'num_cn_samples') > 0 else None,
           _samples, _samples_section, _store(('cn_sample_agreement', 'cn_state_agreement'))),
    Output('posterior_summary', ('cn_posterior_summary',), 'cn_posterior', _is_on, _flag('cn_posterior_summary'),
           _posterior_summary, _posterior_section, _store(posteriors.COMPACT_ARRAYS)),
    Output('region_events', ('cn_regions',), 'region_names', _names,
           lambda config, n: None if _get(config, 'cn_regions') is None else posteriors.parse_regions(_get(config, 'cn_regions')),
           _regional(lambda rs, regions, results, sel: rs.region_events(regions),
                     lambda res, names, a, sel: posteriors.add_region_events(res, names, a)),
           _over_regions(None, lambda nreg, M, sw: [(k, (nreg,)) for k in posteriors.REGION_ARRAYS], 'region_events',
                         add=lambda res, names, sw, a: posteriors.add_region_events(res, names, a)),
           _store(posteriors.REGION_ARRAYS, 'region_events', names='region_names')),
    Output('change_counts', ('cn_region_change_bins',), 'change_bins', lambda v: 0 if v is None else int(v), lambda config, n: posteriors.change_bins(config) or None,
           _regional(lambda rs, regions, results, sel: rs.region_change_counts(regions, sel['change_counts']),
                     lambda res, names, a, sel: posteriors.add_region_change_counts(res, names, sel['change_counts'], a)),
           _over_regions('change_bins', lambda nreg, M, sw: [(k, (nreg, int(sw['change_bins']))) for k in posteriors.COUNT_ARRAYS], 'region_change_counts',
                         add=lambda res, names, sw, a: posteriors.add_region_change_counts(res, names, sw['change_bins'], a)),
           _store(posteriors.COUNT_ARRAYS, 'region_change_counts')),
    Output('call_confidence', ('cn_call_confidence',), 'call_confidence', _is_on, lambda config, n: posteriors.call_confidence_on(config) or None,
           _call_confidence,
           _over_regions('call_confidence', lambda nreg, M, sw: [(k, (nreg,)) for k in posteriors.CALL_ARRAYS], 'call_confidence', tail=('cn_logprob',),
                         add=lambda res, names, sw, a, logprob: posteriors.add_call_confidence(res, names, a, logprob)),
           _store(posteriors.CALL_ARRAYS, 'call_confidence')),
    # (in a store total_cn_mean is also a per-segment array: region_ in front)
    Output('region_moments', ('cn_region_moments',), 'cn_moments', _is_on, lambda config, n: posteriors.region_moments_on(config) or None,
           # (the named regions and the whole genome, for the two *_posterior_sd stats, in the same device call)
           _regional(lambda rs, regions, results, sel: rs.region_cn_moments(posteriors.genome_region(regions, len(results[0]['cn']) if results else 1)),
                     lambda res, names, a, sel: posteriors.add_region_cn_moments(res, names, a), shared=('length',)),
           _over_regions('cn_moments', _moment_fields, 'region_cn_moments', tail=posteriors.MOMENT_STATS,
                         add=lambda res, names, sw, a, *sd: posteriors.add_region_cn_moments(res, names, a, sd)),
           _store(posteriors.MOMENT_ARRAYS, 'region_cn_moments', 'region_')),
    Output('event_extents', ('cn_event_extents', 'cn_extent_window'), 'extent_names', _names, posteriors.extents_on,
           _event_extents, _extents_section, _store(posteriors.EXTENT_ARRAYS, 'event_extents', 'extent_', names='extent_names')),
    Output('event_lengths', ('cn_event_lengths', 'cn_event_length_edges'), 'length_edges', lambda v: None if v is None else len(v[4]), posteriors.lengths_on,
           _event_lengths, _lengths_section,
           _store(posteriors.SPAN_ARRAYS + posteriors.SPAN_EDGE_ARRAYS, 'event_lengths', 'span_', names='span_names')),
    Output('breakend_changes', ('cn_breakend_changes',), 'breakend_changes', _is_on, _flag('cn_breakend_changes'),
           _breakend_changes, _breakend_section, _store(posteriors.BREAKEND_ARRAYS, prefix='breakend_')),
    Output('region_calls', ('cn_region_calls',), 'region_calls', _is_on, lambda config, n: posteriors.region_calls_on(config) or None,
           _regional(lambda rs, regions, results, sel: rs.region_call(regions, cn=[res['cn'] for res in results]),      # (against results[r]['cn'])
                     lambda res, names, a, sel: posteriors.add_region_calls(res, names, a)),
           _over_regions('region_calls', lambda nreg, M, sw: [(k, (nreg,)) for k in posteriors.REGION_CALL_ARRAYS], 'region_calls',
                         add=lambda res, names, sw, a: posteriors.add_region_calls(res, names, a)),
           _store(posteriors.REGION_CALL_ARRAYS, 'region_calls', 'region_call_')),
    # (in a store a row per region, the clones' bins side by side)
    Output('region_extremes', ('cn_region_extremes',), 'region_extremes', _is_on, lambda config, n: posteriors.region_extremes_on(config) or None,
           _regional(lambda rs, regions, results, sel: rs.region_clone_extremes(regions, posteriors.EXTREME_BINS),
                     lambda res, names, a, sel: posteriors.add_region_cn_extremes(res, names, a)),
           _over_regions('region_extremes', lambda nreg, M, sw: [(k, (nreg, M - 1, posteriors.EXTREME_BINS)) for k in posteriors.EXTREME_ARRAYS],
                         'region_cn_extremes', add=lambda res, names, sw, a: posteriors.add_region_cn_extremes(res, names, a)),
           _store(posteriors.EXTREME_ARRAYS, 'region_cn_extremes', 'region_')),
)
CONFIG_KEYS = tuple(k for o in OUTPUTS for k in o.keys)
# a store holds the breakend changes behind everything else (they were stored last before the table, and stay there)
STORE_ORDER = tuple(o for o in OUTPUTS if o.name != 'breakend_changes') + tuple(o for o in OUTPUTS if o.name == 'breakend_changes')
# the record switches with every output off
SWITCHES_OFF = dict((o.switch, o.as_switch(None)) for o in OUTPUTS)


class Selection(collections.OrderedDict):
    """Output name -> resolved value, None where the output is off, in table order."""

    def record_switches(self):
        """The keywords of restarts._record_sections / _pack / _unpack / gather_result_records for this selection."""
        return dict((o.switch, o.as_switch(self[o.name])) for o in OUTPUTS)


def resolve(config, num_segments=None):
    """The selection of a config, every output checked (ValueError for an output without what it needs or a value out of
    range) before any fit.  num_segments: the experiment's number of segments, where known."""
    return Selection((o.name, o.resolve(config, num_segments)) for o in OUTPUTS)
