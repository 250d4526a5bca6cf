"""Algorithm parameters of the hot path, values of the reference's
remixt/defaults.py:113-163, with its `get_param` overlay semantics
(remixt/config.py:5-12: a key present in the config dict wins)."""

max_copy_number = 12
tumour_mix_fractions = [0.45, 0.3, 0.2, 0.1]
min_ploidy = 1.5
max_ploidy = 6.0
h_normal = None
h_tumour = None
max_prop_diverge = 0.5
normal_contamination = True
likelihood_min_segment_length = 10000
likelihood_min_proportion_genotyped = 0.01
divergence_weights = [1e-6, 1e-7, 1e-8]
num_em_iter = 5
num_update_iter = 5
disable_breakpoints = False
do_h_update = True
is_female = True
# (no reference counterpart) posterior copy-number samples per restart behind every fit result: 0 = none (results unchanged);
# K > 0 adds cn_sample_agreement, cn_state_agreement and ploidy / proportion_divergent quantiles (remixt_amd/sampling.py)
num_cn_samples = 0
cn_sample_seed = 0
# (no reference counterpart) exact per-segment posterior summaries behind every fit result: False = none (results unchanged);
# True adds cn_posterior_prob / _max / _entropy, p_subclonal, p_loh, p_hdel, total_cn_mean, total_cn_sd and the stats
# ploidy_posterior_mean / proportion_divergent_posterior_mean (remixt_amd/posteriors.py)
cn_posterior_summary = False
# (no reference counterpart) exact posterior probabilities of copy-number events over regions behind every fit result:
# None = none (results unchanged); a list of (name, first, last) experiment segment intervals adds `region_events` -- the
# names and p_all_loh, p_any_loh, p_all_hdel, p_any_hdel, p_any_subclonal, p_no_change, p_no_total_change per region
# (remixt_amd/posteriors.py)
cn_regions = None
# (no reference counterpart) with cn_regions: the exact posterior distribution of the number of copy-number changes inside
# every region, in this many bins (the last: that many changes minus one, or more).  0 = none (results unchanged);
# 1 .. 16 adds `region_change_counts` -- names, bins, num_changes (state changes) and num_total_changes (changes of the
# per-clone totals), each (regions, bins) -- to every fit result (remixt_amd/posteriors.py)
cn_region_change_bins = 0
# (no reference counterpart) with cn_regions: the exact posterior probability that the reported call holds.  False = none
# (results unchanged); True adds `call_confidence` -- names, p_call (the path equals the result's `cn` at every segment of
# the region), p_call_unphased (up to a swap of the alleles) and p_call_total (the per-clone totals) -- and the stat
# cn_logprob, log q of the whole `cn`, to every fit result (remixt_amd/posteriors.py)
cn_call_confidence = False
# (no reference counterpart) with cn_regions: the exact posterior mean and covariance of copy number over regions.  False =
# none (results unchanged); True adds `region_cn_moments` -- names, length, total_cn_mean / total_cn_cov (the length-weighted
# mean copy number of each clone over the region and its covariance matrix) and fraction_mean / fraction_cov (the length
# fractions of posteriors.MOMENT_FRACTIONS) -- and the stats ploidy_posterior_sd and proportion_divergent_posterior_sd to
# every fit result (remixt_amd/posteriors.py)
cn_region_moments = False
# where copy-number events begin and end around anchor segments: a list of (name, segment, event) -- segment an
# experiment segment index, event a mask name of posteriors.MASK_NAMES ('loh': the LOH run around the segment), a label name
# of posteriors.LABEL_NAMES ('state' / 'total': the constant-state / constant-total run around it) or a (mask, label) pair --
# adds `event_extents` to every fit result: the probability of the event at the segment and the exact 5 / 50 / 95 % posterior
# quantiles of where it starts and stops, with a flag where a quantile lies beyond cn_extent_window segments on that side
# (remixt_amd/posteriors.py).  None: off
cn_event_extents = None
cn_extent_window = 64

# Exact posterior of the length of the events of cn_event_extents (it needs them): every fit result also carries
# `event_lengths` -- per entry the 5 / 50 / 95 % quantiles of the event's length (the sum of the segment lengths between its
# two ends, given the event at the segment) with a flag where a quantile is not reached inside the window, and, for every
# length of cn_event_length_edges (each > 0), P(length <= edge) and the mass for which the window cannot tell -- from the
# joint law of the two ends over cn_extent_window segments on each side, whose table may hold at most 16 384 entries
# (remixt_amd/posteriors.py).  False: off
cn_event_lengths = False
cn_event_length_edges = ()

# Exact joint posterior of a copy-number change at the two breakends of every breakpoint: every fit result also carries
# `p_change` (K, 2) -- the probability that the copy-number state changes across each breakend's adjacency -- and the
# 2 x 2 table of the two, `p_change_both`, `p_change_neither`, `p_change_only_first`, `p_change_only_second` (K,), breakpoints
# in the order of the experiment's `breakpoints` (remixt_amd/posteriors.py batch_breakend_changes).  False: off
cn_breakend_changes = False

# The most probable copy-number configuration of every region of cn_regions and its probability (rmx_region_decode, DESIGN
# 4.17): every fit result also carries `region_calls` -- names, log_prob (the log-probability of the region's most probable
# configuration under the structured posterior), log_prob_call (that of the result's own `cn` over the region) and n_differ
# (the number of the region's segments where the two differ).  The configurations themselves come from region_call of the
# model and restart classes.  Needs cn_regions.  False: off (results, records and stores unchanged)
cn_region_calls = False

# The exact posterior distribution of the highest and of the lowest total copy number of every tumour clone over every region
# of cn_regions (rmx_region_extremes): every fit result also carries `region_cn_extremes` -- names, bins (16),
# peak_total_pmf and floor_total_pmf, (regions, M - 1, bins) each: entry k is the probability that the clone's highest (lowest)
# total copy number over the region's segments is k, the last entry that of bins - 1 or more.  Other quantities, windows and
# 'any clone' come from region_cn_extremes of the model and restart classes.  Needs cn_regions.  False: off (results,
# records and stores unchanged)
cn_region_extremes = False


def get_param(config, name):
    if config is not None and name in config:
        return config[name]
    return globals()[name]


def get_sample_config(config, sample_id):
    """remixt/config.py:56-59: the config with the `sample_specific[sample_id]` overrides applied on top."""
    sample_config = dict(config or {})
    sample_config.update((config or {}).get('sample_specific', dict()).get(sample_id, dict()))
    return sample_config
