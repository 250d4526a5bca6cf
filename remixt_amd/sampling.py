"""Posterior copy-number samples: per-restart seeds and summaries of a set of samples.

The paths themselves are drawn on the device (`rmx_sample_cn`, forward-filtering backward-sampling over the
structured posterior q(c) of the last update_p_cn).  Here: the seed of a restart, derived from (user seed, init_id) so
that a restart's samples do not depend on how restarts are grouped or sharded, and the per-segment agreement with the
decoded path and sample quantiles of ploidy and proportion_divergent (the statistics of analysis/pipeline.py)."""
import numpy as np

_MASK64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def restart_seed(seed, init_id):
    """64-bit Philox key of restart `init_id` under the user's `seed`."""
    return _splitmix64(_splitmix64(int(seed) & _MASK64) ^ (int(init_id) & _MASK64))


def ploidy_and_divergence_samples(samples, l):
    """tumour_ploidy_and_divergence's statistics of every sample at once: samples (K, N, M, 2) ->
    (ploidy (K,), proportion_divergent (K,)) with the formulas of analysis/pipeline.py."""
    t = np.asarray(samples)[:, :, 1:, :]
    l = np.asarray(l, dtype=float)
    mean = t.sum(axis=2) / t.shape[2]                                  # (K, N, 2)
    ploidy = (mean * l[None, :, None]).sum(axis=(1, 2)) / l.sum()
    divergent = (t.max(axis=2) != t.min(axis=2)) * 1.                   # (K, N, 2)
    prop = (divergent * l[None, :, None]).sum(axis=(1, 2)) / (2. * l.sum())
    return ploidy, prop


def sample_summary(samples, cn, l):
    """(arrays, stats) of K posterior samples (K, N, M, 2) against the decoded cn (N, M, 2), all in experiment segment
    order.  arrays: cn_sample_agreement (N, M) -- fraction of samples whose (major, minor) of clone m equals cn --
    and cn_state_agreement (N,) -- the same for the whole state; stats: 5 / 50 / 95 % quantiles of ploidy and
    proportion_divergent over the samples."""
    samples = np.asarray(samples)
    cn = np.asarray(cn)
    eq = (samples == cn[None]).all(axis=3)                              # (K, N, M)
    arrays = {'cn_sample_agreement': eq.mean(axis=0), 'cn_state_agreement': eq.all(axis=2).mean(axis=0)}
    ploidy, prop = ploidy_and_divergence_samples(samples, l)
    stats = {}
    for name, v in (('ploidy', ploidy), ('proportion_divergent', prop)):
        q = np.quantile(v, [0.05, 0.5, 0.95])
        for tag, x in zip(('q05', 'q50', 'q95'), q):
            stats['%s_%s' % (name, tag)] = float(x)
    return arrays, stats


def add_sample_summary(res, samples, l):
    """Fit result dict `res` (collect_fit_results) gains the summary of its posterior samples (K, N, M, 2), experiment order:
    the two agreement arrays next to `cn`, the six quantiles in `stats`."""
    arrays, stats = sample_summary(samples, res['cn'], l)
    res.update(arrays)
    res['stats'].update(stats)
    return res


SUMMARY_STATS = ('ploidy_q05', 'ploidy_q50', 'ploidy_q95', 'proportion_divergent_q05', 'proportion_divergent_q50', 'proportion_divergent_q95')
