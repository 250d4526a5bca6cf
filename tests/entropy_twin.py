"""numpy twin of the path entropy (rmx_path_entropy), on tests.region_twin.RegionTwin in np.longdouble and the log domain.  The
pairwise posterior of an adjacency is xi(s, s') = exp(la[n, s] + log E[n, s, s'] + f[n+1, s'] + lb[n+1, s'] - logZ) and the
marginal p(s') its column sum; H(c_n | c_n+1) = -sum xi log xi + sum p log p, H(c_n) = -sum p log p.  Nothing here follows the
device's formula: no backward kernel, no normaliser, no sums of fa log fa or W log W."""
import itertools

import numpy as np

from tests.region_twin import LD, RegionTwin


def _neg_xlogx_sum(logv):
    """-sum v log v from log v (an entry of -inf adds nothing)."""
    lv = np.asarray(logv, dtype=LD)
    ok = np.isfinite(lv)
    return -(np.exp(lv[ok]) * lv[ok]).sum()


def chain_of(twin, n):
    return int(np.searchsorted(twin.ce, n, side='left'))


def log_marginal(twin, n):
    return twin.la[n] + twin.lb[n] - twin.logZ[chain_of(twin, n)]


def marginal_entropy(twin, n):
    return _neg_xlogx_sum(log_marginal(twin, n))


def step_entropy(twin, n):
    """H(c_n | c_n+1); 0 where n ends a chain."""
    c = chain_of(twin, n)
    if n == twin.ce[c]:
        return LD(0)
    with np.errstate(divide='ignore'):
        lxi = twin.la[n][:, None] + np.log(twin.E[n]) + (twin.f[n + 1] + twin.lb[n + 1])[None, :] - twin.logZ[c]
    return _neg_xlogx_sum(lxi) - _neg_xlogx_sum(log_marginal(twin, n + 1))


def arrays(twin):
    """(marginal, step) over all segments of a tests.region_twin.RegionTwin, as the device call returns them."""
    N = twin.f.shape[0]
    return (np.array([marginal_entropy(twin, n) for n in range(N)], dtype=LD), np.array([step_entropy(twin, n) for n in range(N)], dtype=LD))


def run_entropy(marginal, step, a, b):
    """H(c_a .. c_b) of a run inside one chain from the twin's arrays, added up term by term in long double."""
    return marginal[b] + sum((step[n] for n in range(a, b)), LD(0))


def make(framelogprob, log_transmat, chain_start, chain_end):
    return RegionTwin(framelogprob, log_transmat, chain_start, chain_end)


def enumerate_joint(framelogprob, log_transmat):
    """The normalised joint of one chain that spans all N segments, as an array of shape (S,) * N."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    w = np.zeros((S,) * N, dtype=LD)
    for path in itertools.product(range(S), repeat=N):
        w[path] = np.exp(sum(f[n, path[n]] for n in range(N)) + sum((T[n, path[n], path[n + 1]] for n in range(N - 1)), LD(0)))
    return w / w.sum()


def joint_entropy(joint, keep):
    """The entropy of the segments `keep` (indices) under the enumerated joint: everything else summed out."""
    drop = tuple(i for i in range(joint.ndim) if i not in set(keep))
    p = joint.sum(axis=drop) if drop else joint
    p = p[p > 0]
    return -(p * np.log(p)).sum()
