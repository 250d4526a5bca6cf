"""numpy twin of the region sums (rmx_region_sums): log P(sum_n w_n level_n(c_n) == k) over a run [a, b] of one chain, the last
of the B bins meaning B - 1 or more.  Log domain in np.longdouble on region_twin.RegionTwin's forward rows la, backward rows
lb, emissions f and transition weights E: a vector over (state, sum) starts at b as f_b + lb_b in the column of the first
increment, takes one unrestricted step per adjacency and is shifted by every segment's increments, what passes the last bin
added to it; the forward row into a closes it.  Nothing here follows the device's recursion: no fa, no D, no backward
kernel, no scale."""
import itertools

import numpy as np

from tests.region_twin import LD, NINF, _bwd, _fwd, _lse


def _shift(u, inc):
    """v(s, min(k + inc[s], B - 1)) = log sum exp(u(s, k))"""
    S, B = u.shape
    v = np.full((S, B), NINF)
    rows = np.arange(S)
    for k in range(B):
        to = np.minimum(k + inc, B - 1)
        v[rows, to] = np.logaddexp(v[rows, to], u[:, k])
    return v


def logsums(twin, a, b, level, weights, bins):
    """level int (N, S): the level of every segment's states; weights: w_a .. w_b (python ints: no overflow); (bins,)
    log-probabilities, -inf for a value that cannot be reached."""
    level = np.asarray(level)
    B = int(bins)
    S = twin.f.shape[1]
    c = int(np.searchsorted(twin.ce, a, side='left'))
    assert twin.cs[c] <= a <= b <= twin.ce[c] and len(weights) == b - a + 1

    def inc(n):
        w = int(weights[n - a])
        return np.array([min(w * int(x), B - 1) for x in level[n]], dtype=np.int64)

    u = np.full((S, B), NINF)
    u[:, 0] = twin.f[b] + twin.lb[b]
    v = _shift(u, inc(b))
    for n in range(b - 1, a - 1, -1):
        u = np.stack([twin.f[n] + _bwd(twin.E[n], v[:, k]) for k in range(B)], axis=1)
        v = _shift(u, inc(n))
    head = _fwd(twin.la[a - 1], twin.E[a - 1]) if a > twin.cs[c] else 0
    return np.array([float(_lse(v[:, k] + head) - twin.logZ[c]) for k in range(B)])


def brute_force(framelogprob, log_transmat, a, b, level, weights, bins):
    """The same distribution by enumerating every path of one chain that spans all N segments."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    B = int(bins)
    num = np.zeros(B, dtype=LD)
    den = LD(0)
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        total = sum(int(weights[n - a]) * int(level[n][path[n]]) for n in range(a, b + 1))
        num[min(total, B - 1)] += w
    with np.errstate(divide='ignore'):
        return np.log(num / den).astype(float)
