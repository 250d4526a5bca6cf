"""numpy twin of the locus joints (rmx_locus_joint): the table log P(level_row(c_a) = i and level_col(c_t) = j) of two
segments a <= t of one chain, one region_twin.RegionTwin.logprob call per cell -- the restricted forward-backward in
np.longdouble over the run [a, t] with a per-segment mask that is `level_row == i` at a, `level_col == j` at t and all-true
between.  Nothing here follows the device's recursion (no columns, no backward kernel, no per-column scale)."""
import itertools

import numpy as np

LD = np.longdouble


def logtable(twin, a, t, nrow, ncol, level_row, level_col):
    """level_row, level_col: int (N, S), the levels of every segment's states.  (nrow, ncol) log-probabilities."""
    N, S = twin.f.shape
    level_row, level_col = np.asarray(level_row), np.asarray(level_col)
    out = np.zeros((nrow, ncol))
    for i in range(nrow):
        for j in range(ncol):
            mask = np.ones((N, S), dtype=bool)
            mask[a] &= level_row[a] == i
            mask[t] &= level_col[t] == j
            out[i, j] = twin.logprob(a, t, mask)
    return out


def brute_force(framelogprob, log_transmat, a, t, nrow, ncol, level_row, level_col):
    """The same table by enumerating every path of one chain that spans all N segments."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    num = np.zeros((nrow, ncol), dtype=LD)
    den = LD(0)
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        i, j = level_row[a][path[a]], level_col[t][path[t]]
        if i < nrow and j < ncol:
            num[i, j] += w
    with np.errstate(divide='ignore'):
        return np.log(num / den).astype(float)
