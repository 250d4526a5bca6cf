"""numpy twin of the region extremes (rmx_region_extremes): RegionTwin.logprob (np.longdouble, log domain) called once per
column with the column's own mask, mask and level <= j.  Nothing here follows the device's recursion: there is no shared
walk, no scale and no matrix product."""
import numpy as np

from tests import region_twin


def logcolumns(twin, a, b, ncol, level, mask=None, constrain=None):
    """level (N, S) int: the level of every state of every segment; mask (N, S) bool or None; constrain (N,) bool or None
    (every segment binds).  (ncol,) floats: column j = log P(in mask and level <= j at every constrained segment of [a, b])."""
    level = np.asarray(level)
    out = np.zeros(ncol)
    for j in range(ncol):
        m = level <= j
        if mask is not None:
            m = m & np.asarray(mask, dtype=bool)
        out[j] = twin.logprob(a, b, m, None, constrain)
    return out


def brute_force(framelogprob, log_transmat, a, b, ncol, level, mask=None, constrain=None):
    """The same columns by enumerating every path of one chain (region_twin.brute_force per column)."""
    level = np.asarray(level)
    out = np.zeros(ncol)
    for j in range(ncol):
        m = level <= j
        if mask is not None:
            m = m & np.asarray(mask, dtype=bool)
        out[j] = region_twin.brute_force(framelogprob, log_transmat, a, b, m, None, constrain)
    return out
