"""numpy twin of the conditional marginals given a region event (rmx_region_conditional): a restricted forward-backward over
the dense framelogprob (N, S) / log_transmat (N - 1, S, S) of a RegionTwin in np.longdouble, log domain.  The mask is an
additive -inf on the emissions of the constrained segments of the evidence run, the label constraint -inf on the off-label
transitions of the run's adjacencies; the conditional marginal of a segment is the normalised product of the restricted
forward and backward rows, and log P(E) the restricted logZ - logZ of the chain.  Nothing here follows the device's recursion
(no forward rows of the device, no marginals, no backward kernel, no U)."""
import itertools

import numpy as np

from tests.region_twin import LD, NINF, _bwd, _fwd, _lse


def conditional(twin, a, b, lo, hi, mask=None, label=None, constrain=None):
    """(cond float64 (hi - lo + 1, S), log P(E)) for the event over [a, b] of tests.region_twin.RegionTwin `twin`: mask (N, S)
    bool, the allowed states of every segment; label (N, S) int; constrain (N,) bool or None (all).  cond is NaN where E cannot
    happen."""
    c = int(np.searchsorted(twin.ce, a, side='left'))
    c0, c1 = int(twin.cs[c]), int(twin.ce[c])
    assert c0 <= lo <= a <= b <= hi <= c1

    def emission(n):
        e = twin.f[n].copy()
        if a <= n <= b and mask is not None and (constrain is None or constrain[n]):
            e[~np.asarray(mask[n], dtype=bool)] = NINF
        return e

    def trans(n):
        E = twin.E[n]
        if a <= n < b and label is not None:
            E = np.where(np.asarray(label[n])[:, None] == np.asarray(label[n + 1])[None, :], E, LD(0))
        return E

    S = twin.f.shape[1]
    # restricted forward rows (emission of n included) from a on; the unrestricted ones before it
    F = dict((n, twin.la[n]) for n in range(lo, a))
    F[a] = emission(a) + (_fwd(twin.la[a - 1], twin.E[a - 1]) if a > c0 else 0)
    for n in range(a, hi):
        F[n + 1] = emission(n + 1) + _fwd(F[n], trans(n))
    # restricted backward rows (emission of n excluded) up to b; the unrestricted ones after it
    B = dict((n, twin.lb[n]) for n in range(b, hi + 1))
    for n in range(b - 1, lo - 1, -1):
        B[n] = _bwd(trans(n), emission(n + 1) + B[n + 1])
    logZ_E = _lse(F[b] + twin.lb[b])
    logp = float(logZ_E - twin.logZ[c])
    cond = np.full((hi - lo + 1, S), np.nan)
    if np.isfinite(logZ_E):
        for n in range(lo, hi + 1):
            v = F[n] + B[n]
            cond[n - lo] = np.exp(v - _lse(v)).astype(float)
    return cond, logp


def brute_force(framelogprob, log_transmat, a, b, mask=None, label=None, constrain=None):
    """The same by enumerating every path of one chain that spans all N segments: (cond (N, S), log P(E))."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    num = np.zeros((N, S), dtype=LD)
    den = tot = LD(0)
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        tot += w
        ok = True
        for n in range(a, b + 1):
            if mask is not None and (constrain is None or constrain[n]) and not mask[n][path[n]]:
                ok = False
        for n in range(a, b):
            if label is not None and label[n][path[n]] != label[n + 1][path[n + 1]]:
                ok = False
        if ok:
            den += w
            for n in range(N):
                num[n, path[n]] += w
    with np.errstate(divide='ignore', invalid='ignore'):
        return (num / den).astype(float), float(np.log(den / tot))
