"""numpy twin of the region event probabilities (rmx_region_prob): a restricted forward-backward over a dense
framelogprob (N, S) / log_transmat (N - 1, S, S) in np.longdouble, log domain.  log P(E) = restricted logZ - logZ of the
chain: the mask is an additive -inf on the emissions of the constrained segments of the run, the label constraint -inf
on the off-label transitions of the run's adjacencies.  Only the run itself is walked per query: the unrestricted
forward rows up to the run and backward rows after it are shared.  Nothing here follows the device's recursion (no
forward rows of the device, no marginals, no backward kernel)."""
import numpy as np

LD = np.longdouble
NINF = LD(-np.inf)


def _lse(v):
    m = v.max()
    if not np.isfinite(m):
        return NINF
    return m + np.log(np.exp(v - m).sum())


def _fwd(la, E):
    """log sum_i exp(la_i) E_ij"""
    m = la.max()
    if not np.isfinite(m):
        return np.full(E.shape[1], NINF)
    with np.errstate(divide='ignore'):
        return m + np.log(np.exp(la - m) @ E)


def _bwd(E, lv):
    """log sum_j E_ij exp(lv_j)"""
    m = lv.max()
    if not np.isfinite(m):
        return np.full(E.shape[0], NINF)
    with np.errstate(divide='ignore'):
        return m + np.log(E @ np.exp(lv - m))


class RegionTwin(object):
    def __init__(self, framelogprob, log_transmat, chain_start, chain_end):
        self.f = np.asarray(framelogprob, dtype=LD)
        self.E = np.exp(np.asarray(log_transmat, dtype=LD))
        self.cs, self.ce = np.asarray(chain_start), np.asarray(chain_end)
        N, S = self.f.shape
        self.la = np.full((N, S), NINF)      # log forward rows, emission of n included
        self.lb = np.full((N, S), NINF)      # log backward rows, emission of n excluded
        self.logZ = np.zeros(len(self.cs), dtype=LD)
        for c, (c0, c1) in enumerate(zip(self.cs, self.ce)):
            self.la[c0] = self.f[c0]
            for n in range(c0 + 1, c1 + 1):
                self.la[n] = self.f[n] + _fwd(self.la[n - 1], self.E[n - 1])
            self.lb[c1] = 0
            for n in range(c1 - 1, c0 - 1, -1):
                self.lb[n] = _bwd(self.E[n], self.f[n + 1] + self.lb[n + 1])
            self.logZ[c] = _lse(self.la[c1])

    def logprob(self, a, b, mask=None, label=None, constrain=None):
        """mask (N, S) bool: the allowed states of every segment; label (N, S) int; constrain (N,) bool or None (all)."""
        c = int(np.searchsorted(self.ce, a, side='left'))
        assert self.cs[c] <= a <= b <= self.ce[c]

        def emission(n):
            e = self.f[n].copy()
            if mask is not None and (constrain is None or constrain[n]):
                e[~np.asarray(mask[n], dtype=bool)] = NINF
            return e

        v = emission(a) + (_fwd(self.la[a - 1], self.E[a - 1]) if a > self.cs[c] else 0)
        for n in range(a, b):
            E = self.E[n]
            if label is not None:
                E = np.where(np.asarray(label[n])[:, None] == np.asarray(label[n + 1])[None, :], E, LD(0))
            v = emission(n + 1) + _fwd(v, E)
        return float(_lse(v + self.lb[b]) - self.logZ[c])


def brute_force(framelogprob, log_transmat, a, b, mask=None, label=None, constrain=None):
    """The same probability by enumerating every path of one chain that spans all N segments."""
    import itertools
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    num = den = LD(0)
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        ok = True
        for n in range(a, b + 1):
            if mask is not None and (constrain is None or constrain[n]) and not mask[n][path[n]]:
                ok = False
        for n in range(a, b):
            if label is not None and label[n][path[n]] != label[n + 1][path[n + 1]]:
                ok = False
        if ok:
            num += w
    with np.errstate(divide='ignore'):
        return float(np.log(num / den))
