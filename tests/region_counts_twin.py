"""numpy twin of the region change counts (rmx_region_counts): RegionTwin's restricted forward pass over a dense
framelogprob (N, S) / log_transmat (N - 1, S, S) in np.longdouble, log domain, with a count axis.  The forward vector of
a run is (S, K): entry (s, k) is the log weight of the paths that end in s with k label changes so far (the last bin: K - 1
or more).  An on-label transition keeps the bin, an off-label one moves it up by one, the last bin keeping what it had.
Nothing here follows the device's recursion (no forward rows of the device, no marginals, no backward kernel)."""
import numpy as np

from tests.region_twin import LD, NINF, RegionTwin, _fwd, _lse


def _shift(v):
    """Forward vectors (S, K) moved up one bin, saturating in the last."""
    K = v.shape[1]
    if K == 1:
        return v.copy()
    out = np.full(v.shape, NINF)
    out[:, 1:] = v[:, :-1]
    out[:, K - 1] = np.logaddexp(v[:, K - 2], v[:, K - 1])
    return out


class CountsTwin(RegionTwin):
    @classmethod
    def sharing(cls, twin):
        """A CountsTwin on the forward / backward rows a RegionTwin has already computed."""
        self = cls.__new__(cls)
        self.__dict__.update(twin.__dict__)
        return self

    def logcounts(self, a, b, K, label, mask=None, constrain=None):
        """(K,) log P(mask holds on the run, and k label changes inside it); label (N, S) int, mask (N, S) bool or None,
        constrain (N,) bool or None (all)."""
        c = int(np.searchsorted(self.ce, a, side='left'))
        assert self.cs[c] <= a <= b <= self.ce[c]

        def emission(n):
            e = self.f[n].copy()
            if mask is not None and (constrain is None or constrain[n]):
                e[~np.asarray(mask[n], dtype=bool)] = NINF
            return e

        S = self.f.shape[1]
        v = np.full((S, K), NINF)
        v[:, 0] = emission(a) + (_fwd(self.la[a - 1], self.E[a - 1]) if a > self.cs[c] else 0)
        for n in range(a, b):
            same = np.asarray(label[n])[:, None] == np.asarray(label[n + 1])[None, :]
            on, off = np.where(same, self.E[n], LD(0)), np.where(same, LD(0), self.E[n])
            up = _shift(v)
            e = emission(n + 1)
            v = np.stack([e + np.logaddexp(_fwd(v[:, k], on), _fwd(up[:, k], off)) for k in range(K)], axis=1)
        return np.array([float(_lse(v[:, k] + self.lb[b]) - self.logZ[c]) for k in range(K)])


def brute_force_counts(framelogprob, log_transmat, a, b, K, label, mask=None, constrain=None):
    """The same (K,) log-probabilities by enumerating every path of one chain that spans all N segments."""
    import itertools
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    num, den = np.zeros(K, dtype=LD), LD(0)
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        if mask is not None and any((constrain is None or constrain[n]) and not mask[n][path[n]] for n in range(a, b + 1)):
            continue
        changes = sum(label[n][path[n]] != label[n + 1][path[n + 1]] for n in range(a, b))
        num[min(changes, K - 1)] += w
    with np.errstate(divide='ignore'):
        return np.log(num / den).astype(float)
