"""numpy twin of the region moments (rmx_region_moments) over RegionTwin's log forward / backward rows, in np.longdouble:
the mean and covariance of F_f = sum_{n in [a, b]} w_n phi_n,f(c_n) by the law of total covariance along the *forward*
conditionals of the chain,
  P(c_n+1 = s' | c_n = s) = E_n(s, s') exp(f_n+1(s') + lb_n+1(s') - lb_n(s)),
with m_n,f(s) = E[F_{n+1 .. b, f} | c_n = s] from a backward pass over those conditionals and
  Cov(F_f, F_g) = sum_n [ w_n^2 Cov_n(phi_f, phi_g) + w_n Cov_n(phi_f, m_n,g) + w_n Cov_n(phi_g, m_n,f) ],
every Cov_n under the marginal of segment n.  Nothing here follows the device's recursion: no backward kernel, no
centred columns, no second-moment column that is carried along the run."""
import itertools

import numpy as np

from tests.region_twin import LD


class MomentsTwin(object):
    def __init__(self, twin):
        """twin: a tests.region_twin.RegionTwin (its la, lb, f, E are read, nothing is recomputed)."""
        self.t = twin
        lp = twin.la + twin.lb
        m = lp.max(axis=1, keepdims=True)
        p = np.exp(lp - m)
        self.marg = p / p.sum(axis=1, keepdims=True)      # (N, S)
        self._cond = {}

    def _conditional(self, n):
        """P(c_n+1 = s' | c_n = s) (S, S); rows of states the chain cannot be in are 0."""
        if n not in self._cond:      # (queries share adjacencies)
            t = self.t
            lbn = t.lb[n]
            ok = np.isfinite(lbn)
            with np.errstate(invalid='ignore'):
                P = t.E[n] * np.exp((t.f[n + 1] + t.lb[n + 1])[None, :] - np.where(ok, lbn, LD(0))[:, None])
            self._cond[n] = np.where(ok[:, None], P, LD(0))
        return self._cond[n]

    def moments(self, a, b, feat, w):
        """feat (N, nf, S): the features of every segment under its own class table; w (N,) -> (mean (nf,), cov (nf, nf))."""
        t = self.t
        c = int(np.searchsorted(t.ce, a, side='left'))
        assert t.cs[c] <= a <= b <= t.ce[c]
        feat, w = np.asarray(feat, dtype=LD), np.asarray(w, dtype=LD)
        nf, S = feat.shape[1], feat.shape[2]
        m = np.zeros((nf, S), dtype=LD)                  # m_b = 0
        mean = np.zeros(nf, dtype=LD)
        cov = np.zeros((nf, nf), dtype=LD)

        def cov_n(p, x, y):
            return (p * x * y).sum() - (p * x).sum() * (p * y).sum()

        for n in range(b, a - 1, -1):
            if n < b:
                m = (w[n + 1] * feat[n + 1] + m) @ self._conditional(n).T      # m_n(s) = sum_s' P(s' | s) (w phi + m)_n+1(s')
            p = self.marg[n]
            mean += w[n] * (feat[n] * p).sum(axis=1)
            for f in range(nf):
                for g in range(nf):
                    cov[f, g] += w[n] * w[n] * cov_n(p, feat[n, f], feat[n, g]) + w[n] * cov_n(p, feat[n, f], m[g]) + w[n] * cov_n(p, feat[n, g], m[f])
        return mean.astype(float), cov.astype(float)


def brute_force(framelogprob, log_transmat, a, b, feat, w):
    """The same mean and covariance by enumerating every path of one chain that spans all N segments."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    feat, w = np.asarray(feat, dtype=LD), np.asarray(w, dtype=LD)
    N, S = f.shape
    nf = feat.shape[1]
    den = LD(0)
    s1 = np.zeros(nf, dtype=LD)
    s2 = np.zeros((nf, nf), dtype=LD)
    for path in itertools.product(range(S), repeat=N):
        pw = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        F = np.zeros(nf, dtype=LD)
        for n in range(a, b + 1):
            F += w[n] * feat[n, :, path[n]]
        den += pw
        s1 += pw * F
        s2 += pw * np.outer(F, F)
    mean = s1 / den
    return mean.astype(float), (s2 / den - np.outer(mean, mean)).astype(float)
