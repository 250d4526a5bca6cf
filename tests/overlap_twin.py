"""numpy twin of the restart overlap (rmx_restart_overlap): log Z, Z = sum_x q_A(x_a .. x_b)^lam q_B(pi x_a .. pi x_b)^mu, from two
restarts' dense framelogprob (N, S) / log_transmat (N - 1, S, S) in np.longdouble, log domain.  Under either restart a
run of a chain has log q(x_a .. x_b) = forward row of a at x_a + the run's transitions and emissions + backward row of b
at x_b - log Z of the chain, so Z is one FORWARD pass over the run on the combined potentials lam * (A's) + mu * (B's, at
the permuted states).  Nothing here follows the device's recursion (no forward rows of the device, no marginals, no
backward kernel, no roots)."""
import itertools

import numpy as np

from tests.region_twin import LD, NINF, RegionTwin, _lse

MODES = {0: (LD(0.5), LD(0.5)), 1: (LD(1), LD(1))}


def _scaled(lam, v):
    """lam * v with -inf kept (v holds no +inf)"""
    return np.where(np.isneginf(v), NINF, lam * np.where(np.isneginf(v), LD(0), v))


class Side(RegionTwin):
    """One restart: the forward / backward rows of every chain (tests.region_twin.RegionTwin) and its log transitions."""

    def __init__(self, framelogprob, log_transmat, chain_start, chain_end):
        RegionTwin.__init__(self, framelogprob, log_transmat, chain_start, chain_end)
        self.T = np.asarray(log_transmat, dtype=LD)


class OverlapTwin(object):
    def __init__(self, side_a, side_b):
        self.A, self.B = side_a, side_b

    def logz_modes(self, a, b, perm_seg=None):
        """(log Z of mode 0, log Z of mode 1) of the run [a, b].  perm_seg (N, S) int: per segment, the state of B that a state
        of A is compared with (None: the identity).  The two modes share the gathers: mode 1's potentials are twice mode 0's."""
        A, B = self.A, self.B
        N, S = A.f.shape
        c = int(np.searchsorted(A.ce, a, side='left'))
        assert A.cs[c] <= a <= b <= A.ce[c]
        pi = np.tile(np.arange(S), (N, 1)) if perm_seg is None else np.asarray(perm_seg, dtype=np.int64)
        half = LD(0.5)
        v = [_scaled(half * k, A.la[a] + B.la[a][pi[a]]) for k in (1, 2)]
        for n in range(a, b):
            E1 = np.exp(_scaled(half, A.T[n] + B.T[n][pi[n]][:, pi[n + 1]]))
            emit = A.f[n + 1] + B.f[n + 1][pi[n + 1]]
            for k, E in ((0, E1), (1, E1 * E1)):
                m = v[k].max()
                if not np.isfinite(m):
                    v[k] = np.full(S, NINF)
                    continue
                with np.errstate(divide='ignore'):
                    v[k] = m + np.log(np.exp(v[k] - m) @ E) + _scaled(half * (k + 1), emit)
        out = []
        for k in (0, 1):
            lam = half * (k + 1)
            out.append(float(_lse(v[k] + _scaled(lam, A.lb[b] + B.lb[b][pi[b]])) - lam * (A.logZ[c] + B.logZ[c])))
        return tuple(out)

    def logz(self, a, b, mode, perm_seg=None):
        return self.logz_modes(a, b, perm_seg)[mode]


def build(frame_a, trans_a, frame_b, trans_b, chain_start, chain_end):
    A = Side(frame_a, trans_a, chain_start, chain_end)
    same = frame_b is frame_a and trans_b is trans_a
    return OverlapTwin(A, A if same else Side(frame_b, trans_b, chain_start, chain_end))


def _run_marginal(f, T, a, b):
    """{(x_a, .., x_b): probability} of one chain spanning all N segments, by enumerating every path"""
    f, T = np.asarray(f, dtype=LD), np.asarray(T, dtype=LD)
    N, S = f.shape
    out, den = {}, LD(0)
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        out[path[a:b + 1]] = out.get(path[a:b + 1], LD(0)) + w
    return dict((k, v / den) for k, v in out.items())


def brute_force(frame_a, trans_a, frame_b, trans_b, a, b, mode, perm_seg=None):
    """The same sum from the two run marginals, each by enumeration of every path."""
    lam, mu = MODES[mode]
    qa, qb = _run_marginal(frame_a, trans_a, a, b), _run_marginal(frame_b, trans_b, a, b)
    z = LD(0)
    for x, pa in qa.items():
        y = x if perm_seg is None else tuple(int(perm_seg[a + i][s]) for i, s in enumerate(x))
        pb = qb[y]
        if pa > 0 and pb > 0:
            z += pa ** lam * pb ** mu
    with np.errstate(divide='ignore'):
        return float(np.log(z))
