"""numpy twin of the region automata (rmx_region_automaton): log P(the automaton ends in q) for a deterministic finite
automaton that reads one symbol per read segment of a run [a, b] of one chain, FROM b DOWN TO a.  Log domain in np.longdouble
on region_twin.RegionTwin's forward rows la, backward rows lb, emissions f and transition weights E: a vector over (state,
automaton state) starts at b as f_b + lb_b in the column the first symbol leads to, takes one unrestricted step per adjacency
and is regrouped by delta at every read segment; the forward row into a closes it.  Nothing here follows the device's
recursion: no fa, no D, no backward kernel, no scale."""
import itertools

import numpy as np

from tests.region_twin import LD, NINF, _bwd, _fwd, _lse


def _regroup(u, sym_n, delta):
    """v(s, q) = log sum over the q' with delta[q', sym_n[s]] == q of exp(u(s, q'))"""
    S, Q = u.shape
    v = np.full((S, Q), NINF)
    rows = np.arange(S)
    for qp in range(Q):
        to = delta[qp, sym_n]
        v[rows, to] = np.logaddexp(v[rows, to], u[:, qp])
    return v


def logfinal(twin, a, b, sym, delta, start, constrain=None):
    """sym int (N, S): the symbol of every segment's states; delta int (Q, A); constrain (N,) bool or None (every segment is
    read).  (Q,) log-probabilities, -inf for a state that cannot be reached."""
    sym, delta = np.asarray(sym), np.asarray(delta, dtype=np.int64)
    Q = delta.shape[0]
    S = twin.f.shape[1]
    c = int(np.searchsorted(twin.ce, a, side='left'))
    assert twin.cs[c] <= a <= b <= twin.ce[c]

    def read(n):
        return constrain is None or bool(constrain[n])

    u = np.full((S, Q), NINF)
    u[:, start] = twin.f[b] + twin.lb[b]
    v = _regroup(u, sym[b], delta) if read(b) else u
    for n in range(b - 1, a - 1, -1):
        u = np.stack([twin.f[n] + _bwd(twin.E[n], v[:, q]) for q in range(Q)], axis=1)
        v = _regroup(u, sym[n], delta) if read(n) else u
    head = _fwd(twin.la[a - 1], twin.E[a - 1]) if a > twin.cs[c] else 0
    return np.array([float(_lse(v[:, q] + head) - twin.logZ[c]) for q in range(Q)])


def run_automaton(symbols, delta, start):
    """The final state after reading `symbols` in the order given."""
    q = int(start)
    for x in symbols:
        q = int(delta[q][x])
    return q


def brute_force(framelogprob, log_transmat, a, b, sym, delta, start, constrain=None):
    """The same distribution by enumerating every path of one chain that spans all N segments and running the automaton over
    each path's reversed symbol string (the read segments of b, b - 1, .. a)."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    Q = np.asarray(delta).shape[0]
    num = np.zeros(Q, dtype=LD)
    den = LD(0)
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        string = [sym[n][path[n]] for n in range(b, a - 1, -1) if constrain is None or constrain[n]]
        num[run_automaton(string, delta, start)] += w
    with np.errstate(divide='ignore'):
        return np.log(num / den).astype(float)
