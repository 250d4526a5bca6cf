"""numpy twin of the region alternatives (rmx_region_kbest): decode_twin's log-domain np.longdouble Viterbi pass over a run with
a rank axis.  Every state keeps the K best partial paths that end in it; an entry is extended by every transition, and the K
best of a state's candidates -- ties to the lower (previous state, rank) -- go on.  The result is the K largest of the final
entries, ties to the lower (state, rank).  Different (previous state, rank) are different paths, so the K paths are pairwise
distinct.  Nothing here follows the device's recursion (it runs the other way, in the log domain, without normalisers).  The
log-probability of a given path is call_twin.logprob(twin, a, b, None, path)."""
import itertools

import numpy as np

from tests import decode_twin
from tests.region_twin import LD, NINF, _fwd


def kbest(twin, a, b, K, mask=None, label=None, constrain=None):
    """(logp float (K,), descending, -inf for a missing rank; paths: a list of K int arrays (b - a + 1,), None for a missing
    rank).  mask, label and constrain as decode_twin.decode."""
    c = int(np.searchsorted(twin.ce, a, side='left'))
    assert twin.cs[c] <= a <= b <= twin.ce[c] and K >= 1
    S = twin.f.shape[1]

    def emission(n):
        e = twin.f[n].copy()
        if mask is not None and (constrain is None or constrain[n]):
            e[~np.asarray(mask[n], dtype=bool)] = NINF
        return e

    v = np.full((S, K), NINF, dtype=LD)
    v[:, 0] = emission(a) + (_fwd(twin.la[a - 1], twin.E[a - 1]) if a > twin.cs[c] else 0)
    back = []
    for n in range(a, b):
        logE = decode_twin._log_transitions(twin, n)
        if label is not None:
            logE = np.where(np.asarray(label[n])[:, None] == np.asarray(label[n + 1])[None, :], logE, NINF)
        t = (v[:, :, None] + logE[:, None, :]).reshape(S * K, S)      # row s * K + j: ties to the lower (s, j)
        order = np.argsort(-t, axis=0, kind='stable')[:K]            # (K, s')
        top = np.take_along_axis(t, order, axis=0)
        back.append(np.where(np.isfinite(top), order, -1).T)        # (s', K)
        v = emission(n + 1)[:, None] + top.T
    end = (v + twin.lb[b][:, None]).reshape(S * K)
    order = np.argsort(-end, kind='stable')[:K]
    logp = np.full(K, -np.inf)
    paths = [None] * K
    for k, e in enumerate(order):
        if not np.isfinite(end[e]):
            break
        logp[k] = float(end[e] - twin.logZ[c])
        s, j = divmod(int(e), K)
        path = [s]
        for bp in reversed(back):
            s, j = divmod(int(bp[s, j]), K)
            path.append(s)
        paths[k] = np.array(path[::-1], dtype=np.int64)
    return logp, paths


def brute_force(framelogprob, log_transmat, a, b, K, mask=None, label=None, constrain=None):
    """The same list by enumerating every path of one chain that spans all N segments: the marginal of every configuration of
    the run, then the K largest over those that satisfy the event.  (logp (K,), -inf padded; the sorted list of (log marginal,
    configuration) over every configuration with positive probability)."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    den = LD(0)
    marg = {}
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        key = path[a:b + 1]
        marg[key] = marg.get(key, LD(0)) + w
    ok = sorted(((float(np.log(w / den)), k) for k, w in marg.items() if w > 0 and decode_twin.satisfies(k, a, b, mask, label, constrain)),
                key=lambda t: (-t[0], t[1]))
    logp = np.full(K, -np.inf)
    logp[:min(K, len(ok))] = [t[0] for t in ok[:K]]
    return logp, ok


class KbestTwinBatch(decode_twin.DecodeTwinBatch):
    """What posteriors.batch_region_alternatives needs of a RemixtBatch, answered by the twins."""

    def region_kbest_raw(self, r0, nr, queries, k, masks=None, labels=None, constrain=None, max_len=None):
        q = np.asarray(queries).reshape(-1, 4)
        self.calls.append(('region_kbest', nr, len(q), k))
        L = int((q[:, 1] - q[:, 0] + 1).max()) if max_len is None else int(max_len)
        logp = np.zeros((nr, len(q), k))
        states = np.full((nr, len(q), k, L), -1, dtype=np.int16)
        con = None if constrain is None else np.asarray(constrain) != 0
        for i in range(nr):
            for j, (a, b, mi, li) in enumerate(q):
                mk, lb = self._tables(mi, li, masks, labels)
                logp[i, j], paths = kbest(self.twins[r0 + i], a, b, k, mk, lb, con)
                for rank, path in enumerate(paths):
                    if path is not None:
                        states[i, j, rank, :len(path)] = path
        return logp, states
