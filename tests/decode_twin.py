"""numpy twin of the region decode (rmx_region_decode), on top of region_twin.RegionTwin: the most probable configuration
of a run under the chain's posterior, in np.longdouble and the log domain on the dense framelogprob / log_transmat.  The
marginal of a run (c_a .. c_b) is exp(forward message into a + emissions + transitions of the run + backward message out
of b - logZ), so the maximum over the run is a Viterbi pass over the run alone that starts from emission(a) + the forward
message and ends with + lb[b] - logZ; the mask is -inf on the emissions of the constrained segments, the label constraint
-inf on the off-label transitions.  Nothing here follows the device's recursion (no forward rows of the device, no
marginals, no backward kernel, no normalisers).  The log-probability of a given path is call_twin.logprob(twin, a, b, None,
path)."""
import itertools

import numpy as np

from tests.region_twin import LD, NINF, _fwd


def _log_transitions(twin, n):
    """log of the twin's transition matrix of adjacency n, kept with the twin (a case decodes many runs over the same chain)."""
    cache = twin.__dict__.setdefault('_decode_logE', {})
    if n not in cache:
        with np.errstate(divide='ignore'):
            cache[n] = np.log(twin.E[n])
    return cache[n]


def decode(twin, a, b, mask=None, label=None, constrain=None):
    """(log P*, path int (b - a + 1,) or None when P* = 0): mask (N, S) bool, label (N, S) int, constrain (N,) bool or
    None (all), as RegionTwin.logprob takes them.  Ties go to the lowest state index."""
    c = int(np.searchsorted(twin.ce, a, side='left'))
    assert twin.cs[c] <= a <= b <= twin.ce[c]

    def emission(n):
        e = twin.f[n].copy()
        if mask is not None and (constrain is None or constrain[n]):
            e[~np.asarray(mask[n], dtype=bool)] = NINF
        return e

    v = emission(a) + (_fwd(twin.la[a - 1], twin.E[a - 1]) if a > twin.cs[c] else 0)
    back = []
    for n in range(a, b):
        logE = _log_transitions(twin, n)
        if label is not None:
            logE = np.where(np.asarray(label[n])[:, None] == np.asarray(label[n + 1])[None, :], logE, NINF)
        t = v[:, None] + logE                       # (s, s')
        back.append(np.argmax(t, axis=0))
        v = emission(n + 1) + t.max(axis=0)
    end = v + twin.lb[b]
    best = end.max()
    if not np.isfinite(best):
        return -np.inf, None
    path = [int(np.argmax(end))]
    for bp in reversed(back):
        path.append(int(bp[path[-1]]))
    return float(best - twin.logZ[c]), np.array(path[::-1], dtype=np.int64)


def satisfies(path, a, b, mask=None, label=None, constrain=None):
    """Whether the path (states of segments a .. b) satisfies the event exactly."""
    path = np.asarray(path)
    if len(path) != b - a + 1 or (path < 0).any():
        return False
    for k, n in enumerate(range(a, b + 1)):
        if mask is not None and (constrain is None or constrain[n]) and not mask[n][path[k]]:
            return False
        if label is not None and n < b and label[n][path[k]] != label[n + 1][path[k + 1]]:
            return False
    return True


def brute_force(framelogprob, log_transmat, a, b, mask=None, label=None, constrain=None):
    """The same maximum by enumerating every path of one chain that spans all N segments: the marginal of every
    configuration of the run, summed over the rest, then the maximum over those that satisfy the event.
    (log P*, the set of configurations within 1e-12 of it)."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    den = LD(0)
    marg = {}
    for path in itertools.product(range(S), repeat=N):
        w = np.exp(sum(f[n, path[n]] for n in range(N)) + sum(T[n, path[n], path[n + 1]] for n in range(N - 1)))
        den += w
        key = path[a:b + 1]
        marg[key] = marg.get(key, LD(0)) + w
    ok = dict((k, w) for k, w in marg.items() if satisfies(k, a, b, mask, label, constrain))
    best = max(ok.values()) if ok else LD(0)
    if not best > 0:
        return -np.inf, set()
    return float(np.log(best / den)), set(k for k, w in ok.items() if w >= best * (1 - LD(1e-12)))


class DecodeTwinBatch(object):
    """What posteriors.batch_region_calls needs of a RemixtBatch, answered by the twins: region_decode_raw here,
    region_logprob_raw and call_logprob_raw through RegionTwin / call_twin."""

    def __init__(self, cn_classes, seg_class, framelogprobs, log_transmats, chain_start, chain_end):
        from tests import region_twin
        self.cn_classes = np.asarray(cn_classes)
        self.seg_class = np.asarray(seg_class)
        self.num_segments, self.num_cn_states = np.asarray(framelogprobs[0]).shape
        self.twins = [region_twin.RegionTwin(f, T, chain_start, chain_end) for f, T in zip(framelogprobs, log_transmats)]
        self.calls = []

    def _tables(self, mi, li, masks, labels):
        mk = None if mi < 0 else np.asarray(masks)[self.seg_class, mi].astype(bool)
        lb = None if li < 0 else np.asarray(labels)[self.seg_class, li]
        return mk, lb

    def region_decode_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None, max_len=None):
        q = np.asarray(queries).reshape(-1, 4)
        self.calls.append(('region_decode', nr, len(q)))
        L = int((q[:, 1] - q[:, 0] + 1).max()) if max_len is None else int(max_len)
        logp = np.zeros((nr, len(q)))
        states = np.full((nr, len(q), L), -1, dtype=np.int16)
        con = None if constrain is None else np.asarray(constrain) != 0
        for i in range(nr):
            for j, (a, b, mi, li) in enumerate(q):
                mk, lb = self._tables(mi, li, masks, labels)
                logp[i, j], path = decode(self.twins[r0 + i], a, b, mk, lb, con)
                if path is not None:
                    states[i, j, :len(path)] = path
        return logp, states

    def region_logprob_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None):
        q = np.asarray(queries).reshape(-1, 4)
        self.calls.append(('region_logprob', nr, len(q)))
        con = None if constrain is None else np.asarray(constrain) != 0
        out = np.zeros((nr, len(q)))
        for i in range(nr):
            for j, (a, b, mi, li) in enumerate(q):
                mk, lb = self._tables(mi, li, masks, labels)
                out[i, j] = self.twins[r0 + i].logprob(a, b, mk, lb, con)
        return out

    def call_logprob_raw(self, r0, nr, paths, queries, labels=None, constrain=None):
        from tests import call_twin
        paths, q = np.asarray(paths), np.asarray(queries).reshape(-1, 4)
        self.calls.append(('call_logprob', nr, len(q)))
        con = None if constrain is None else np.asarray(constrain) != 0
        out = np.zeros((nr, len(q)))
        for i in range(nr):
            for j, (a, b, li, pi) in enumerate(q):
                lab = None if li < 0 else np.asarray(labels)[self.seg_class, li]
                out[i, j] = call_twin.logprob(self.twins[r0 + i], a, b, lab, paths[i, pi], con)
        return out
