"""numpy twin of the region event spans (rmx_region_span): RegionTwin.logprob asked once per interval [n0 - a, n0 + c] around
the anchor -- a restricted forward-backward in np.longdouble that does not follow the device's recursion -- and the device's
column recursion itself, with its per-column scaling, restated over dense fa / W / post to pin the formula."""
import numpy as np

from tests.region_twin import LD


def span(twin, n0, wl, wr, mask=None, label=None, constrain=None):
    """The table of a query (anchor n0, mask, label) with window (wl, wr): entry (a, c) holds log P(E on [n0 - a, n0 + c]),
    -inf where the interval leaves the anchor's chain or [0, N).  mask (N, S) bool, label (N, S) int, constrain (N,) as
    RegionTwin.logprob takes them."""
    c = int(np.searchsorted(twin.ce, n0, side='left'))
    c0, c1 = int(twin.cs[c]), int(twin.ce[c])
    out = np.full((wl + 1, wr + 1), -np.inf)
    for a in range(wl + 1):
        for k in range(wr + 1):
            if c0 <= n0 - a and n0 + k <= c1:
                out[a, k] = twin.logprob(n0 - a, n0 + k, mask, label, constrain)
    return out


def column_walk(fa, W, post, n0, wl, wr, mask=None, label=None, constrain=None):
    """The table of span() for one chain of N segments by the device's recursion: one column per right end j = n0 + c, started
    at segment j with g_j(s) = [s in A_j] post_j(s) and walked left with
      g_n(s) = [s in A_n] fa_n(s) sum_s' [label(s) == label(s')] W_n(s, s') g_n+1(s') / D_n(s'),   D_n(s') = sum_s fa_n(s) W_n(s, s');
    every column is divided by its own sum after every step and the logarithms are added; entry (n0 - n, j - n0) is the
    column's accumulator at n <= n0."""
    N, S = fa.shape

    def allowed(n):
        if mask is None or (constrain is not None and not constrain[n]):
            return np.ones(S, dtype=bool)
        return np.asarray(mask[n], dtype=bool)

    out = np.full((wl + 1, wr + 1), -np.inf)
    top, lo = min(n0 + wr, N - 1), max(n0 - wl, 0)
    G = np.zeros((S, wr + 1), dtype=LD)
    logacc = np.full(wr + 1, -np.inf, dtype=LD)
    for n in range(top, lo - 1, -1):
        if n < top:
            same = np.ones((S, S), dtype=bool) if label is None else np.asarray(label[n])[:, None] == np.asarray(label[n + 1])[None, :]
            D = (fa[n][:, None] * W[n]).sum(axis=0)
            H = np.where(G != 0, G / np.where(D > 0, D, 1)[:, None], LD(0))
            G = (allowed(n) * fa[n])[:, None] * ((W[n] * same) @ H)
            Z = G.sum(axis=0)
            live = Z > 0
            with np.errstate(divide='ignore'):
                logacc = np.where(live, logacc + np.log(np.where(live, Z, 1)), -np.inf)
            G = np.where(live[None, :], G / np.where(live, Z, 1)[None, :], LD(0))
        if n >= n0:
            g = allowed(n) * post[n]
            Z = g.sum()
            if Z > 0:
                G[:, n - n0] = g / Z
                logacc[n - n0] = np.log(Z)
        if n <= n0:
            out[n0 - n] = logacc.astype(float)
    return out
