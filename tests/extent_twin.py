"""numpy twin of the region event extents (rmx_region_extent): RegionTwin.logprob asked once per nested interval around
the anchor -- a restricted forward-backward in np.longdouble that follows neither of the device's two recursions -- and
the right-walk recursion itself restated over dense fa / W / post, to pin the formula."""
import numpy as np

from tests.region_twin import LD


def extent(twin, n0, wl, wr, mask=None, label=None, constrain=None):
    """The row of a query (anchor n0, mask, label) with window (wl, wr): slot k stands for segment n = n0 - wl + k and holds
    log P(E on [min(n, n0), max(n, n0)]), -inf outside the anchor's chain or outside [0, N).  mask (N, S) bool, label (N, S)
    int, constrain (N,) as RegionTwin.logprob takes them."""
    c = int(np.searchsorted(twin.ce, n0, side='left'))
    c0, c1 = int(twin.cs[c]), int(twin.ce[c])
    out = np.full(wl + wr + 1, -np.inf)
    for k in range(wl + wr + 1):
        n = n0 - wl + k
        if c0 <= n <= c1:
            out[k] = twin.logprob(min(n, n0), max(n, n0), mask, label, constrain)
    return out


def dense_posterior(framelogprob, log_transmat):
    """(fa, W, post) of one chain, in np.longdouble: forward rows fa (N, S) (any per-row scale would do: the recursion is
    homogeneous in fa), weights W (N - 1, S, S) = exp(log_transmat) and marginals post (N, S)."""
    f, T = np.asarray(framelogprob, dtype=LD), np.asarray(log_transmat, dtype=LD)
    N, S = f.shape
    W = np.exp(T)
    fa = np.zeros((N, S), dtype=LD); fb = np.ones((N, S), dtype=LD)
    fa[0] = np.exp(f[0])
    for n in range(1, N):
        fa[n] = np.exp(f[n]) * (fa[n - 1] @ W[n - 1])
        fa[n] /= fa[n].sum()
    for n in range(N - 2, -1, -1):
        fb[n] = W[n] @ (np.exp(f[n + 1]) * fb[n + 1])
        fb[n] /= fb[n].sum()
    post = fa * fb
    post /= post.sum(axis=1, keepdims=True)
    return fa, W, post


def right_walk(fa, W, post, n0, wr, mask=None, label=None, constrain=None):
    """log P(E on [n0, n]) for n = n0 .. min(n0 + wr, N - 1) by the right-walk recursion: U_n0(s) = [s in A_n0],
    num(s') = sum_s [label(s) == label(s')] fa_n(s) W_n(s, s') U_n(s), D(s') = sum_s fa_n(s) W_n(s, s'),
    U_n+1(s') = [s' in A_n+1] num(s') / D(s'), P = sum_s' post_n+1(s') U_n+1(s') / sum_s' post_n+1(s')."""
    N, S = fa.shape

    def allowed(n):
        if mask is None or (constrain is not None and not constrain[n]):
            return np.ones(S, dtype=bool)
        return np.asarray(mask[n], dtype=bool)

    U = allowed(n0).astype(LD)
    out = [np.log((post[n0] * U).sum() / post[n0].sum())]
    for n in range(n0, min(n0 + wr, N - 1)):
        same = np.ones((S, S), dtype=bool) if label is None else np.asarray(label[n])[:, None] == np.asarray(label[n + 1])[None, :]
        num = ((fa[n] * U)[:, None] * W[n] * same).sum(axis=0)
        D = (fa[n][:, None] * W[n]).sum(axis=0)
        U = np.where(allowed(n + 1) & (num != 0), num / np.where(D > 0, D, 1), LD(0))
        with np.errstate(divide='ignore'):
            out.append(np.log((post[n + 1] * U).sum() / post[n + 1].sum()))
    return np.array(out, dtype=float)
