"""CPU twin of the device's posterior path sampler (k_sample_cn): forward-filtering backward-sampling over a dense
framelogprob (N, S) / log_transmat (N-1, S, S), with the same Philox4x32-10 stream (key: the 64-bit restart seed,
counter (segment, sample, 0, 0), one 53-bit uniform per draw) and the same inverse-CDF rule in state order."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10_scalar(ctr, key):
    """Reference form on Python ints: ctr 4 words, key 2 words -> 4 words."""
    c = [int(x) & 0xFFFFFFFF for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for i in range(10):
        if i:
            k0 = (k0 + _PHILOX_W0) & 0xFFFFFFFF; k1 = (k1 + _PHILOX_W1) & 0xFFFFFFFF
        p0 = 0xD2511F53 * c[0]; p1 = 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
    return c


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised form: uint64 arrays holding 32-bit words (broadcast together)."""
    c0, c1, c2, c3 = [np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0 = np.asarray(k0, dtype=np.uint64) & M32; k1 = np.asarray(k1, dtype=np.uint64) & M32
    for i in range(10):
        if i:
            k0 = (k0 + np.uint64(_PHILOX_W0)) & M32; k1 = (k1 + np.uint64(_PHILOX_W1)) & M32
        p0 = _PHILOX_M0 * c0; p1 = _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0), p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1), p0 & M32
    return c0, c1, c2, c3


def uniform53_scalar(seed, sample, n):
    c = philox4x32_10_scalar([n, sample, 0, 0], [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF])
    return float(((c[0] >> 5) << 26) | (c[1] >> 6)) * 2.0 ** -53


def uniform53(seed, samples, n):
    """u of draw (sample, segment n) for an array of sample indices under one 64-bit seed."""
    seed = int(seed)
    samples = np.asarray(samples, dtype=np.uint64)
    c0, c1, _, _ = philox4x32_10(np.full(samples.shape, n, dtype=np.uint64), samples, 0, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return (((c0 >> np.uint64(5)) << np.uint64(26)) | (c1 >> np.uint64(6))).astype(np.float64) * 2.0 ** -53


def forward_log(framelogprob, log_transmat):
    f = np.asarray(framelogprob, dtype=float); T = np.asarray(log_transmat, dtype=float)
    la = np.empty_like(f)
    la[0] = f[0]
    for n in range(len(f) - 1):
        a = la[n][:, None] + T[n]
        mx = a.max(axis=0)
        la[n + 1] = mx + np.log(np.exp(a - mx).sum(axis=0)) + f[n + 1]
    return la


def sample(framelogprob, log_transmat, seed, samples, tol=1e-9):
    """(states (K, N) int64, flagged (K, N) bool): flagged where u lies within tol of a CDF boundary (the device may
    pick the neighbouring state there; what follows on that path depends on it)."""
    la = forward_log(framelogprob, log_transmat)
    T = np.asarray(log_transmat, dtype=float)
    N, S = la.shape
    samples = np.asarray(samples)
    K = len(samples)
    out = np.zeros((K, N), dtype=np.int64)
    flag = np.zeros((K, N), dtype=bool)
    nxt = None
    for n in range(N - 1, -1, -1):
        lw = np.broadcast_to(la[n], (K, S)) if nxt is None else la[n][None, :] + T[n][:, nxt].T
        w = np.exp(lw - lw.max(axis=1, keepdims=True))
        cdf = np.cumsum(w, axis=1)
        tot = cdf[:, -1:]
        u = uniform53(seed, samples, n)
        s = (cdf <= (u[:, None] * tot)).sum(axis=1)
        s = np.minimum(s, S - 1)
        flag[:, n] = (np.abs(cdf / tot - u[:, None]) < tol).any(axis=1)
        out[:, n] = s
        nxt = s
    return out, flag


def path_logprob(framelogprob, log_transmat, path):
    f = np.asarray(framelogprob); T = np.asarray(log_transmat)
    return f[np.arange(len(path)), path].sum() + sum(T[n, path[n], path[n + 1]] for n in range(len(path) - 1))
