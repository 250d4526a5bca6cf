"""numpy twin of rmx_posterior_summary on a dense (N, S) posterior: the projection through per-class weight tables,
the row maximum, entropy, gathered entry and arg-max, and the error scales the device comparison uses."""
import numpy as np


def project(post, weights, seg_class):
    """post (N, S), weights (C, S, Q), seg_class (N,) -> (N, Q)."""
    post = np.asarray(post); weights = np.asarray(weights); seg_class = np.asarray(seg_class)
    out = np.zeros((post.shape[0], weights.shape[2]))
    for c in np.unique(seg_class):
        sel = seg_class == c
        out[sel] = post[sel] @ weights[c]
    return out


def entropy_terms(post):
    """p log p where p > 0, else 0."""
    post = np.asarray(post, dtype=float)
    pos = post > 0
    return np.where(pos, post * np.log(np.where(pos, post, 1.)), 0.)


def summary(post, weights=None, seg_class=None, states=None):
    """(proj or None, stats (N, 3), argmax (N,)) as the entry point defines them."""
    post = np.asarray(post, dtype=float)
    N = post.shape[0]
    proj = None if weights is None else project(post, weights, np.zeros(N, dtype=int) if seg_class is None else seg_class)
    stats = np.zeros((N, 3))
    stats[:, 0] = post.max(axis=1)
    stats[:, 1] = -entropy_terms(post).sum(axis=1)
    if states is not None:
        stats[:, 2] = post[np.arange(N), np.asarray(states)]
    return proj, stats, post.argmax(axis=1)


def projection_scale(post, weights, seg_class):
    """|post| @ |weights|: the magnitude the rounding error of an S-term sum is relative to."""
    return project(np.abs(post), np.abs(weights), seg_class)


def entropy_scale(post):
    return np.abs(entropy_terms(post)).sum(axis=1)
