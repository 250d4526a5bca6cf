"""numpy twin of the call probabilities (rmx_call_prob), on top of region_twin.RegionTwin: the event "the path agrees
with a reference path, up to a label, at every bound segment of a run" is a per-segment state mask,
mask[n] = (label_seg[n] == label_seg[n, ref_n]), handed to the twin's restricted forward-backward in np.longdouble.
Nothing here follows the device's recursion."""
import numpy as np

from tests import region_twin


def call_mask(label_seg, ref, S):
    """(N, S) bool: the allowed states of every segment.  label_seg (N, S) int, or None for the state itself."""
    ref = np.asarray(ref, dtype=np.int64)
    N = len(ref)
    lab = np.tile(np.arange(S), (N, 1)) if label_seg is None else np.asarray(label_seg)
    return lab == lab[np.arange(N), ref][:, None]


def logprob(twin, a, b, label_seg, ref, constrain=None):
    """log P(label(c_n) == label(ref_n) at every n in [a, b] with constrain[n]) under the chain of `twin`."""
    return twin.logprob(a, b, call_mask(label_seg, ref, twin.f.shape[1]), None, constrain)


class TwinBatch(object):
    """What posteriors.batch_call_confidence / batch_cn_logprob need of a RemixtBatch, answered by the twin: one dense
    (framelogprob, log_transmat) per restart."""

    def __init__(self, cn_classes, seg_class, framelogprobs, log_transmats, chain_start, chain_end):
        self.cn_classes = np.asarray(cn_classes)
        self.seg_class = np.asarray(seg_class)
        self.num_segments, self.num_cn_states = np.asarray(framelogprobs[0]).shape
        self.twins = [region_twin.RegionTwin(f, T, chain_start, chain_end) for f, T in zip(framelogprobs, log_transmats)]
        self.calls = []      # (nr, npaths, nq) of every call

    def call_logprob_raw(self, r0, nr, paths, queries, labels=None, constrain=None):
        paths, queries = np.asarray(paths), np.asarray(queries).reshape(-1, 4)
        assert paths.shape[0] == nr and paths.shape[2] == self.num_segments
        self.calls.append((nr, paths.shape[1], len(queries)))
        out = np.zeros((nr, len(queries)))
        for i in range(nr):
            for j, (a, b, li, pi) in enumerate(queries):
                lab = None if li < 0 else np.asarray(labels)[self.seg_class, li]
                out[i, j] = logprob(self.twins[r0 + i], a, b, lab, paths[i, pi], None if constrain is None else np.asarray(constrain) != 0)
        return out
