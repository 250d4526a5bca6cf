"""MI355X-native `RemixtModel`: the object protocol of the reference's Cython
class `remixt.bpmodel.RemixtModel` (reference remixt/bpmodel.pyx:397-1210) on
top of the HIP C ABI (include/remixt_amd.h).

Two objects:

* `RemixtBatch` -- one dataset (segments, state tables, topology) resident in
  HBM with R independent restarts; coordinate updates and ELBOs run for any
  restart range in single launches.
* `RemixtModel` -- the drop-in per-model view.  Constructed with the
  reference's positional signature it owns a batch of one; `batch.model(r)`
  gives the same protocol on restart r of a shared batch.

State lives on the device.  Array attributes are copied to the host on read and
to the device on assignment (the reference hands out memoryviews of host
buffers; code that mutates a returned array in place must assign it back).
`log_transmat`, `cached_log_transmat` and `joint_posterior_marginals`
((N-1) x S x S) are never stored: they are materialised only when read.
"""
import ctypes as C

import numpy as np

from . import _lib

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)

RMX_EVALUE, RMX_EASSERT, RMX_EDEVICE, RMX_EUNSUPPORTED, RMX_EARG = 1, 2, 3, 4, 5

MAX_CLONES = 4      # RMX_MAX_CLONES (include/remixt_amd.h)
PARAM_IDS = {
    'negbin_r_0': 0, 'negbin_r_1': 1, 'negbin_hdel_mu': 2, 'negbin_hdel_r_0': 3, 'negbin_hdel_r_1': 4,
    'betabin_M_0': 5, 'betabin_M_1': 6, 'betabin_loh_p': 7, 'betabin_loh_M_0': 8, 'betabin_loh_M_1': 9,
    'prior_outlier_total': 10, 'prior_outlier_allele': 11, 'divergence_weight': 12, 'hmm_log_norm_const': 13,
}
ARRAY_IDS = {
    'h': 0, 'p_breakpoint': 1, 'p_allele_swap': 2, 'p_outlier_total': 3, 'p_outlier_allele': 4,
    'posterior_marginals': 5, 'framelogprob': 6, 'total_likelihood_mask': 7, 'allele_likelihood_mask': 8,
    'log_transmat': 9, 'cached_log_transmat': 10, 'joint_posterior_marginals': 11, 'state_sequence': 12,
}
_WRITABLE = {'h', 'p_breakpoint', 'p_allele_swap', 'p_outlier_total', 'p_outlier_allele', 'posterior_marginals',
             'total_likelihood_mask', 'allele_likelihood_mask'}
_STATE_TABLES = {'cn_states_total': 0, 'num_alleles_subclonal': 1, 'is_hdel': 2, 'is_loh': 3}


# enum rmx_option_id (include/remixt_amd.h)
OPTION_IDS = dict((n, i) for i, n in enumerate((
    'fb_kernel', 'fb_nv', 'fb_breakend_codes', 'fuse_sweeps', 'two_streams', 'viterbi_plain', 'search_mode', 'ell_dense', 'strip',
    'cell_cache', 'sparse_trial', 'fb_debug', 'pairwise_kernel', 'pace_sweeps', 'fb_wg_budget', 'trial_kernel', 'grad_kernel', 'stream_pool', 'viterbi_cluster', 'traceback', 'lt_classes')))


def set_default_option(name, value):
    """Process-wide default of a tuning option for batches created afterwards (tests and A/B measurements)."""
    lib = _lib.load()
    rc = lib.rmx_set_default_option(OPTION_IDS[name], int(value))
    if rc:
        _raise(lib, rc)


def last_error_restarts():
    """Restarts flagged by the calling thread's last failing call (rmx_last_error_restarts)."""
    lib = _lib.load()
    n = lib.rmx_last_error_restarts(None, 0)      # the count first: the list is as long as the batch has restarts
    if n <= 0:
        return []
    buf = (C.c_int32 * n)()
    n = min(n, lib.rmx_last_error_restarts(buf, n))
    return [int(buf[i]) for i in range(n)]


def _raise(lib, rc):
    msg = lib.rmx_last_error().decode()
    if rc == RMX_EVALUE:
        err = ValueError(msg)
        err.restarts = last_error_restarts()
        raise err
    if rc == RMX_EASSERT:
        err = AssertionError(msg)
        err.restarts = last_error_restarts()
        raise err
    if rc == RMX_EUNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == RMX_EARG:
        raise ValueError('bad argument: ' + msg)
    raise RuntimeError('HIP backend failure: ' + msg)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _class_weights(weights, num_classes, num_cn_states):
    """weights (C, S, Q), or (S, Q) for all classes alike, as a contiguous float64 (C, S, Q)."""
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim == 2:
        w = np.broadcast_to(w[None], (num_classes,) + w.shape)
    if w.ndim != 3 or w.shape[:2] != (num_classes, num_cn_states):
        raise ValueError('weights must have shape (num_classes, num_cn_states, Q) or (num_cn_states, Q)')
    return np.ascontiguousarray(w)


def _restart_states(states, rows, num_segments):
    """states int (rows, N), or (N,) with rows = 1, as a contiguous int16 array."""
    st = np.asarray(states)
    if st.shape != (rows, num_segments) and not (rows == 1 and st.shape == (num_segments,)):
        raise ValueError('states must have shape (nr, num_segments)')
    if st.size and (st.min() < -32768 or st.max() > 32767):
        raise ValueError('state index out of range')
    return np.ascontiguousarray(st, dtype=np.int16)


def _longest_query(q):
    """The default max_len of the decode calls: the longest run of queries q (nq, 4), within 1 .. 16384."""
    return int(np.clip((q[:, 1].astype(np.int64) - q[:, 0] + 1).max(), 1, 16384)) if q.shape[0] else 1


def compress_cn_states(cn_states, max_classes=64):
    """(N,S,M,2) int64 -> (classes (C,S,M,2), seg_class (N,) int32)."""
    lib = _lib.load()
    cn_states = _i64(cn_states)
    N, S, M, A = cn_states.shape
    if A != 2:
        raise ValueError('cn_states must have shape (num_segments, num_cn_states, num_clones, num_alleles)')
    seg_class = np.zeros(N, dtype=np.int32)
    classes = np.zeros((max_classes, S, M, 2), dtype=np.int64)
    nc = C.c_int32(0)
    rc = lib.rmx_compress_cn_states(cn_states.ctypes.data_as(_ip), N, S, M, max_classes,
                                    seg_class.ctypes.data_as(_i32p), classes.ctypes.data_as(_ip), C.byref(nc))
    if rc:
        _raise(lib, rc)
    return classes[:nc.value].copy(), seg_class


class RemixtBatch(object):
    """R restarts of one dataset on one GPU."""

    def __init__(self, num_clones, num_segments, num_breakpoints, normal_contamination,
                 cn_classes, seg_class, brk_states, h_init, l, x, y,
                 is_telomere, breakpoint_idx, breakpoint_orient, transition_penalty,
                 divergence_weight, device=0):
        self._lib = lib = _lib.load()
        self._handle = None
        cn_classes = _i64(cn_classes)
        if cn_classes.ndim != 4:
            raise ValueError('cn_classes must have shape (num_classes, num_cn_states, num_clones, 2)')
        brk_states = _i64(brk_states)
        seg_class = np.ascontiguousarray(seg_class, dtype=np.int32)
        h_init = np.atleast_2d(_f64(h_init))
        R = h_init.shape[0]
        divergence_weight = _f64(np.broadcast_to(np.asarray(divergence_weight, dtype=np.float64), (R,)))
        C_, S, M, A = cn_classes.shape
        # shape validation of bpmodel.pyx:509-529
        if M != num_clones or A != 2 or seg_class.shape[0] != num_segments:
            raise ValueError('cn_states must have shape (num_segments, num_cn_states, num_clones, num_alleles)')
        if brk_states.ndim != 2 or brk_states.shape[1] != num_clones:
            raise ValueError('cn_states must have shape (num_brk_states, num_clones)')
        if h_init.shape[1] != num_clones:
            raise ValueError('h must have length equal to num_clones')
        is_telomere = _i64(is_telomere); breakpoint_idx = _i64(breakpoint_idx); breakpoint_orient = _i64(breakpoint_orient)
        if is_telomere.shape[0] != num_segments:
            raise ValueError('is_telomere must have length equal to num_segments')
        if breakpoint_idx.shape[0] != num_segments:
            raise ValueError('breakpoint_idx must have length equal to num_segments')
        if breakpoint_orient.shape[0] != num_segments:
            raise ValueError('breakpoint_orient must have length equal to num_segments')
        l = _f64(l); x = _f64(x); y = _f64(y)
        if l.shape != (num_segments,) or x.shape != (num_segments,) or y.shape != (num_segments, 2):
            raise ValueError('l, x, y must have shapes (N,), (N,), (N, 2)')
        pr = _lib.RmxProblem()
        pr.num_clones = M; pr.num_segments = num_segments; pr.num_breakpoints = num_breakpoints
        pr.num_cn_states = S; pr.num_brk_states = brk_states.shape[0]; pr.num_classes = C_
        pr.normal_contamination = int(bool(normal_contamination))
        pr.cn_classes = cn_classes.ctypes.data_as(_ip); pr.seg_class = seg_class.ctypes.data_as(_i32p)
        pr.brk_states = brk_states.ctypes.data_as(_ip)
        pr.l = l.ctypes.data_as(_dp); pr.x = x.ctypes.data_as(_dp); pr.y = y.ctypes.data_as(_dp)
        pr.is_telomere = is_telomere.ctypes.data_as(_ip); pr.breakpoint_idx = breakpoint_idx.ctypes.data_as(_ip)
        pr.breakpoint_orient = breakpoint_orient.ctypes.data_as(_ip)
        pr.transition_penalty = float(transition_penalty)
        handle = C.c_void_p()
        rc = lib.rmx_batch_create(C.byref(pr), R, h_init.ctypes.data_as(_dp), divergence_weight.ctypes.data_as(_dp),
                                  int(device), C.byref(handle))
        if rc:
            _raise(lib, rc)
        self._handle = handle
        self.device = int(device)
        self.num_restarts = R
        self.num_clones = M
        self.num_segments = int(num_segments)
        self.num_breakpoints = int(num_breakpoints)
        self.num_cn_states = S
        self.num_brk_states = int(brk_states.shape[0])
        self.num_alleles = 2
        self.normal_contamination = bool(normal_contamination)
        self.transition_penalty = abs(float(transition_penalty))
        self.cn_classes = cn_classes
        self.seg_class = seg_class
        self.brk_states = brk_states
        self.is_telomere = is_telomere
        self.breakpoint_idx = breakpoint_idx
        self.breakpoint_orient = breakpoint_orient
        self.l = l; self.x = x; self.y = y
        self.cn_max = self.info(0)
        self._transition_model = 0
        self._samples = {}

    # -- lifetime ------------------------------------------------------------
    def close(self):
        if self._handle is not None:
            self._lib.rmx_batch_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            _raise(self._lib, rc)

    def info(self, what):
        out = C.c_int64(0)
        self._ck(self._lib.rmx_info(self._handle, what, C.byref(out)))
        return int(out.value)

    def synchronize(self):
        self._ck(self._lib.rmx_synchronize(self._handle))

    def set_option(self, name, value):
        """Tuning option of this batch (include/remixt_amd.h rmx_option_id): which equivalent kernel / launch shape runs."""
        self._ck(self._lib.rmx_set_option(self._handle, OPTION_IDS[name], int(value)))

    def get_option(self, name):
        out = C.c_int32(0)
        self._ck(self._lib.rmx_get_option(self._handle, OPTION_IDS[name], C.byref(out)))
        return int(out.value)

    def model(self, r):
        return RemixtModel._from_batch(self, r)

    # -- attributes ----------------------------------------------------------
    def array_shape(self, name):
        N, S, M, K, B = self.num_segments, self.num_cn_states, self.num_clones, self.num_breakpoints, self.num_brk_states
        return {
            'h': (M,), 'p_breakpoint': (K, B), 'p_allele_swap': (N, 2), 'p_outlier_total': (N, 2),
            'p_outlier_allele': (N, 2), 'posterior_marginals': (N, S), 'framelogprob': (N, S),
            'total_likelihood_mask': (N,), 'allele_likelihood_mask': (N,), 'log_transmat': (N - 1, S, S),
            'cached_log_transmat': (N - 1, S, S), 'joint_posterior_marginals': (N - 1, S, S), 'state_sequence': (N,),
        }[name]

    def get_array(self, r, name):
        shape = self.array_shape(name)
        dt = np.int64 if name in ('total_likelihood_mask', 'allele_likelihood_mask', 'state_sequence') else np.float64
        out = np.zeros(shape, dtype=dt)
        if out.size:
            self._ck(self._lib.rmx_get_array(self._handle, r, ARRAY_IDS[name], out.ctypes.data_as(C.c_void_p)))
        return out

    def fetch_indicators(self, r0=None, r1=None):
        """(p_outlier_total, p_outlier_allele) of restarts [r0, r1) as [r1 - r0][N][2] float64 arrays: views of pinned memory
        the batch owns, overwritten by the next call (rmx_fetch_indicators: two copies queued in order on the batch stream -- behind everything already queued there -- and waited for)."""
        r0, r1 = self._range(r0, r1)
        pt, pa = _dp(), _dp()
        self._ck(self._lib.rmx_fetch_indicators(self._handle, r0, r1, C.byref(pt), C.byref(pa)))
        shape = (r1 - r0, self.num_segments, 2)
        return np.ctypeslib.as_array(pt, shape=shape), np.ctypeslib.as_array(pa, shape=shape)

    def set_array(self, r, name, value):
        if name not in _WRITABLE:
            raise AttributeError('%s is read-only' % name)
        shape = self.array_shape(name)
        dt = np.int64 if name in ('total_likelihood_mask', 'allele_likelihood_mask') else np.float64
        v = np.ascontiguousarray(value, dtype=dt)
        if v.shape != shape:
            raise ValueError('%s must have shape %s' % (name, shape))
        if v.size:
            self._ck(self._lib.rmx_set_array(self._handle, r, ARRAY_IDS[name], v.ctypes.data_as(C.c_void_p)))

    def get_param(self, r, name):
        out = C.c_double(0.)
        self._ck(self._lib.rmx_get_param(self._handle, r, PARAM_IDS[name], C.byref(out)))
        return float(out.value)

    def set_param(self, r, name, value):
        self._ck(self._lib.rmx_set_param(self._handle, r, PARAM_IDS[name], float(value)))

    @property
    def transition_model(self):
        return self._transition_model

    @transition_model.setter
    def transition_model(self, value):
        self._ck(self._lib.rmx_set_transition_model(self._handle, int(value)))
        self._transition_model = int(value)

    def state_table(self, name):
        N, S, M = self.num_segments, self.num_cn_states, self.num_clones
        shape = (N, S, M) if name == 'cn_states_total' else (N, S)
        out = np.zeros(shape, dtype=np.int64)
        self._ck(self._lib.rmx_get_state_table(self._handle, _STATE_TABLES[name], out.ctypes.data_as(_ip)))
        return out

    # -- batched operations on restarts [r0, r1) -------------------------------
    def _range(self, r0, r1):
        if r0 is None:
            r0 = 0
        if r1 is None:
            r1 = self.num_restarts
        return int(r0), int(r1)

    def update_framelogprob(self, r0=None, r1=None):
        self._ck(self._lib.rmx_update_framelogprob(self._handle, *self._range(r0, r1)))

    def update_p_cn(self, r0=None, r1=None):
        self._ck(self._lib.rmx_update_p_cn(self._handle, *self._range(r0, r1)))

    def update_p_breakpoint(self, r0=None, r1=None):
        self._ck(self._lib.rmx_update_p_breakpoint(self._handle, *self._range(r0, r1)))

    def update_p_outlier_total(self, r0=None, r1=None):
        self._ck(self._lib.rmx_update_p_outlier_total(self._handle, *self._range(r0, r1)))

    def update_p_outlier_allele(self, r0=None, r1=None):
        self._ck(self._lib.rmx_update_p_outlier_allele(self._handle, *self._range(r0, r1)))

    def update_p_allele_swap(self, r0=None, r1=None):
        self._ck(self._lib.rmx_update_p_allele_swap(self._handle, *self._range(r0, r1)))

    def variational_update(self, iters=1, r0=None, r1=None):
        r0, r1 = self._range(r0, r1)
        self._ck(self._lib.rmx_variational_update(self._handle, r0, r1, int(iters)))

    def _scalar_range(self, fn, r0, r1):
        r0, r1 = self._range(r0, r1)
        out = np.zeros(r1 - r0, dtype=np.float64)
        self._ck(fn(self._handle, r0, r1, out.ctypes.data_as(_dp)))
        return out

    def calculate_elbo(self, r0=None, r1=None):
        return self._scalar_range(self._lib.rmx_calculate_elbo, r0, r1)

    def calculate_elbo_begin(self, r0=None, r1=None):
        """Queue the ELBO of restarts [r0, r1) without waiting (rmx_calculate_elbo_begin); calculate_elbo_end() returns the values."""
        r0, r1 = self._range(r0, r1)
        self._ck(self._lib.rmx_calculate_elbo_begin(self._handle, r0, r1))
        self._elbo_pending = r1 - r0

    def calculate_elbo_end(self):
        n = getattr(self, '_elbo_pending', 0)
        out = np.zeros(max(n, 1), dtype=np.float64)
        self._elbo_pending = 0
        self._ck(self._lib.rmx_calculate_elbo_end(self._handle, out.ctypes.data_as(_dp)))
        return out[:n]

    def calculate_variational_energy(self, r0=None, r1=None):
        return self._scalar_range(self._lib.rmx_calculate_variational_energy, r0, r1)

    def calculate_variational_entropy(self, r0=None, r1=None):
        return self._scalar_range(self._lib.rmx_calculate_variational_entropy, r0, r1)

    def _use_sample(self, r, sample):
        """Upload the sample mask unless it is the very array object last uploaded for this restart
        (the M-steps evaluate hundreds of times on one mask they never modify).  A caller that
        mutates a mask in place must pass a new array (or call invalidate_sample)."""
        if self._samples.get(r) is sample:
            return
        s64 = _i64(sample)
        if s64.shape != (self.num_segments,):
            raise ValueError('sample must have length num_segments')
        self._ck(self._lib.rmx_set_sample(self._handle, r, s64.ctypes.data_as(_ip)))
        self._samples[r] = sample

    def invalidate_sample(self, r=None):
        if r is None:
            self._samples.clear()
        else:
            self._samples.pop(r, None)

    def expected_log_likelihood(self, r, sample, want_grad=False):
        self._use_sample(r, sample)
        ell = C.c_double(0.)
        grad = np.zeros(self.num_clones, dtype=np.float64) if want_grad else None
        self._ck(self._lib.rmx_expected_log_likelihood(
            self._handle, r, None, C.byref(ell), grad.ctypes.data_as(_dp) if want_grad else None))
        return float(ell.value), grad

    def expected_log_likelihood_param_grid(self, r, name, values, sample):
        self._use_sample(r, sample)
        v = _f64(values).ravel()
        out = np.zeros(len(v), dtype=np.float64)
        self._ck(self._lib.rmx_expected_ll_param_grid(self._handle, r, PARAM_IDS[name], v.ctypes.data_as(_dp), len(v),
                                                      out.ctypes.data_as(_dp)))
        return out

    def expected_log_likelihood_batch(self, restarts, name, values):
        """E[ll] on each listed restart's current sample with likelihood parameter `name` set to the
        matching entry of `values` (and left there): the evaluation round of lock-step optimisers."""
        rl = np.ascontiguousarray(restarts, dtype=np.int32)
        v = _f64(values).ravel()
        if rl.shape != v.shape:
            raise ValueError('one value per listed restart')
        out = np.zeros(len(v), dtype=np.float64)
        self._ck(self._lib.rmx_expected_ll_batch(self._handle, len(v), rl.ctypes.data_as(_i32p), PARAM_IDS[name],
                                                 v.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out

    def param_search(self, restarts, name, lo, hi, grid):
        """scipy.optimize.brute over `grid` + Nelder-Mead polish of likelihood parameter `name` for all
        listed restarts in lock step (rmx_param_search); returns the optimum per restart."""
        rl = np.ascontiguousarray(restarts, dtype=np.int32)
        g = _f64(grid).ravel()
        out = np.zeros(len(rl), dtype=np.float64)
        self._ck(self._lib.rmx_param_search(self._handle, len(rl), rl.ctypes.data_as(_i32p), PARAM_IDS[name], float(lo), float(hi),
                                            g.ctypes.data_as(_dp), len(g), out.ctypes.data_as(_dp)))
        return out

    def set_sample_slot(self, r, slot, sample):
        """The M-step sample of restart r for parameter slot `slot` of param_search_multi."""
        s64 = _i64(sample)
        if s64.shape != (self.num_segments,):
            raise ValueError('sample must have length num_segments')
        self._ck(self._lib.rmx_set_sample_slot(self._handle, int(r), int(slot), s64.ctypes.data_as(_ip)))

    def set_sample_lists(self, entries):
        """M-step samples of several restarts in one call (rmx_set_sample_lists).  `entries`: (restart, slot, mask, indices) with
        slot -1 = the restart's current sample (what _use_sample uploads) or 0..3 = its parameter slot of param_search_multi;
        `indices` = np.flatnonzero(mask), `mask` the dense array the per-restart calls take (kept for _use_sample's identity test)."""
        if not entries:
            return
        rl = np.array([e[0] for e in entries], dtype=np.int32)
        sl = np.array([e[1] for e in entries], dtype=np.int32)
        idx = [np.ascontiguousarray(e[3], dtype=np.int32).ravel() for e in entries]
        off = np.zeros(len(entries) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(i) for i in idx])
        flat = np.concatenate(idx) if len(idx) else np.zeros(0, dtype=np.int32)
        flat = np.ascontiguousarray(flat, dtype=np.int32)
        self._ck(self._lib.rmx_set_sample_lists(self._handle, len(entries), rl.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p),
                                                off.ctypes.data_as(_i32p), flat.ctypes.data_as(_i32p)))
        for r, slot, mask, _ in entries:
            if slot < 0:
                self._samples[int(r)] = mask

    def param_search_multi(self, restarts, names, los, his, grids):
        """The searches of param_search for several of the four standard likelihood parameters at once
        (rmx_param_search_multi; samples from set_sample_slot, slot = position in `names`).  Returns
        (xopt, lastval), each [len(names)][len(restarts)]; the model is not modified.  Raises
        NotImplementedError when the request does not qualify -- fall back to param_search."""
        rl = np.ascontiguousarray(restarts, dtype=np.int32)
        ids = np.ascontiguousarray([PARAM_IDS[n] for n in names], dtype=np.int32)
        lo = _f64(los).ravel(); hi = _f64(his).ravel()
        g = _f64(grids)
        if g.ndim != 2 or g.shape[0] != len(ids) or len(lo) != len(ids) or len(hi) != len(ids):
            raise ValueError('one grid, lower and upper bound per parameter')
        xopt = np.zeros((len(ids), len(rl))); last = np.zeros((len(ids), len(rl)))
        self._ck(self._lib.rmx_param_search_multi(self._handle, len(rl), rl.ctypes.data_as(_i32p), len(ids), ids.ctypes.data_as(_i32p),
                                                  lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp), g.ctypes.data_as(_dp), g.shape[1],
                                                  xopt.ctypes.data_as(_dp), last.ctypes.data_as(_dp)))
        return xopt, last

    def expected_log_likelihood_h_batch(self, restarts, hs):
        """(E[ll], dE[ll]/dh) on each listed restart's current sample with h set to the matching row
        of `hs` (and left there): the evaluation round of the lock-step h M-step."""
        rl = np.ascontiguousarray(restarts, dtype=np.int32)
        h = _f64(hs).reshape(len(rl), self.num_clones)
        out = np.zeros((len(rl), 1 + MAX_CLONES), dtype=np.float64)
        self._ck(self._lib.rmx_expected_ll_h_batch(self._handle, len(rl), rl.ctypes.data_as(_i32p),
                                                   h.ctypes.data_as(_dp), out.ctypes.data_as(_dp)))
        return out[:, 0].copy(), out[:, 1:1 + self.num_clones].copy()

    def h_batch_evaluator(self, restarts):
        """`evaluate(ids, xs)` for lockstep.run_lockstep over the listed restarts: (-E[ll], -dE[ll]/dh) of restart restarts[ids[k]] at
        h = xs[k], through expected_log_likelihood_h_batch's entry point with the argument buffers and their ctypes views made once
        (a round of the lock-step h M-step is a few hundred microseconds; the generic wrapper's conversions were a quarter of it)."""
        live = [int(r) for r in restarts]
        n, M = len(live), self.num_clones
        rl = np.zeros(max(n, 1), dtype=np.int32)
        h = np.zeros((max(n, 1), M), dtype=np.float64)
        out = np.zeros((max(n, 1), 1 + MAX_CLONES), dtype=np.float64)
        p_rl, p_h, p_out = rl.ctypes.data_as(_i32p), h.ctypes.data_as(_dp), out.ctypes.data_as(_dp)
        fn, handle, lib = self._lib.rmx_expected_ll_h_batch, self._handle, self._lib

        neg = np.zeros((max(n, 1), 1 + MAX_CLONES), dtype=np.float64)

        def evaluate(ids, xs):
            """(-E[ll] (k,), -dE[ll]/dh (k, M)) at the rows of xs (a (k, M) array or a list of k vectors); the arrays are views
            of buffers the next call overwrites."""
            k = len(ids)
            for j in range(k):
                rl[j] = live[ids[j]]
            h[:k] = xs
            rc = fn(handle, k, p_rl, p_h, p_out)
            if rc:
                _raise(lib, rc)
            np.negative(out[:k], out=neg[:k])
            return neg[:k, 0], neg[:k, 1:1 + M]
        return evaluate

    def expected_log_likelihood_full(self, r0=None, r1=None):
        """E[ll] over all segments for restarts [r0, r1)."""
        return self._scalar_range(self._lib.rmx_expected_ll_full, r0, r1)

    def expected_log_likelihood_full_trial(self, r0=None, r1=None):
        """E[ll] over all segments at h / parameter values that are on trial (rmx_expected_ll_full_trial):
        nothing of the restarts' committed state changes; follow with set_param / set h (accept) or
        rollback_param / rollback_h (reject)."""
        return self._scalar_range(self._lib.rmx_expected_ll_full_trial, r0, r1)

    # component of E[ll] each of the four standard likelihood parameters moves (column of expected_log_likelihood_components)
    PARAM_COMPONENT = {'negbin_r_0': 0, 'negbin_r_1': 1, 'betabin_M_0': 2, 'betabin_M_1': 3}

    def expected_log_likelihood_components(self, r0=None, r1=None, trial=False):
        """[r1-r0][4]: E[ll] over all segments split into the components negbin_r_0, negbin_r_1, betabin_M_0, betabin_M_1 move,
        at the committed values or (trial=True) with changed parameters on trial (rmx_expected_ll_components); trial=2: from the
        scratch expectations the last trial pass left behind, without another pass."""
        r0, r1 = self._range(r0, r1)
        out = np.zeros((r1 - r0, 4), dtype=np.float64)
        self._ck(self._lib.rmx_expected_ll_components(self._handle, r0, r1, int(trial), out.ctypes.data_as(_dp)))
        return out

    def rollback_param(self, r, name, value):
        v = _f64([value])
        self._ck(self._lib.rmx_trial_rollback(self._handle, int(r), PARAM_IDS[name], v.ctypes.data_as(_dp)))

    def rollback_h(self, r, h):
        v = _f64(h).ravel()
        if len(v) != self.num_clones:
            raise ValueError('h must have one entry per clone')
        self._ck(self._lib.rmx_trial_rollback(self._handle, int(r), -1, v.ctypes.data_as(_dp)))

    def infer_cn(self, r):
        cn = np.zeros((self.num_segments, self.num_clones, 2), dtype=np.int64)
        lp = C.c_double(0.)
        self._ck(self._lib.rmx_infer_cn(self._handle, r, cn.ctypes.data_as(_ip), C.byref(lp)))
        return cn, float(lp.value)

    def infer_cn_batch(self, r0, nr):
        """Viterbi decode of restarts r0 .. r0+nr-1 in one call: (cn [nr][N][M][2], logprob [nr])."""
        cn = np.zeros((nr, self.num_segments, self.num_clones, 2), dtype=np.int64)
        lp = np.zeros(nr)
        self._ck(self._lib.rmx_infer_cn_batch(self._handle, int(r0), int(nr), cn.ctypes.data_as(_ip), lp.ctypes.data_as(_dp)))
        return cn, lp

    def sample_states(self, r0, nr, num_samples, seeds):
        """num_samples posterior paths of restarts r0 .. r0+nr-1 (forward-filtering backward-sampling over the
        structured posterior of their last update_p_cn): int16 (nr, num_samples, N) indices into each segment's state
        table.  seeds: nr 64-bit seeds, one stream per restart."""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        if len(seeds) != nr:
            raise ValueError('one seed per restart')
        out = np.zeros((max(int(nr), 0), max(int(num_samples), 0), self.num_segments), dtype=np.int16)
        self._ck(self._lib.rmx_sample_cn(self._handle, int(r0), int(nr), int(num_samples), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         out.ctypes.data_as(C.POINTER(C.c_int16))))
        return out

    def states_to_cn(self, states):
        """state indices (..., N) -> copy numbers int64 (..., N, M, 2) through the segments' class tables."""
        states = np.asarray(states)
        return self.cn_classes[self.seg_class, states]

    def posterior_summary_raw(self, r0, nr, weights=None, states=None, want_stats=True, want_argmax=True):
        """Linear functionals and row statistics of posterior_marginals of restarts r0 .. r0+nr-1 from one device pass
        (rmx_posterior_summary): (proj, stats, argmax), each None where not requested.  weights (C, S, Q), or (S, Q) for
        all classes alike, Q <= 256 -> proj (nr, N, Q) = marginals @ weights[seg_class]; stats (nr, N, 3): row maximum,
        entropy, marginal at states[r, n] (states: int (nr, N) or (N,) with nr = 1; 0 without); argmax int16 (nr, N):
        the first index of the row maximum."""
        r0, nr = int(r0), int(nr)
        N, S, C_ = self.num_segments, self.num_cn_states, self.cn_classes.shape[0]
        rows = max(nr, 0)
        Q, wp, proj = 0, _dp(), None
        if weights is not None:
            w = _class_weights(weights, C_, S)
            Q = w.shape[2]
            wbuf = w if w.size else np.zeros(1)      # (Q = 0 is the library's error to raise: a non-null pointer reaches it)
            wp = wbuf.ctypes.data_as(_dp)
            proj = np.zeros((rows, N, Q), dtype=np.float64)
            pbuf = proj if proj.size else np.zeros(1)
        i16p = C.POINTER(C.c_int16)
        sp = i16p()
        if states is not None:
            st = _restart_states(states, rows, N)
            sp = st.ctypes.data_as(i16p)
        stats = np.zeros((rows, N, 3), dtype=np.float64) if want_stats else None
        amax = np.zeros((rows, N), dtype=np.int16) if want_argmax else None
        self._ck(self._lib.rmx_posterior_summary(
            self._handle, r0, nr, Q, wp, sp, pbuf.ctypes.data_as(_dp) if proj is not None else _dp(),
            stats.ctypes.data_as(_dp) if stats is not None else _dp(), amax.ctypes.data_as(i16p) if amax is not None else i16p()))
        return proj, stats, amax

    def _region_args(self, queries, masks, labels, constrain):
        """The query and table arguments of rmx_region_prob / rmx_region_counts: (queries int32 (nq, 4), the C arguments
        nq, queries, nmask, masks, nlabel, labels, constrain, and the arrays those point into)."""
        N, S, C_ = self.num_segments, self.num_cn_states, self.cn_classes.shape[0]
        q = np.asarray(queries)
        if q.ndim != 2 or q.shape[1] != 4:
            raise ValueError('queries must have shape (nq, 4)')
        if q.size and (q.min() < -2 ** 31 or q.max() >= 2 ** 31):
            raise ValueError('query entry out of range')
        q = np.ascontiguousarray(q, dtype=np.int32)
        u8p, i16p = C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
        nmask, mp, nlabel, lp, cp = 0, u8p(), 0, i16p(), u8p()
        keep = []
        if masks is not None:
            mk = np.asarray(masks)
            if mk.ndim != 3 or mk.shape[0] != C_ or mk.shape[2] != S:
                raise ValueError('masks must have shape (num_classes, nmask, num_cn_states)')
            mk = np.ascontiguousarray(mk != 0, dtype=np.uint8)
            nmask = mk.shape[1]
            if nmask:
                mp = mk.ctypes.data_as(u8p)
                keep.append(mk)
        if labels is not None:
            lb = np.asarray(labels)
            if lb.ndim != 3 or lb.shape[0] != C_ or lb.shape[2] != S:
                raise ValueError('labels must have shape (num_classes, nlabel, num_cn_states)')
            if lb.size and (lb.min() < -32768 or lb.max() > 32767):
                raise ValueError('label out of the int16 range')
            lb = np.ascontiguousarray(lb, dtype=np.int16)
            nlabel = lb.shape[1]
            if nlabel:
                lp = lb.ctypes.data_as(i16p)
                keep.append(lb)
        if constrain is not None:
            cs = np.asarray(constrain)
            if cs.shape != (N,):
                raise ValueError('constrain must have shape (num_segments,)')
            cs = np.ascontiguousarray(cs != 0, dtype=np.uint8)
            cp = cs.ctypes.data_as(u8p)
            keep.append(cs)
        qbuf = q if q.size else np.zeros(4, dtype=np.int32)
        keep.append(qbuf)
        return q, (q.shape[0], qbuf.ctypes.data_as(C.POINTER(C.c_int32)), nmask, mp, nlabel, lp, cp), keep

    def region_logprob_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None):
        """log-probabilities (nr, nq) of path events over runs of model segments under the structured posterior of the
        last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_prob).  queries int (nq, 4): first segment, last segment
        (both of one chain), mask index or -1, label index or -1; masks (C, nmask, S), non-zero = allowed state; labels
        int (C, nlabel, S); constrain (N,), whether a mask binds at the segment (None: everywhere).  A query asks for
        log P(state in mask at every constrained segment of the run, and equal labels across every adjacency of the
        run); -inf for an impossible event."""
        r0, nr = int(r0), int(nr)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        out = np.zeros((max(nr, 0), q.shape[0]), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_region_prob(self._handle, r0, nr, *args, obuf.ctypes.data_as(_dp)))
        return out

    def region_counts_raw(self, r0, nr, queries, masks, labels, constrain, nbins):
        """log-probabilities (nr, nq, nbins) of the number of label changes over runs of model segments under the
        structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_counts).  queries, masks,
        labels and constrain as region_logprob_raw, but every query names a label.  Bin k of a query is
        log P(state in mask at every constrained segment of the run, and exactly k adjacencies of the run change the
        label); the last bin takes nbins - 1 changes or more; -inf for a bin that cannot happen (and for one below about
        1e-308 of the query's total).  nbins in 1 .. 16."""
        r0, nr, nbins = int(r0), int(nr), int(nbins)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        out = np.zeros((max(nr, 0), q.shape[0], max(nbins, 0)), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_region_counts(self._handle, r0, nr, *args, nbins, obuf.ctypes.data_as(_dp)))
        return out

    def region_extremes_raw(self, r0, nr, queries, masks, levels, constrain, ncol):
        """log-probabilities (nr, nq, ncol) that a per-state integer level stays at or below each of ncol nested
        thresholds over runs of model segments, under the structured posterior of the last update_p_cn of restarts
        r0 .. r0+nr-1 (rmx_region_extremes).  queries and masks as region_logprob_raw, but field 3 of a query is a level
        index; levels int (C, nlevel, S), every entry >= 0; constrain (N,), whether mask and level bind at the segment
        (None: everywhere).  Column j of a query is log P(state in mask and level(state) <= j at every constrained segment
        of the run); -inf for a column that cannot happen.  Every column has its own scale.  ncol in 1 .. 16."""
        r0, nr, ncol = int(r0), int(nr), int(ncol)
        q, args, _keep = self._region_args(queries, masks, levels, constrain)
        out = np.zeros((max(nr, 0), q.shape[0], max(ncol, 0)), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_region_extremes(self._handle, r0, nr, *args, ncol, obuf.ctypes.data_as(_dp)))
        return out

    def locus_joint_raw(self, r0, nr, queries, levels, nrow, ncol, nslot=0):
        """The exact joint posterior of two per-state integer levels at two model segments of one chain, under the structured
        posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_locus_joint).  queries int (nq, 4): segments a <= t,
        row level index, column level index; levels int (C, nlevel, S), every entry >= 0.  nslot = 0: (nr, nq, nrow, ncol),
        entry [i, j] = log P(level_row(c_a) = i and level_col(c_t) = j).  nslot >= 1: (nr, nq, nslot, nrow, ncol), slot k the
        same table of segment t - k against t for k = 0 .. t - a, NaN in the later slots.  A state whose level is >= nrow
        (>= ncol) is in no row (column); -inf for an empty cell.  nrow, ncol in 1 .. 16, nslot in 0 .. 4096."""
        r0, nr, nrow, ncol, nslot = int(r0), int(nr), int(nrow), int(ncol), int(nslot)
        q, args, _keep = self._region_args(queries, None, levels, None)
        ok = 1 <= nrow <= 16 and 1 <= ncol <= 16 and 0 <= nslot <= 4096
        shape = ((nslot,) if nslot >= 1 else ()) + (nrow, ncol)
        out = np.zeros((max(nr, 0), q.shape[0]) + (shape if ok else (1, 1)), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_locus_joint(self._handle, r0, nr, args[0], args[1], args[4], args[5], nrow, ncol, nslot, obuf.ctypes.data_as(_dp)))
        return out

    def region_automaton_raw(self, r0, nr, queries, symbols, delta, start, constrain=None):
        """The exact distribution of the final state of deterministic finite automata that read one symbol per segment of a
        run of model segments, under the structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1
        (rmx_region_automaton).  queries int (nq, 4): segments a <= b of one chain, symbol table index, automaton index;
        symbols int (C, nsym, S) with entries in [0, A); delta int (nauto, Q, A) with entries in [0, Q), delta[u, q, x] the
        state after reading symbol x in state q; start int (nauto,).  THE AUTOMATON READS A RUN FROM ITS LAST SEGMENT TO ITS
        FIRST; a segment with constrain[n] == 0 is not read (its state is marginalised, the automaton does not move).
        Returns (nr, nq, Q): log P(the automaton ends in state q), -inf for a state that cannot be reached.  Q, A in 1 .. 16,
        nauto in 1 .. 64."""
        r0, nr = int(r0), int(nr)
        q, args, _keep = self._region_args(queries, None, symbols, constrain)
        dl = np.asarray(delta)
        if dl.ndim != 3:
            raise ValueError('delta must have shape (nauto, Q, A)')
        if dl.size and (dl.min() < 0 or dl.max() > 255):
            raise ValueError('delta entry out of the uint8 range')
        dl = np.ascontiguousarray(dl, dtype=np.uint8)
        st = np.asarray(start)
        if st.shape != (dl.shape[0],):
            raise ValueError('start must have shape (nauto,)')
        if st.size and (st.min() < -2 ** 31 or st.max() >= 2 ** 31):
            raise ValueError('start entry out of range')
        st = np.ascontiguousarray(st, dtype=np.int32)
        nauto, Q, A = dl.shape
        out = np.zeros((max(nr, 0), q.shape[0], Q if 1 <= Q <= 16 else 1), dtype=np.float64)
        obuf, dbuf, sbuf = out if out.size else np.zeros(1), dl if dl.size else np.zeros(1, dtype=np.uint8), st if st.size else np.zeros(1, dtype=np.int32)
        self._ck(self._lib.rmx_region_automaton(self._handle, r0, nr, args[0], args[1], args[4], args[5], nauto, Q, A,
                                                dbuf.ctypes.data_as(C.POINTER(C.c_uint8)), sbuf.ctypes.data_as(C.POINTER(C.c_int32)), args[6],
                                                obuf.ctypes.data_as(_dp)))
        return out

    def region_sums_raw(self, r0, nr, queries, levels, weights, bins):
        """The exact distribution of sum_n w_n level(c_n) over runs of model segments, under the structured posterior of the
        last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_sums).  queries int (nq, 4): segments a <= b of one chain,
        level table index, offset o of the run's weights in the pool; levels int (C, nlevel, S), every entry >= 0 (a mask is
        a 0/1 table); weights int (nwt,), every entry >= 0: segment n of a run has weight weights[o + n - a], and 0 is "this
        segment does not count".  Returns (nr, nq, bins): log P(the sum == k), the last bin log P(the sum >= bins - 1); -inf
        for a value that cannot be reached.  Exact for these integer weights.  bins in 1 .. 64 and at most
        posteriors.sums_max_bins(num_cn_states)."""
        r0, nr, bins = int(r0), int(nr), int(bins)
        q, args, _keep = self._region_args(queries, None, levels, None)
        wt = np.asarray(weights)
        if wt.ndim != 1:
            raise ValueError('weights must have shape (nwt,)')
        if wt.size and (wt.min() < -2 ** 31 or wt.max() >= 2 ** 31):
            raise ValueError('weight out of the int32 range')
        wt = np.ascontiguousarray(wt, dtype=np.int32)
        out = np.zeros((max(nr, 0), q.shape[0], bins if 1 <= bins <= 64 else 1), dtype=np.float64)
        obuf, wbuf = out if out.size else np.zeros(1), wt if wt.size else np.zeros(1, dtype=np.int32)
        self._ck(self._lib.rmx_region_sums(self._handle, r0, nr, args[0], args[1], args[4], args[5], wt.shape[0],
                                           wbuf.ctypes.data_as(C.POINTER(C.c_int32)), bins, obuf.ctypes.data_as(_dp)))
        return out

    def path_entropy_raw(self, r0, nr, n0=0, n1=None):
        """The two arrays from which the entropy (nats) of the copy-number path posterior over any run of model segments
        follows, under the structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_path_entropy), for the
        model segments n0 .. n1-1 (n1 None: to the last): (marginal, step), (nr, n1 - n0) each.  marginal[n] = H(post_n);
        step[n] = H(c_n | c_n+1), +0.0 where segment n ends a chain.  H(c_a .. c_b) = marginal[b] + sum step[a .. b-1] inside
        one chain (posteriors.entropy_runs)."""
        r0, nr, n0 = int(r0), int(nr), int(n0)
        n1 = self.num_segments if n1 is None else int(n1)
        width = n1 - n0 if 0 <= n0 < n1 <= self.num_segments else 1
        marg = np.zeros((max(nr, 0), width), dtype=np.float64)
        step = np.zeros((max(nr, 0), width), dtype=np.float64)
        mbuf, sbuf = (marg, step) if marg.size else (np.zeros(1), np.zeros(1))
        self._ck(self._lib.rmx_path_entropy(self._handle, r0, nr, n0, n1, mbuf.ctypes.data_as(_dp), sbuf.ctypes.data_as(_dp)))
        return marg, step

    def restart_overlap_raw(self, other, pairs, queries, perms, mode):
        """log Z (npairs, nq) of the structured posteriors of pairs of restarts over runs of model segments
        (rmx_restart_overlap): Z = sum_x q_A(x)^lam q_B(pi x)^mu, mode 0 the Bhattacharyya overlap (lam = mu = 1/2), mode 1 the
        probability that independent draws coincide (lam = mu = 1).  other: the batch of the B side (None: this one; another
        batch must describe the same problem on the same device); pairs int (npairs, 2): restart of this batch, restart of
        `other`; queries int (nq, 4): first segment, last segment (both of one chain), permutation index, 0; perms int
        (nperm, C, S): per state class, the state of B that a state of A is compared with.  -inf where the two posteriors
        share no configuration."""
        other = self if other is None else other
        S, C_ = self.num_cn_states, self.cn_classes.shape[0]
        pr = np.asarray(pairs)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError('pairs must have shape (npairs, 2)')
        q = np.asarray(queries)
        if q.ndim != 2 or q.shape[1] != 4:
            raise ValueError('queries must have shape (nq, 4)')
        pm = np.asarray(perms)
        if pm.ndim != 3 or pm.shape[1] != C_ or pm.shape[2] != S:
            raise ValueError('perms must have shape (nperm, num_classes, num_cn_states)')
        for arr, name, lo, hi in ((pr, 'pair', -2 ** 31, 2 ** 31), (q, 'query', -2 ** 31, 2 ** 31), (pm, 'permutation', -32768, 32768)):
            if arr.size and (arr.min() < lo or arr.max() >= hi):
                raise ValueError('%s entry out of range' % name)
        pr, q, pm = (np.ascontiguousarray(pr, dtype=np.int32), np.ascontiguousarray(q, dtype=np.int32), np.ascontiguousarray(pm, dtype=np.int16))
        out = np.zeros((pr.shape[0], q.shape[0]), dtype=np.float64)
        i32p = C.POINTER(C.c_int32)
        bufs = [x if x.size else np.zeros(4, dtype=x.dtype) for x in (pr, q, pm, out)]
        self._ck(self._lib.rmx_restart_overlap(self._handle, other._handle, pr.shape[0], bufs[0].ctypes.data_as(i32p), q.shape[0],
                                               bufs[1].ctypes.data_as(i32p), pm.shape[0], bufs[2].ctypes.data_as(C.POINTER(C.c_int16)), int(mode),
                                               bufs[3].ctypes.data_as(_dp)))
        return out

    def call_logprob_raw(self, r0, nr, paths, queries, labels=None, constrain=None):
        """log-probabilities (nr, nq) that the copy-number path agrees with a reference path over runs of model segments,
        under the structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_call_prob).  paths int
        (nr, npaths, N): state indices into each segment's class table; queries int (nq, 4): first segment, last segment
        (both of one chain), label index or -1, path index; labels int (C, nlabel, S); constrain (N,), whether the event
        binds at the segment (None: everywhere).  A query asks for log P(label(state) == label(reference state) at every
        bound segment of the run), label -1 for the state itself; -inf for an impossible event."""
        r0, nr = int(r0), int(nr)
        q, args, _keep = self._region_args(queries, None, labels, constrain)
        nq, qp, _, _, nlabel, lp, cp = args
        pt = np.asarray(paths)
        if pt.ndim != 3 or pt.shape[0] != max(nr, 0) or pt.shape[2] != self.num_segments:
            raise ValueError('paths must have shape (nr, npaths, num_segments)')
        if pt.size and (pt.min() < -32768 or pt.max() > 32767):
            raise ValueError('state index out of range')
        pt = np.ascontiguousarray(pt, dtype=np.int16)
        pbuf = pt if pt.size else np.zeros(1, dtype=np.int16)
        out = np.zeros((max(nr, 0), q.shape[0]), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_call_prob(self._handle, r0, nr, pt.shape[1], pbuf.ctypes.data_as(C.POINTER(C.c_int16)), nq, qp, nlabel, lp, cp,
                                         obuf.ctypes.data_as(_dp)))
        return out

    def region_moments_raw(self, r0, nr, queries, features, weights, nf):
        """Exact means and covariances (nr, nq, nf + nf (nf + 1) / 2) of weighted sums of state features over runs of model
        segments, under the structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_moments).
        queries int (nq, 4): first segment, last segment (both of one chain), first feature f0, weight vector; features
        (C, nfeat, S) and weights (nw, N), finite doubles.  With F_f = sum over the run of weights[n] features[class of n,
        f0 + f, state of n] for f < nf, a query gives E[F_f] for every f, then Cov(F_f, F_g) for f <= g in row-major order
        of the upper triangle.  nf in 1 .. 4."""
        r0, nr, nf = int(r0), int(nr), int(nf)
        N, S, C_ = self.num_segments, self.num_cn_states, self.cn_classes.shape[0]
        q, args, _keep = self._region_args(queries, None, None, None)
        ft = np.ascontiguousarray(features, dtype=np.float64)
        if ft.ndim != 3 or ft.shape[0] != C_ or ft.shape[2] != S:
            raise ValueError('features must have shape (num_classes, nfeat, num_cn_states)')
        wt = np.ascontiguousarray(weights, dtype=np.float64)
        if wt.ndim != 2 or wt.shape[1] != N:
            raise ValueError('weights must have shape (nw, num_segments)')
        per = max(nf, 0) + max(nf, 0) * (max(nf, 0) + 1) // 2
        out = np.zeros((max(nr, 0), q.shape[0], per), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_region_moments(self._handle, r0, nr, args[0], args[1], ft.shape[1], ft.ctypes.data_as(_dp) if ft.size else _dp(),
                                              wt.shape[0], wt.ctypes.data_as(_dp) if wt.size else _dp(), nf, obuf.ctypes.data_as(_dp)))
        return out

    def region_extent_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None, wl=0, wr=0):
        """log-probabilities (nr, nq, wl + wr + 1) of where an event of region_logprob_raw begins and ends around an anchor,
        under the structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_extent).  queries int
        (nq, 4): anchor segment n0, mask index or -1, label index or -1, 0; masks, labels and constrain as
        region_logprob_raw.  Slot k of a query stands for model segment n = n0 - wl + k and holds the log-probability of
        the event over [min(n, n0), max(n, n0)]: slot wl is the event at the anchor alone, and both halves do not increase
        away from it.  -inf for a segment outside the anchor's chain (a run cannot pass a chain end) and for an impossible
        event.  wl, wr >= 0, wl + wr + 1 <= 4096."""
        r0, nr, wl, wr = int(r0), int(nr), int(wl), int(wr)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        if not (-2 ** 31 <= wl < 2 ** 31 and -2 ** 31 <= wr < 2 ** 31):
            raise ValueError('window width out of range')
        per = max(wl, 0) + max(wr, 0) + 1
        out = np.zeros((max(nr, 0), q.shape[0], per if per <= 4096 else 1), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_region_extent(self._handle, r0, nr, *args, wl, wr, obuf.ctypes.data_as(_dp)))
        return out

    def region_conditional_raw(self, r0, nr, queries, windows, masks, labels, constrain, weights, states=None):
        """Conditional marginals of the segments of a window given that an event of region_logprob_raw holds over an evidence run
        inside it, under the structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_conditional):
        (logp (nr, nq), out (nr, nq, nslot, Q + 3)).  queries int (nq, 4): the evidence run's first and last segment, mask
        index or -1, label index or -1; windows int (nq, 2): first and last segment that come back, around the run and in its
        chain; masks, labels and constrain as region_logprob_raw; weights (C, S, Q) or (S, Q), Q in 1 .. 64, as
        posterior_summary_raw; states int (nr, N) or (N,) with nr = 1, or None.  logp is log P(event).  Slot k of a query
        stands for model segment windows[i, 0] + k (nslot: the longest window) and holds the conditional marginal's projection
        on the Q weight columns, its maximum, the first index of the maximum and its entry at states[r, n] (0 without states);
        slots past the window are NaN, as is every slot of an impossible event (logp -inf).  A window holds at most 16 384
        segments, an evidence run at most 4 096."""
        r0, nr = int(r0), int(nr)
        N, S, C_ = self.num_segments, self.num_cn_states, self.cn_classes.shape[0]
        rows = max(nr, 0)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        wn = np.asarray(windows)
        if wn.shape != (q.shape[0], 2):
            raise ValueError('windows must have shape (nq, 2)')
        if wn.size and (wn.min() < -2 ** 31 or wn.max() >= 2 ** 31):
            raise ValueError('window entry out of range')
        wn = np.ascontiguousarray(wn, dtype=np.int32)
        nslot = int(np.clip((wn[:, 1].astype(np.int64) - wn[:, 0] + 1).max(), 1, 16384)) if wn.shape[0] else 1
        w = _class_weights(weights, C_, S)
        Q = w.shape[2]
        i16p, i32p = C.POINTER(C.c_int16), C.POINTER(C.c_int32)
        sp = i16p()
        if states is not None:
            st = _restart_states(states, rows, N)
            sp = st.ctypes.data_as(i16p)
        logp = np.zeros((rows, q.shape[0]), dtype=np.float64)
        out = np.zeros((rows, q.shape[0], nslot, (Q + 3) if 1 <= Q <= 64 else 1), dtype=np.float64)
        bufs = [x if x.size else np.zeros(4, dtype=x.dtype) for x in (wn, w, logp, out)]
        self._ck(self._lib.rmx_region_conditional(self._handle, r0, nr, args[0], args[1], bufs[0].ctypes.data_as(i32p), nslot, *args[2:], Q,
                                                  bufs[1].ctypes.data_as(_dp), sp, bufs[2].ctypes.data_as(_dp), bufs[3].ctypes.data_as(_dp)))
        return logp, out

    def region_span_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None, wl=0, wr=0):
        """log-probabilities (nr, nq, wl + 1, wr + 1) of an event of region_logprob_raw over every interval around an anchor,
        under the structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_span): the joint law of
        the event's two ends.  queries, masks, labels and constrain as region_extent_raw.  Entry (a, c) of a query with anchor
        n0 is the log-probability of the event over model segments [n0 - a, n0 + c]: entry (0, 0) is the event at the anchor
        alone, row 0 and column 0 are the two halves of region_extent_raw, and the table does not increase in a or in c.
        -inf for an interval that leaves the anchor's chain and for an impossible event.  wl, wr >= 0,
        (wl + 1) (wr + 1) <= 16384."""
        r0, nr, wl, wr = int(r0), int(nr), int(wl), int(wr)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        if not (-2 ** 31 <= wl < 2 ** 31 and -2 ** 31 <= wr < 2 ** 31):
            raise ValueError('window width out of range')
        ok = wl >= 0 and wr >= 0 and (wl + 1) * (wr + 1) <= 16384
        out = np.zeros((max(nr, 0), q.shape[0]) + ((wl + 1, wr + 1) if ok else (1, 1)), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_region_span(self._handle, r0, nr, *args, wl, wr, obuf.ctypes.data_as(_dp)))
        return out

    def region_pattern_raw(self, r0, nr, queries, pieces, masks=None, labels=None, constrain=None):
        """log-probabilities (nr, nq) of joint events over several runs of model segments of one chain, under the structured
        posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_pattern).  queries int (nq, 4): first piece,
        piece count, 0, 0; pieces int (npieces, 4): first segment, last segment, mask index or -1, label index or -1, each
        the event of region_logprob_raw over its run; the pieces of a query ascending, disjoint and in one chain.  masks,
        labels and constrain as region_logprob_raw.  A query asks for the log-probability that the events of all its pieces
        hold; nothing binds in the gaps, nor at the adjacency between two pieces, even where they touch.  -inf for an
        impossible event.  At most 4 194 304 pieces per call."""
        r0, nr = int(r0), int(nr)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        pc = np.asarray(pieces)
        if pc.ndim != 2 or pc.shape[1] != 4:
            raise ValueError('pieces must have shape (npieces, 4)')
        if pc.size and (pc.min() < -2 ** 31 or pc.max() >= 2 ** 31):
            raise ValueError('piece entry out of range')
        pc = np.ascontiguousarray(pc, dtype=np.int32)
        pbuf = pc if pc.size else np.zeros(4, dtype=np.int32)
        out = np.zeros((max(nr, 0), q.shape[0]), dtype=np.float64)
        obuf = out if out.size else np.zeros(1)
        self._ck(self._lib.rmx_region_pattern(self._handle, r0, nr, args[0], args[1], pc.shape[0], pbuf.ctypes.data_as(C.POINTER(C.c_int32)), *args[2:],
                                              obuf.ctypes.data_as(_dp)))
        return out

    def region_decode_raw(self, r0, nr, queries, masks=None, labels=None, constrain=None, max_len=None):
        """The most probable configuration of every query's run, and its log-probability, under the structured posterior of
        the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_decode): (logp (nr, nq), states int16 (nr, nq, max_len)).
        queries, masks, labels and constrain as region_logprob_raw; logp is the maximum, over the paths of the run that
        satisfy the query's event, of the run's marginal probability -- the sum of the same terms is region_logprob_raw --
        and states[r, i, k] the state of segment a + k of one path that attains it (ties to the lowest state index); entries
        past the run, and those of an impossible query (logp -inf), are -1.  max_len: 1 .. 16384 and at least the longest
        query; None: the longest query."""
        r0, nr = int(r0), int(nr)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        if max_len is None:
            max_len = _longest_query(q)
        max_len = int(max_len)
        out = np.zeros((max(nr, 0), q.shape[0]), dtype=np.float64)
        states = np.full((max(nr, 0), q.shape[0], max(max_len, 0)), -1, dtype=np.int16)
        obuf = out if out.size else np.zeros(1)
        sbuf = states if states.size else np.zeros(1, dtype=np.int16)
        self._ck(self._lib.rmx_region_decode(self._handle, r0, nr, *args, max_len, sbuf.ctypes.data_as(C.POINTER(C.c_int16)), obuf.ctypes.data_as(_dp)))
        return out, states

    def region_kbest_raw(self, r0, nr, queries, k, masks=None, labels=None, constrain=None, max_len=None):
        """The k most probable pairwise distinct configurations of every query's run, and their log-probabilities, under the
        structured posterior of the last update_p_cn of restarts r0 .. r0+nr-1 (rmx_region_kbest): (logp (nr, nq, k), states
        int16 (nr, nq, k, max_len)).  queries, masks, labels, constrain and max_len as region_decode_raw; 1 <= k <= 8.
        logp[r, i] does not increase along its ranks, rank 0 is region_decode_raw's result bit for bit, and ranks past the
        number of configurations with positive probability are -inf with states -1.  Ties: equal values keep the lower
        (next state, rank) first at every step, the final order is value descending, then state, then rank ascending."""
        r0, nr, k = int(r0), int(nr), int(k)
        q, args, _keep = self._region_args(queries, masks, labels, constrain)
        if not -2 ** 31 <= k < 2 ** 31:
            raise ValueError('k out of range')
        if max_len is None:
            max_len = _longest_query(q)
        max_len = int(max_len)
        kk = k if 1 <= k <= 8 else 1
        out = np.zeros((max(nr, 0), q.shape[0], kk), dtype=np.float64)
        states = np.full((max(nr, 0), q.shape[0], kk, max(max_len, 0)), -1, dtype=np.int16)
        obuf = out if out.size else np.zeros(1)
        sbuf = states if states.size else np.zeros(1, dtype=np.int16)
        self._ck(self._lib.rmx_region_kbest(self._handle, r0, nr, *args, k, max_len, sbuf.ctypes.data_as(C.POINTER(C.c_int16)), obuf.ctypes.data_as(_dp)))
        return out, states

    # -- measurement ------------------------------------------------------------
    def timer_start(self):
        self._ck(self._lib.rmx_timer_start(self._handle))

    def timer_stop(self):
        ms = C.c_double(0.)
        self._ck(self._lib.rmx_timer_stop(self._handle, C.byref(ms)))
        return float(ms.value)

    def profile_enable(self, on=True):
        self._ck(self._lib.rmx_profile_enable(self._handle, int(on)))    # 0 off, 1 all kernels, 2 sweep kernels only

    def profile_reset(self):
        self._ck(self._lib.rmx_profile_reset(self._handle))

    def profile(self):
        """{kernel name: (total_ms, launches)} since the last reset."""
        out = {}
        for i in range(self._lib.rmx_num_profile_ids()):
            ms = C.c_double(0.); n = C.c_int64(0)
            self._ck(self._lib.rmx_profile_get(self._handle, i, C.byref(ms), C.byref(n)))
            if n.value:
                out[self._lib.rmx_profile_name(i).decode()] = (float(ms.value), int(n.value))
        return out


class RemixtModel(object):
    """Drop-in for remixt.bpmodel.RemixtModel (bpmodel.pyx:397)."""

    _own = ('_batch', '_r', '_owns_batch')

    def __init__(self, num_clones, num_segments, num_breakpoints, normal_contamination,
                 cn_states, brk_states, h_init, l, x, y, is_telomere, breakpoint_idx,
                 breakpoint_orient, transition_penalty, divergence_weight, device=0):
        cn_states = np.asarray(cn_states)
        if cn_states.ndim != 4 or cn_states.shape[0] != num_segments or cn_states.shape[2] != num_clones or cn_states.shape[3] != 2:
            raise ValueError('cn_states must have shape (num_segments, num_cn_states, num_clones, num_alleles)')
        classes, seg_class = compress_cn_states(cn_states)
        batch = RemixtBatch(num_clones, num_segments, num_breakpoints, normal_contamination,
                            classes, seg_class, brk_states, np.asarray(h_init, dtype=np.float64)[None, :], l, x, y,
                            is_telomere, breakpoint_idx, breakpoint_orient, transition_penalty,
                            [float(divergence_weight)], device=device)
        object.__setattr__(self, '_batch', batch)
        object.__setattr__(self, '_r', 0)
        object.__setattr__(self, '_owns_batch', True)

    @classmethod
    def from_classes(cls, num_clones, num_segments, num_breakpoints, normal_contamination,
                     cn_classes, seg_class, brk_states, h_init, l, x, y, is_telomere, breakpoint_idx,
                     breakpoint_orient, transition_penalty, divergence_weight, device=0):
        """Same as the constructor with the state array given class-compressed
        (cn_classes (C,S,M,2), seg_class (N,)): avoids building the (N,S,M,2) array."""
        batch = RemixtBatch(num_clones, num_segments, num_breakpoints, normal_contamination,
                            cn_classes, seg_class, brk_states, np.asarray(h_init, dtype=np.float64)[None, :], l, x, y,
                            is_telomere, breakpoint_idx, breakpoint_orient, transition_penalty,
                            [float(divergence_weight)], device=device)
        self = cls.__new__(cls)
        object.__setattr__(self, '_batch', batch)
        object.__setattr__(self, '_r', 0)
        object.__setattr__(self, '_owns_batch', True)
        return self

    @classmethod
    def _from_batch(cls, batch, r):
        self = cls.__new__(cls)
        object.__setattr__(self, '_batch', batch)
        object.__setattr__(self, '_r', int(r))
        object.__setattr__(self, '_owns_batch', False)
        return self

    # -- attribute protocol ---------------------------------------------------------
    def __getattr__(self, name):
        b = object.__getattribute__(self, '_batch')
        r = object.__getattribute__(self, '_r')
        if name in ARRAY_IDS:
            return b.get_array(r, name)
        if name in PARAM_IDS:
            return b.get_param(r, name)
        if name in _STATE_TABLES:
            return b.state_table(name)
        if name == 'cn_states':
            return b.cn_classes[b.seg_class]
        if name in ('num_clones', 'num_segments', 'num_breakpoints', 'num_alleles', 'num_cn_states', 'num_brk_states',
                    'cn_max', 'normal_contamination', 'transition_penalty', 'transition_model', 'brk_states',
                    'is_telomere', 'breakpoint_idx', 'breakpoint_orient', 'l', 'x', 'y'):
            return getattr(b, name)
        if name == 'breakpoint_side':
            side = np.zeros(b.num_segments, dtype=np.int64)
            seen = np.zeros(max(b.num_breakpoints, 1), dtype=np.int64)
            for n in range(b.num_segments):
                k = b.breakpoint_idx[n]
                if k < 0:
                    continue
                side[n] = seen[k]
                seen[k] += 1
            return side
        raise AttributeError(name)

    def __setattr__(self, name, value):
        b = object.__getattribute__(self, '_batch')
        r = object.__getattribute__(self, '_r')
        if name in ARRAY_IDS:
            b.set_array(r, name, value)
        elif name in PARAM_IDS:
            if name == 'hmm_log_norm_const':
                raise AttributeError('hmm_log_norm_const is read-only')
            b.set_param(r, name, value)
        elif name == 'transition_model':
            b.transition_model = value
        else:
            raise AttributeError('cannot set attribute %r' % name)

    def __dir__(self):
        return sorted(set(list(ARRAY_IDS) + list(PARAM_IDS) + list(_STATE_TABLES) + [
            'cn_states', 'num_clones', 'num_segments', 'num_breakpoints', 'num_alleles', 'num_cn_states',
            'num_brk_states', 'cn_max', 'normal_contamination', 'transition_penalty', 'transition_model',
            'brk_states', 'is_telomere', 'breakpoint_idx', 'breakpoint_orient', 'breakpoint_side', 'l', 'x', 'y']))

    # -- methods (cpdef surface of bpmodel.pyx) ----------------------------------------
    def update_framelogprob(self):
        self._batch.update_framelogprob(self._r, self._r + 1)

    def update_p_cn(self):
        self._batch.update_p_cn(self._r, self._r + 1)

    def update_p_breakpoint(self):
        self._batch.update_p_breakpoint(self._r, self._r + 1)

    def update_p_outlier_total(self):
        self._batch.update_p_outlier_total(self._r, self._r + 1)

    def update_p_outlier_allele(self):
        self._batch.update_p_outlier_allele(self._r, self._r + 1)

    def update_p_allele_swap(self):
        self._batch.update_p_allele_swap(self._r, self._r + 1)

    def calculate_elbo(self):
        return float(self._batch.calculate_elbo(self._r, self._r + 1)[0])

    def calculate_variational_energy(self):
        return float(self._batch.calculate_variational_energy(self._r, self._r + 1)[0])

    def calculate_variational_entropy(self):
        return float(self._batch.calculate_variational_entropy(self._r, self._r + 1)[0])

    def calculate_expected_log_likelihood(self, sample):
        return self._batch.expected_log_likelihood(self._r, sample)[0]

    def calculate_expected_log_likelihood_param_grid(self, name, values, sample):
        """E[ll] for each value of the likelihood parameter `name` (left at values[-1]), one round trip."""
        return self._batch.expected_log_likelihood_param_grid(self._r, name, values, sample)

    def calculate_expected_log_likelihood_partial_h(self, sample, partial_h):
        _, g = self._batch.expected_log_likelihood(self._r, sample, want_grad=True)
        partial_h[:] = g

    def calculate_log_transmat(self, log_transmat):
        """bpmodel.pyx:639-684 with the *current* p_breakpoint, into the caller's (N-1, S, S) array."""
        b = self._batch
        out = np.ascontiguousarray(log_transmat, dtype=np.float64)
        if out.shape != (b.num_segments - 1, b.num_cn_states, b.num_cn_states):
            raise ValueError('log_transmat must have shape (num_segments - 1, num_cn_states, num_cn_states)')
        b._ck(b._lib.rmx_calculate_log_transmat(b._handle, self._r, out.ctypes.data_as(_dp)))
        if out is not log_transmat:
            np.asarray(log_transmat)[...] = out

    def calculate_log_likelihood_total(self, n, s, u):
        out = C.c_double(0.)
        b = self._batch
        b._ck(b._lib.rmx_log_likelihood_total(b._handle, self._r, int(n), int(s), int(u), C.byref(out)))
        return float(out.value)

    def calculate_log_likelihood_allele(self, n, s, v, w):
        out = C.c_double(0.)
        b = self._batch
        b._ck(b._lib.rmx_log_likelihood_allele(b._handle, self._r, int(n), int(s), int(v), int(w), C.byref(out)))
        return float(out.value)

    # the remaining per-cell cpdef methods (bpmodel.pyx:686-749, 778-807, 855-896); partial_h is the caller's (M,) array
    def _cell(self, which, n, s, u=0, v=0, w=0):
        b = self._batch
        if not (0 <= int(n) < b.num_segments and 0 <= int(s) < b.num_cn_states):
            raise IndexError('segment / state index out of range')       # the reference's bounds-checked memoryviews
        out = np.zeros(MAX_CLONES)
        b._ck(b._lib.rmx_cell_quantity(b._handle, self._r, int(n), int(s), which, int(u), int(v), int(w), out.ctypes.data_as(_dp)))
        return out

    def calculate_expected_total_reads(self, n, s):
        return float(self._cell(0, n, s)[0])

    def calculate_expected_total_reads_partial_h(self, n, s, partial_h):
        partial_h[:] = self._cell(1, n, s)[:self._batch.num_clones]

    def calculate_expected_allele_ratio(self, n, s):
        return float(self._cell(2, n, s)[0])

    def calculate_expected_allele_ratio_partial_h(self, n, s, partial_h):
        partial_h[:] = self._cell(3, n, s)[:self._batch.num_clones]

    def calculate_log_prior_cn(self, n, s):
        return float(self._cell(4, n, s)[0])

    def calculate_log_likelihood_total_partial_h(self, n, s, u, partial_h):
        partial_h[:] = self._cell(5, n, s, u=u)[:self._batch.num_clones]

    def calculate_log_likelihood_allele_partial_h(self, n, s, v, w, partial_h):
        partial_h[:] = self._cell(6, n, s, v=v, w=w)[:self._batch.num_clones]

    def infer_cn(self, cn):
        out, _ = self._batch.infer_cn(self._r)
        cn[...] = out

    def sample_cn(self, num_samples, seed):
        """num_samples posterior copy-number paths (K, N, M, 2) int64 of this model (seed: 64-bit)."""
        states = self._batch.sample_states(self._r, 1, num_samples, [seed])[0]
        return self._batch.states_to_cn(states)

    def posterior_summary_raw(self, weights=None, states=None, want_stats=True, want_argmax=True):
        """RemixtBatch.posterior_summary_raw of this model: (proj (N, Q), stats (N, 3), argmax (N,)), None where not requested."""
        out = self._batch.posterior_summary_raw(self._r, 1, weights=weights, states=states, want_stats=want_stats, want_argmax=want_argmax)
        return tuple(None if a is None else a[0] for a in out)

    def region_logprob(self, queries, masks=None, labels=None, constrain=None):
        """RemixtBatch.region_logprob_raw of this model: log-probabilities (nq,)."""
        return self._batch.region_logprob_raw(self._r, 1, queries, masks, labels, constrain)[0]

    def region_counts(self, queries, masks, labels, constrain, nbins):
        """RemixtBatch.region_counts_raw of this model: log-probabilities (nq, nbins)."""
        return self._batch.region_counts_raw(self._r, 1, queries, masks, labels, constrain, nbins)[0]

    def region_extremes(self, queries, masks, levels, constrain, ncol):
        """RemixtBatch.region_extremes_raw of this model: log-probabilities (nq, ncol)."""
        return self._batch.region_extremes_raw(self._r, 1, queries, masks, levels, constrain, ncol)[0]

    def locus_joint(self, queries, levels, nrow, ncol, nslot=0):
        """RemixtBatch.locus_joint_raw of this model: log-probabilities (nq, nrow, ncol), or (nq, nslot, nrow, ncol)."""
        return self._batch.locus_joint_raw(self._r, 1, queries, levels, nrow, ncol, nslot)[0]

    def region_automaton(self, queries, symbols, delta, start, constrain=None):
        """RemixtBatch.region_automaton_raw of this model: log-probabilities (nq, Q)."""
        return self._batch.region_automaton_raw(self._r, 1, queries, symbols, delta, start, constrain)[0]

    def region_sums(self, queries, levels, weights, bins):
        """RemixtBatch.region_sums_raw of this model: log-probabilities (nq, bins)."""
        return self._batch.region_sums_raw(self._r, 1, queries, levels, weights, bins)[0]

    def path_entropy(self, n0=0, n1=None):
        """RemixtBatch.path_entropy_raw of this model: (marginal, step), (n1 - n0,) each."""
        marg, step = self._batch.path_entropy_raw(self._r, 1, n0, n1)
        return marg[0], step[0]

    def region_moments(self, queries, features, weights, nf):
        """RemixtBatch.region_moments_raw of this model: means and covariances (nq, nf + nf (nf + 1) / 2)."""
        return self._batch.region_moments_raw(self._r, 1, queries, features, weights, nf)[0]

    def region_extent(self, queries, masks=None, labels=None, constrain=None, wl=0, wr=0):
        """RemixtBatch.region_extent_raw of this model: log-probabilities (nq, wl + wr + 1)."""
        return self._batch.region_extent_raw(self._r, 1, queries, masks, labels, constrain, wl, wr)[0]

    def region_conditional(self, queries, windows, masks, labels, constrain, weights, states=None):
        """RemixtBatch.region_conditional_raw of this model: (logp (nq,), out (nq, nslot, Q + 3))."""
        logp, out = self._batch.region_conditional_raw(self._r, 1, queries, windows, masks, labels, constrain, weights, states)
        return logp[0], out[0]

    def region_span(self, queries, masks=None, labels=None, constrain=None, wl=0, wr=0):
        """RemixtBatch.region_span_raw of this model: log-probabilities (nq, wl + 1, wr + 1)."""
        return self._batch.region_span_raw(self._r, 1, queries, masks, labels, constrain, wl, wr)[0]

    def region_pattern(self, queries, pieces, masks=None, labels=None, constrain=None):
        """RemixtBatch.region_pattern_raw of this model: log-probabilities (nq,)."""
        return self._batch.region_pattern_raw(self._r, 1, queries, pieces, masks, labels, constrain)[0]

    def region_kbest(self, queries, k, masks=None, labels=None, constrain=None, max_len=None):
        """RemixtBatch.region_kbest_raw of this model: (logp (nq, k), states int16 (nq, k, max_len))."""
        logp, states = self._batch.region_kbest_raw(self._r, 1, queries, k, masks, labels, constrain, max_len)
        return logp[0], states[0]

    def region_decode(self, queries, masks=None, labels=None, constrain=None, max_len=None):
        """RemixtBatch.region_decode_raw of this model: (logp (nq,), states int16 (nq, max_len))."""
        logp, states = self._batch.region_decode_raw(self._r, 1, queries, masks, labels, constrain, max_len)
        return logp[0], states[0]

    def call_logprob(self, paths, queries, labels=None, constrain=None):
        """RemixtBatch.call_logprob_raw of this model: paths (npaths, N) -> log-probabilities (nq,)."""
        return self._batch.call_logprob_raw(self._r, 1, np.asarray(paths)[None], queries, labels, constrain)[0]

    def posterior_project(self, weights):
        """posterior_marginals @ weights[class of the segment] -> (N, Q), on the device: weights (C, S, Q) or (S, Q), Q <= 256."""
        return self.posterior_summary_raw(weights=weights, want_stats=False, want_argmax=False)[0]


def sum_product(framelogprob, log_transmat, alphas, betas, device=0):
    """bpmodel.pyx:1213-1246 on caller-supplied dense inputs (HIP)."""
    lib = _lib.load()
    f = _f64(framelogprob); T = _f64(log_transmat)
    N, S = f.shape
    if T.shape != (N - 1, S, S):
        raise ValueError('log_transmat must have shape (N-1, S, S)')
    a = np.zeros_like(f); b = np.zeros_like(f)
    Tp = T if T.size else np.zeros(1)
    rc = lib.rmx_sum_product(f.ctypes.data_as(_dp), Tp.ctypes.data_as(_dp), a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), N, S, device)
    if rc:
        _raise(lib, rc)
    alphas[...] = a
    betas[...] = b


def max_product(framelogprob, log_transmat, state_sequence, device=0):
    """bpmodel.pyx:1296-1333 on caller-supplied dense inputs (HIP); returns the log probability."""
    lib = _lib.load()
    f = _f64(framelogprob); T = _f64(log_transmat)
    N, S = f.shape
    if T.shape != (N - 1, S, S):
        raise ValueError('log_transmat must have shape (N-1, S, S)')
    ss = np.zeros(N, dtype=np.int64)
    lp = C.c_double(0.)
    Tp = T if T.size else np.zeros(1)
    rc = lib.rmx_max_product(f.ctypes.data_as(_dp), Tp.ctypes.data_as(_dp), ss.ctypes.data_as(_ip), C.byref(lp), N, S, device)
    if rc:
        _raise(lib, rc)
    state_sequence[...] = ss
    return float(lp.value)
