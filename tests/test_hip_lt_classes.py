"""GPU: the cell cache with its read-depth planes kept per (segment, total-copy class) -- option lt_classes = 1, the
default -- against its twin with six planes per (segment, state), lt_classes = 0.  The two read-depth values of a cell
depend on the state through its total copy numbers alone, so both forms hold the same values and every sum takes them in
the same order: everything the library returns must be the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARRAYS = ('posterior_marginals', 'p_outlier_total', 'p_outlier_allele', 'p_allele_swap', 'p_breakpoint')


def _both(fn):
    """fn() under lt_classes = 1 and = 0 (a creation-time option: the process-wide default while the model is built)"""
    from remixt_amd import bpmodel
    outs = []
    try:
        for v in (1, 0):
            bpmodel.set_default_option('lt_classes', v)
            outs.append(fn(v))
    finally:
        bpmodel.set_default_option('lt_classes', 1)
    return outs


def _same(a, b, what=''):
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (what, i))
    elif isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            _same(a[k], b[k], '%s[%r]' % (what, k))
    else:
        assert np.array_equal(np.asarray(a), np.asarray(b)), what


def _sweeps(N, clones, max_cn, R, states, classes, options=None, chains=4, seed=11, masks=False, h_of=None, **model_kw):
    from remixt_amd import synthetic
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(N, num_clones=clones, max_copy_number=max_cn, num_chains=chains, seed=seed)
    ps = synthetic.make_init_params(e, R, max_cn, num_clones=clones)
    hs = [h_of(p) for p in ps] if h_of else None

    def run(v):
        rs = RestartSet(e, ps, max_copy_number=max_cn, num_clones=clones, quiet=True, options=options, h_init=hs, **model_kw)
        b = rs.batch
        assert b.num_cn_states == states and b.get_option('lt_classes') == v
        assert (classes is None or b.info(64) == classes) and b.info(65) == v
        if masks:
            mt = np.ones(b.num_segments, dtype=np.int64); mt[::3] = 0
            ma = np.ones(b.num_segments, dtype=np.int64); ma[::5] = 0
            for r in range(R):
                b.set_array(r, 'total_likelihood_mask', mt)
                b.set_array(r, 'allele_likelihood_mask', ma)
        b.variational_update(3)
        out = [b.calculate_elbo()] + [[b.get_array(r, a) for r in range(R)] for a in ARRAYS]
        rs.close()
        return out
    one, zero = _both(run)
    assert np.isfinite(np.asarray(one[0])).all()
    _same(one, zero)


@pytest.mark.parametrize('fuse', [1, 0])
def test_165_states_with_breakends(fuse):
    """700 segments, 3 clones, max_cn 8: 165 states (3 per lane), 39 classes; the fused marginal pass, and with fuse_sweeps = 0
    the separate frame / marginal passes and the stand-alone indicator kernels."""
    _sweeps(700, 3, 8, 3, 165, 39, options=None if fuse else {'fuse_sweeps': 0})


def test_165_states_through_two_em_iterations():
    """The refresh passes of every component mask behind accepted parameters and h, and the trial / rollback path next to a
    compact cache."""
    from remixt_amd import synthetic
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(700, num_clones=3, max_copy_number=8, num_chains=4, seed=11)
    ps = synthetic.make_init_params(e, 3, 8)

    def run(v):
        rs = RestartSet(e, ps, max_copy_number=8, num_clones=3, quiet=True, seeds=[5, 6, 7], mstep_threads=1)
        assert rs.batch.info(65) == v
        rs.fit(num_em_iter=2, num_update_iter=2)
        out = [(m.prev_elbo, np.array(m.h), m.get_likelihood_param_values()) for m in rs.models]
        rs.close()
        return out
    one, zero = _both(run)
    assert all(np.isfinite(o[0]) for o in one)
    _same(one, zero)


def test_355_states():
    """max_cn 12: 355 states (6 per lane: two words of class indices, two of four allele planes stashed), 59 classes."""
    _sweeps(300, 3, 12, 3, 355, 59)


def test_four_clones_207_states_use_the_second_class_slot():
    """65 classes: lanes 0 .. 63 own one class, lane 0 a second one."""
    _sweeps(200, 4, 4, 2, 207, 65, h_of=lambda p: np.array([p['h_normal']] + [p['h_tumour'] * f for f in (0.5, 0.3, 0.2)]))


def test_47_states():
    """max_cn 4: one state per lane, 19 classes."""
    _sweeps(300, 3, 4, 3, 47, 19)


def test_model_without_a_normal_clone():
    """The configuration of tests/golden/model_nonormal.npz (the hdel branch of the read-depth likelihood; 6 states: row kernels,
    no cell cache in either form), and the same branch at 47 states, where the cache is in use."""
    from remixt_amd import bpmodel
    from tests import golden_runner as G
    g = G.load('model_nonormal')

    def run(v):
        m = G.build(g, bpmodel)
        m.num_em_iter = 0
        m.fit(g['h_init'])
        for _ in range(2):
            m.variational_update()
        return [m.model.calculate_elbo()] + [np.asarray(getattr(m.model, a)) for a in ARRAYS]
    one, zero = _both(run)
    _same(one, zero)
    _sweeps(300, 3, 4, 3, 47, None, normal_contamination=False)


def test_165_states_with_masked_segments():
    """total_likelihood_mask zero on every third segment (the class rows hold exactly 0 there), allele_likelihood_mask zero on
    every fifth."""
    _sweeps(700, 3, 8, 3, 165, 39, masks=True)
