"""CPU: the path entropy without a device.  The numpy twin (tests/entropy_twin.py) against path enumeration;
posteriors.entropy_runs against enumeration on runs with inserted segments, with the slack bound; posteriors.batch_path_entropy
through a stand-in batch with planted arrays; the query table's fourth tuple; what is declared and bound; and the
NotImplementedError over the oracle module."""
import inspect
import os
import re

import numpy as np
import pytest

from remixt_amd import _lib, cn_model, posteriors, queries, restarts
from tests import entropy_twin
from tests.region_twin import RegionTwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL_CLASSES = (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def _problem(N, S, seed, scale=2.0):
    rng = np.random.RandomState(seed)
    return rng.normal(0, scale, size=(N, S)), -rng.exponential(scale, size=(max(N - 1, 0), S, S))


# ---- the twin against enumeration ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('lengths,S,seed', [((1,), 3, 0), ((2,), 4, 1), ((6,), 2, 2), ((5,), 3, 3), ((4, 1, 3), 3, 4), ((1, 1), 4, 5), ((3, 4), 4, 6)])
def test_twin_against_enumeration(lengths, S, seed):
    """Every interval of every chain, those that start or end at a chain end and a chain of one segment included: the entropy
    of the enumerated joint of the chain, marginalised outside the interval."""
    N = sum(lengths)
    f, T = _problem(N, S, seed)
    ce = np.cumsum(lengths) - 1
    cs = np.concatenate([[0], ce[:-1] + 1])
    twin = RegionTwin(f, T, cs, ce)
    marg, step = entropy_twin.arrays(twin)
    assert marg.shape == step.shape == (N,) and (step[ce] == 0).all()
    worst, count = 0., 0
    for c0, c1 in zip(cs, ce):
        joint = entropy_twin.enumerate_joint(f[c0:c1 + 1], T[c0:c1])
        for a in range(c0, c1 + 1):
            for b in range(a, c1 + 1):
                want = entropy_twin.joint_entropy(joint, range(a - c0, b - c0 + 1))
                got = entropy_twin.run_entropy(marg, step, a, b)
                worst = max(worst, abs(float(got - want)))
                count += 1
                assert abs(got - want) <= 1e-13, (a, b, got, want)
    assert count == sum(n * (n + 1) // 2 for n in lengths)
    # posteriors.entropy_runs on the twin's arrays: every interval again, by prefix sums in double
    runs = [(a, b) for c0, c1 in zip(cs, ce) for a in range(c0, c1 + 1) for b in range(a, c1 + 1)]
    got = posteriors.entropy_runs(marg.astype(float), step.astype(float), runs, np.ones(N, dtype=int))
    want = np.array([float(entropy_twin.run_entropy(marg, step, a, b)) for a, b in runs])
    assert np.abs(got['path_entropy'] - want).max() <= 1e-12 and (got['inserted_slack'] == 0).all()
    assert np.array_equal(got['num_segments'], [b - a + 1 for a, b in runs])
    # a step is a conditional entropy: within [0, the segment's marginal entropy]
    assert (step >= -1e-15).all() and (step <= marg + 1e-15).all()


# ---- entropy_runs against enumeration, with inserted segments ---------------------------------------------------------------
def _one_chain(f, T):
    N = len(f)
    twin = RegionTwin(f, T, np.array([0]), np.array([N - 1]))
    marg, step = entropy_twin.arrays(twin)
    return marg.astype(float), step.astype(float), entropy_twin.enumerate_joint(f, T)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_entropy_runs_against_enumeration(seed):
    N, S = 6, 3
    f, T = _problem(N, S, 10 + seed)
    marg, step, joint = _one_chain(f, T)
    real = np.array([1, 1, 0, 1, 0, 1])
    runs = [(0, 5), (1, 3), (0, 1), (3, 5), (1, 5), (3, 3)]
    out = posteriors.entropy_runs(marg, step, runs, real)
    assert list(out) == ['path_entropy', 'marginal_entropy_sum', 'inserted_slack', 'num_segments']
    assert np.array_equal(out['num_segments'], [4, 2, 2, 2, 3, 1]) and out['num_segments'].dtype == np.int64
    for i, (a, b) in enumerate(runs):
        H = float(entropy_twin.joint_entropy(joint, range(a, b + 1)))
        Hreal = float(entropy_twin.joint_entropy(joint, [n for n in range(a, b + 1) if real[n]]))
        inserted = [n for n in range(a, b + 1) if not real[n]]
        assert abs(out['path_entropy'][i] - H) <= 1e-12, (a, b)
        assert abs(out['marginal_entropy_sum'][i] - marg[a:b + 1].sum()) <= 1e-12
        assert abs(out['inserted_slack'][i] - step[inserted].sum()) <= 1e-12
        assert H - out['inserted_slack'][i] - 1e-12 <= Hreal <= H + 1e-12, (a, b, H, Hreal, out['inserted_slack'][i])
        assert out['marginal_entropy_sum'][i] - out['path_entropy'][i] >= -1e-12      # total correlation
        if not inserted:
            assert out['inserted_slack'][i] == 0 and abs(Hreal - H) <= 1e-15
    # leading axes ride along
    both = posteriors.entropy_runs(np.stack([marg, 2 * marg]), np.stack([step, 3 * step]), runs, real)
    assert both['path_entropy'].shape == (2, len(runs)) and np.array_equal(both['path_entropy'][0], out['path_entropy'])
    assert np.allclose(both['inserted_slack'][1], 3 * out['inserted_slack'], rtol=1e-14, atol=1e-300)
    none = posteriors.entropy_runs(marg, step, np.zeros((0, 2), dtype=int), real)
    assert none['path_entropy'].shape == (0,) and none['num_segments'].shape == (0,)
    for bad in ([(2, 1)], [(-1, 2)], [(0, N)]):
        with pytest.raises(ValueError):
            posteriors.entropy_runs(marg, step, bad, real)


def test_the_slack_bound_is_not_vacuous():
    """An inserted segment whose posterior is nearly uniform and nearly free of its neighbours: it carries almost log S of the
    path's entropy, the slack says so, and the real segments' entropy sits near the lower end of the bound."""
    N, S = 5, 4
    f, T = _problem(N, S, 3)
    f[2] = 0.
    T[1] = T[2] = -1e-3 * np.abs(T[1])
    marg, step, joint = _one_chain(f, T)
    real = np.array([1, 1, 0, 1, 1])
    out = posteriors.entropy_runs(marg, step, [(0, 4)], real)
    H, slack = out['path_entropy'][0], out['inserted_slack'][0]
    Hreal = float(entropy_twin.joint_entropy(joint, [0, 1, 3, 4]))
    assert slack > 0.9 * np.log(S) and slack == step[2]
    assert H - slack - 1e-12 <= Hreal <= H + 1e-12 and Hreal < H - 0.5 * slack


# ---- batch_path_entropy through a stand-in batch ----------------------------------------------------------------------------
class FakeBatch(object):
    """path_entropy_raw answers with planted arrays and counts its calls."""

    def __init__(self, marg, step):
        self.marg, self.step, self.calls = marg, step, []

    def path_entropy_raw(self, r0, nr, n0=0, n1=None):
        self.calls.append((r0, nr, n0, n1))
        return self.marg[r0:r0 + nr].copy(), self.step[r0:r0 + nr].copy()


# eight model segments in two chains (0 .. 4 and 5 .. 7), segment 2 inserted; seven experiment segments
TEL = np.array([0, 0, 0, 0, 1, 0, 0, 1])
REAL = np.array([1, 1, 0, 1, 1, 1, 1, 1])
FWD = np.array([0, 1, 3, 4, 5, 6, 7])


def _planted(R=3):
    rng = np.random.RandomState(5)
    marg = rng.uniform(0.1, 2., size=(R, 8))
    step = rng.uniform(0.01, 0.1, size=(R, 8))
    step[:, TEL != 0] = 0.
    return marg, step


def test_batch_path_entropy():
    marg, step = _planted()
    fb = FakeBatch(marg, step)
    regions = [(1, 2), (2, 5), (0, 6), (4, 4), (3, 4)]
    out = posteriors.batch_path_entropy(fb, 1, 2, regions, FWD, REAL, TEL)
    assert fb.calls == [(1, 2, 0, None)] or fb.calls == [(1, 2)]            # one device call over all segments
    assert list(out) == ['segment_entropy', 'step_entropy', 'adjacent_information', 'path_entropy', 'inserted_slack', 'marginal_entropy_sum',
                         'total_correlation', 'perplexity', 'entropy_per_segment']
    m, s = marg[1:3], step[1:3]
    assert np.array_equal(out['segment_entropy'], m[:, FWD])
    want_step = np.stack([s[:, 0], s[:, 1] + s[:, 2], s[:, 3], np.full(2, np.nan), s[:, 5], s[:, 6]], axis=1)
    assert out['step_entropy'].shape == (2, 6) and np.array_equal(np.isnan(out['step_entropy']), np.isnan(want_step))
    assert np.allclose(out['step_entropy'], want_step, rtol=0, atol=1e-14, equal_nan=True)
    want_info = np.stack([m[:, 0] - s[:, 0], np.full(2, np.nan), m[:, 3] - s[:, 3], np.full(2, np.nan), m[:, 5] - s[:, 5], m[:, 6] - s[:, 6]], axis=1)
    assert np.array_equal(np.isnan(out['adjacent_information']), np.isnan(want_info))
    assert np.allclose(out['adjacent_information'], want_info, rtol=0, atol=1e-14, equal_nan=True)
    # (1, 2): the model run 1 .. 3 with the inserted segment 2; (2, 5): pieces (3, 4) and (5, 6) in two chains add;
    # (0, 6): the genome; (4, 4): one segment; (3, 4): model 4 | 5, the two sides of a chain end
    H = np.stack([m[:, 3] + s[:, 1] + s[:, 2], m[:, 4] + s[:, 3] + m[:, 6] + s[:, 5], m[:, 4] + s[:, :4].sum(axis=1) + m[:, 7] + s[:, 5:7].sum(axis=1),
                  m[:, 5], m[:, 4] + m[:, 5]], axis=1)
    slack = np.stack([s[:, 2], 0 * s[:, 0], s[:, 2], 0 * s[:, 0], 0 * s[:, 0]], axis=1)
    msum = np.stack([m[:, 1:4].sum(axis=1), m[:, 3:7].sum(axis=1), m.sum(axis=1), m[:, 5], m[:, 4:6].sum(axis=1)], axis=1)
    nreal = np.array([2, 4, 7, 1, 2])
    for key, want in (('path_entropy', H), ('inserted_slack', slack), ('marginal_entropy_sum', msum), ('total_correlation', msum - H),
                      ('perplexity', np.exp(H)), ('entropy_per_segment', H / nreal)):
        assert out[key].shape == (2, 5) and np.allclose(out[key], want, rtol=1e-13, atol=1e-13), key
    # regions=None: one region, the genome
    fb.calls = []
    whole = posteriors.batch_path_entropy(fb, 0, 3, None, FWD, REAL, TEL)
    assert len(fb.calls) == 1 and whole['path_entropy'].shape == (3, 1)
    assert np.allclose(whole['path_entropy'][1:, 0], H[:, 2], rtol=1e-13) and np.allclose(whole['entropy_per_segment'][1:, 0], H[:, 2] / 7, rtol=1e-13)
    assert np.array_equal(whole['segment_entropy'][1:], out['segment_entropy']) and np.array_equal(whole['step_entropy'][1:], out['step_entropy'], equal_nan=True)
    # no regions: the per-segment arrays, and empty per-region ones
    fb.calls = []
    none = posteriors.batch_path_entropy(fb, 0, 3, [], FWD, REAL, TEL)
    assert len(fb.calls) == 1 and np.array_equal(none['segment_entropy'], marg[:, FWD])
    for key in posteriors.PATH_ENTROPY_ARRAYS:
        assert none[key].shape == (3, 0), key
    with pytest.raises(ValueError):
        posteriors.batch_path_entropy(fb, 0, 3, [(3, 2)], FWD, REAL, TEL)
    with pytest.raises(ValueError):
        posteriors.batch_path_entropy(fb, 0, 3, [(0, 7)], FWD, REAL, TEL)


def test_posteriors_stays_free_of_the_package():
    """entropy_runs and batch_path_entropy came without an import of the package."""
    import ast
    assert callable(posteriors.entropy_runs) and callable(posteriors.batch_path_entropy)
    tree = ast.parse(_read('remixt_amd', 'posteriors.py'))
    for node in tree.body:
        assert not (isinstance(node, ast.ImportFrom) and node.level > 0)
        assert not (isinstance(node, ast.Import) and any(a.name.startswith('remixt_amd') for a in node.names))


# ---- the query table ----------------------------------------------------------------------------------------------------------
OLD_NAMES = ['posterior_summary', 'region_events', 'region_change_counts', 'region_cn_extremes', 'region_clone_extremes', 'region_cn_moments',
             'event_extent', 'conditional_summary', 'event_span', 'event_joint', 'focal_events', 'breakend_changes', 'region_call',
             'region_alternatives', 'call_confidence', 'cn_logprob', 'cn_change_prob', 'locus_joint', 'locus_dependence', 'region_automaton',
             'event_runs', 'event_run_of']


def test_query_table():
    assert [e.name for e in queries.ENTROPY_QUERIES] == ['path_entropy']
    assert [e.name for e in queries.ALL_QUERIES] == OLD_NAMES and sorted(queries.BY_NAME) == sorted(OLD_NAMES)
    assert len(queries.BY_NAME) == len(queries.QUERIES) + len(queries.LATER_QUERIES) + 3 and 'path_entropy' not in queries.BY_NAME
    assert queries.ALL_QUERIES == queries.QUERIES + queries.LATER_QUERIES + queries.AUTOMATON_QUERIES
    for name in OLD_NAMES:
        assert queries.entry(name) is queries.BY_NAME[name]
    e = queries.entry('path_entropy')
    assert e is queries.ENTROPY_QUERIES[0] and e.needs == 'path_entropy_raw' and e.lacks == 'has no path entropy'
    assert e.cn is None and e.shared == () and e.extend == () and e.each == () and not e.many and e.finish is None and not e.flat
    with pytest.raises(KeyError):
        queries.entry('no_such_query')
    from remixt_amd import bpmodel
    assert hasattr(bpmodel.RemixtBatch, 'path_entropy_raw') and hasattr(bpmodel.RemixtModel, 'path_entropy')
    assert str(inspect.signature(bpmodel.RemixtBatch.path_entropy_raw)) == '(self, r0, nr, n0=0, n1=None)'
    assert str(inspect.signature(bpmodel.RemixtModel.path_entropy)) == '(self, n0=0, n1=None)'
    for cls in LEVEL_CLASSES:
        method = getattr(cls, 'path_entropy')
        assert 'path_entropy' in vars(cls) and inspect.isfunction(method)
        assert str(inspect.signature(method)) == '(self, regions=None)'
        assert method.__doc__ and method.__doc__.strip() and method.__name__ == 'path_entropy' and method.__qualname__ == '%s.path_entropy' % cls.__name__
        for name in OLD_NAMES:
            assert name in vars(cls)
    assert 'perplexity' in cn_model.BreakpointModel.path_entropy.__doc__ and 'restart axis' in restarts.RestartSet.path_entropy.__doc__
    # no config key, no result record
    from remixt_amd import outputs
    assert 'path_entropy' not in _read('remixt_amd', 'defaults.py') and 'path_entropy' not in _read('remixt_amd', 'outputs.py') and not any('path_entropy' in k for k in vars(outputs))


def test_join_and_only_along_the_restart_axis():
    e = queries.entry('path_entropy')
    marg, step = _planted(4)
    a = posteriors.batch_path_entropy(FakeBatch(marg, step), 0, 3, [(1, 2), (2, 5)], FWD, REAL, TEL)
    b = posteriors.batch_path_entropy(FakeBatch(marg, step), 3, 1, [(1, 2), (2, 5)], FWD, REAL, TEL)
    whole = posteriors.batch_path_entropy(FakeBatch(marg, step), 0, 4, [(1, 2), (2, 5)], FWD, REAL, TEL)
    joined = queries._join([a, b], e.shared, e.extend, e.each)
    assert list(joined) == list(whole)
    for k in whole:
        assert joined[k].shape == whole[k].shape and np.array_equal(joined[k], whole[k], equal_nan=True), k
    one = queries._only(e, b)
    for k in whole:
        assert one[k].shape == whole[k].shape[1:] and np.array_equal(one[k], whole[k][3], equal_nan=True), k


def test_the_levels_forward_to_the_batch_function():
    """The model level strips the restart axis, the set level asks all its restarts at once."""
    marg, step = _planted(3)

    class Model(object):
        seg_fwd_remap, seg_is_original, is_telomere = FWD, REAL, TEL

    fb = FakeBatch(marg, step)
    models = [Model(), Model(), Model()]
    e = queries.entry('path_entropy')
    got = e.call(queries.Restarts(fb, 0, 3, models), regions=[(0, 6)])
    assert fb.calls[0][:2] == (0, 3) and got['path_entropy'].shape == (3, 1)
    one = queries._only(e, e.call(queries.Restarts(fb, 2, 1, models[2:]), regions=None))
    assert one['path_entropy'].shape == (1,) and one['path_entropy'][0] == got['path_entropy'][2, 0]


# ---- declared and bound -------------------------------------------------------------------------------------------------------
def test_declared_and_bound():
    header = re.sub(r'\s+', ' ', _read('include', 'remixt_amd.h'))
    assert 'int rmx_path_entropy(rmx_batch *b, int32_t r0, int32_t nr, int32_t n0, int32_t n1, double *marginal_out, double *step_out);' in header
    for words in ('DESIGN 4.24', 'bpmodel.pyx:1213-1246', 'nats', '+0.0', 'RMX_EASSERT', 'E1(s\')', 'E2(s\')'):
        assert words in header, words
    res, args = _lib.SYMBOLS['rmx_path_entropy']
    assert len(args) == 7
    api = _read('remixt_amd', 'csrc', 'rmx_api.hip')
    assert re.search(r'^int rmx_path_entropy\(rmx_batch \*b, int32_t r0, int32_t nr, int32_t n0, int32_t n1, double \*marginal_out, double \*step_out\) \{', api, re.M)
    for words in ('require_snapshot(b, r0, nr, "path_entropy")', 'for_model_runs(b, r0, rb, rb + nrr', 'report_flags(b, b->d_rflags, r0, nr, "path_entropy', 'rmxh::entropy_chunk(',
                  'rmxh::entropy_tiles(', 'rmxh::entropy_range_ok('):
        assert words in api, words
    host = _read('remixt_amd', 'csrc', 'rmx_host.h')
    for sig in ('inline bool entropy_range_ok(int64_t N, int64_t n0, int64_t n1)',
                'inline EntropyCounts entropy_tiles(int32_t n0, int32_t n1, const int32_t *tclass, const int32_t *brk_slot, int32_t TC, int32_t *tiles_out, int32_t *singles_out)',
                'inline int64_t entropy_chunk(int64_t nr, int64_t nseg, int64_t budget_bytes)'):
        assert sig in host, sig
    assert 'hip' not in host.split('namespace rmxh')[1].split('entropy_range_ok')[1].split('check_pairs')[0].lower()      # usable without a device


def test_the_kernels_place_and_shape():
    k = _read('remixt_amd', 'csrc', 'rmx_kernels.h')
    at = k.index('void k_path_entropy(')
    assert k.index('void k_restart_overlap(') < at < k.index('void k_region_automaton(')
    section = k[k.rindex('// =====', 0, k.rindex('// =====', 0, at)):k.index('// Region automata (DESIGN 4.23)')]
    assert 'DESIGN 4.24' in section
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64(' in section and 'atomicAdd' not in section and 'asm' not in section
    bodies = section.split('__global__')[1:]
    assert len(bodies) == 2 and 'void k_path_entropy(' in bodies[0] and 'void k_path_entropy_adj(' in bodies[1]
    for body in bodies:
        assert body.count('atomicOr(&flags[r]') == 1 and 'RGN_ERR_DENOM' in body
    assert '__builtin_amdgcn_mfma_f64_16x16x4f64(' in bodies[0] and 'rgn_adj(' in bodies[1] and 'rgn_block_sum(' in bodies[1] and 'group_sum(' in section


def test_the_kernel_name_lists_are_the_parents():
    api = _read('remixt_amd', 'csrc', 'rmx_api.hip')

    def names(var):
        body = re.search(r'static const char \*%s\[[^\]]*\] = \{(.*?)\};' % var, api, re.S).group(1)
        return re.findall(r'"([^"]*)"', body)
    first, pair, later = names('kKernelNames'), names('kPairKernelNames'), names('kLaterKernelNames')
    assert len(first) == 31 and first[0] == 'k_state_tables' and first[-1] == 'k_region_extremes'
    assert pair == ['k_restart_overlap'] and later == ['k_region_conditional']
    assert not any('entropy' in n for n in first + pair + later)
    assert 'KID_NONE' in api.split('int rmx_path_entropy(')[0].rsplit('// Path entropy', 1)[1] or 'no profile id' in api.split('int rmx_path_entropy(')[0].rsplit('// Path entropy', 1)[1]


def test_no_path_entropy_without_the_kernel():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError, match='has no path entropy'):
        mo.path_entropy()
    with pytest.raises(NotImplementedError):
        mo.path_entropy([(1, 4)])
