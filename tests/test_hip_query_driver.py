"""The host path the posterior queries share (rmx_sample_cn, rmx_region_prob, rmx_region_counts, rmx_call_prob): a call
whose restarts took their snapshots under different transition models is cut into runs, and queries that exceed one chunk
of the 64 MiB staging buffer go through it in several."""
import time

import numpy as np
import pytest

from remixt_amd import posteriors, synthetic
from tests.test_hip_call_confidence import _check_against_twin
from tests.test_hip_region_counts import CountsCase
from tests.test_hip_region_events import LABELS, MASKS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def hip():
    from remixt_amd import bpmodel
    return bpmodel


def _restart_set(num_restarts):
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=4)
    ps = synthetic.make_init_params(e, num_restarts, 4)
    rs = RestartSet(e, ps, 4, num_clones=3, quiet=True, seeds=list(range(num_restarts)))
    # the sweeps run on the total read counts alone: a state and its allele swap tie, so paths and probabilities are not all 0 or 1
    for r in range(num_restarts):
        rs.batch.set_array(r, 'allele_likelihood_mask', np.zeros(rs.batch.num_segments, dtype=np.int64))
    rs.variational_update(2)
    return rs


def _argmax_paths(b, nr):
    post = np.stack([b.get_array(r, 'posterior_marginals') for r in range(nr)])
    return np.argmax(post, axis=2).astype(np.int16)[:, None]      # (nr, 1, N)


def _runs(case):
    """A segment, a pair, every whole chain, a run from a chain start and one to a chain end."""
    cs, ce = case.cs, case.ce
    c = int(np.argmax(ce - cs))
    mid = int((cs[c] + ce[c]) // 2)
    return [(mid, mid), (mid, mid + 1)] + [(int(a), int(z)) for a, z in zip(cs, ce)] + [(int(cs[1]), int(min(cs[1] + 3, ce[1]))), (int(max(ce[0] - 2, cs[0])), int(ce[0]))]


def test_several_model_runs_in_one_call(hip):
    """Restarts 0 and 3 keep their model-0 snapshot, restarts 1 and 2 take theirs under model 1: a call over 0 .. 3 has three
    runs.  Each entry point returns for the whole range what it returns restart by restart, and restarts 0 and 1 agree with
    the numpy twins on their own snapshot within the bounds of the entry points' test_mixed_transition_model."""
    rs = _restart_set(4)
    try:
        b = rs.batch
        T_before = [b.get_array(r, 'log_transmat') for r in range(4)]
        b.transition_model = 1
        b.update_p_cn(1, 3)
        for r in range(4):
            assert np.array_equal(b.get_array(r, 'log_transmat'), T_before[r]) == (r in (0, 3)), r
        cases = [CountsCase(rs.models[r]) for r in (0, 1)]
        assert [c.r for c in cases] == [0, 1] and all(c.b is b for c in cases)
        case = cases[0]
        runs = _runs(case)
        masks, labels, constrain = case.masks, case.labels, case.constrain
        paths = _argmax_paths(b, 4)
        qr = np.array([[a, z, mi, li] for a, z in runs for mi, li in ((-1, -1), (1, -1), (-1, 1), (5, 2))], dtype=np.int32)
        qc = np.array([[a, z, mi, li] for a, z in runs for mi, li in ((-1, 0), (1, 1), (5, 2))], dtype=np.int32)
        qp = np.array([[a, z, li, 0] for a, z in runs for li in (-1, 0, 1, 2)], dtype=np.int32)
        seeds = [11, 12, 13, 14]
        calls = {
            'k_sample_cn': lambda r0, nr: b.sample_states(r0, nr, 9, seeds[r0:r0 + nr]),
            'k_region_prob': lambda r0, nr: b.region_logprob_raw(r0, nr, qr, masks, labels, constrain),
            'k_region_counts': lambda r0, nr: b.region_counts_raw(r0, nr, qc, masks, labels, constrain, 5),
            'k_call_prob': lambda r0, nr: b.call_logprob_raw(r0, nr, paths[r0:r0 + nr], qp, labels, constrain),
        }
        for kernel, call in calls.items():
            b.profile_reset(); b.profile_enable(1)
            full = call(0, 4)
            launches = b.profile()[kernel][1]; b.profile_enable(0)
            assert launches == 3, (kernel, launches)
            distinct = len(np.unique(full.reshape(4 if full.dtype.kind == 'f' else 4 * 9, -1), axis=0))
            print('%s: %d launches, %d distinct %s' % (kernel, launches, distinct, 'rows' if full.dtype.kind == 'f' else 'paths'))
            assert len(full) == 4 and distinct > 1, kernel      # (restarts that all answered alike would hide a wrong offset)
            for r in range(4):
                assert np.array_equal(call(r, 1)[0], full[r], equal_nan=True), (kernel, r)
            assert np.array_equal(call(1, 3), full[1:], equal_nan=True), kernel      # (two runs, the first not at restart 0)
        for c in cases:
            tag = 'restart %d' % c.r
            c.check_against_twin(runs, tag=tag)
            c.check_counts(runs, bins=(5,), tag=tag)
            _check_against_twin(c, paths[c.r], runs, tag=tag)
    finally:
        rs.close()


def test_more_than_one_chunk(hip):
    """16 restarts and more queries than one chunk of the staging buffer holds -- (64 MiB) // (16 * 8 + 16) of them with
    one output per query -- through rmx_region_prob and rmx_call_prob: at least two launches, and every copy of a query
    returns what its first occurrence returns (timed, no time asserted)."""
    nr = 16
    rs = _restart_set(nr)
    try:
        b, m = rs.batch, rs.models[0]
        masks, labels = posteriors.event_tables(b.cn_classes)
        cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
        chunk = (64 << 20) // (nr * 8 + 16)
        assert chunk < 500000
        a0, a1 = int(cs[0]), int(cs[1])
        z0, z1 = min(a0 + 2, int(ce[0])), min(a1 + 5, int(ce[1]))
        paths = _argmax_paths(b, nr)
        for kernel, short, call in (
                ('k_region_prob', [[a0, z0, MASKS.index('not_loh'), LABELS.index('total')], [a1, z1, -1, LABELS.index('state')]],
                 lambda q: b.region_logprob_raw(0, nr, q, masks, labels, None)),
                ('k_call_prob', [[a0, z0, -1, 0], [a1, z1, LABELS.index('total'), 0]],
                 lambda q: b.call_logprob_raw(0, nr, paths, q, labels, None))):
            short = np.array(short, dtype=np.int32)
            first = call(short)
            assert first.shape == (nr, 2) and not np.isnan(first).any() and np.isfinite(first).any() and len(np.unique(first, axis=0)) > 1
            many = np.tile(short, (chunk // 2 + 2, 1))
            assert chunk < len(many) < 2 * chunk
            b.profile_reset(); b.profile_enable(1)
            t0 = time.perf_counter()
            big = call(many)
            wall = time.perf_counter() - t0
            ms, launches = b.profile()[kernel]; b.profile_enable(0)
            print('%s: %d restarts x %d queries, chunks of %d: %.1f ms wall, %.2f ms device in %d launches' % (kernel, nr, len(many), chunk, wall * 1e3, ms, launches))
            assert launches >= 2
            assert big.shape == (nr, len(many))
            assert (big[:, 0::2] == first[:, :1]).all() and (big[:, 1::2] == first[:, 1:2]).all()
    finally:
        rs.close()
