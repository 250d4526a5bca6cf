"""Host side of the region alternatives (rmx_region_kbest; remixt_amd/posteriors.py combine_kbest, batch_region_alternatives) and
its numpy twin, without a GPU: the twin against path enumeration and its identities, combine_kbest against brute force over all
rank tuples, batch_region_alternatives against a batch answered by the twin, and the declarations.
test_twin_* run test-side code only: they check the reference the device tests are held to, and pass with or without the
feature; every other test here needs it."""
import itertools
import os
import re

import numpy as np
import pytest

from remixt_amd import posteriors
from tests import call_twin, decode_twin, kbest_twin, region_twin
from tests.test_region_decode_cpu import _CASES, _chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _full(path, a, N):
    return np.concatenate([np.zeros(a, dtype=int), path, np.zeros(N - a - len(path), dtype=int)])


@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('use_constrain', [False, True])
@pytest.mark.parametrize('case', range(len(_CASES)))
def test_twin_against_enumeration(case, use_constrain, K):
    N, S, a, b, mi, li = _CASES[case]
    f, T, masks, labels, constrain = _chain(20 + case, N, S)
    cs = constrain if use_constrain else None
    mk, lb = (None if mi < 0 else masks[mi]), (None if li < 0 else labels[li])
    twin = region_twin.RegionTwin(f, T, [0], [N - 1])
    logp, paths = kbest_twin.kbest(twin, a, b, K, mk, lb, cs)
    want, every = kbest_twin.brute_force(f, T, a, b, K, mk, lb, cs)
    marg = dict((k, v) for v, k in every)
    found = min(K, len(every))
    assert np.isfinite(want[0]) and np.abs(logp[:found] - want[:found]).max() <= 1e-12
    assert (logp[found:] == -np.inf).all() and all(p is None for p in paths[found:])
    keys = [tuple(int(s) for s in p) for p in paths[:found]]
    assert len(set(keys)) == found                                                   # pairwise distinct
    assert (np.diff(logp[:found]) <= 0).all()                                       # values do not increase
    for k, key in enumerate(keys):
        # the path's own marginal is the k-th optimum, it satisfies the event, and the call twin agrees
        assert abs(marg[key] - want[k]) <= 1e-12 and decode_twin.satisfies(paths[k], a, b, mk, lb, cs)
        assert abs(call_twin.logprob(twin, a, b, None, _full(paths[k], a, N)) - logp[k]) <= 1e-12
    # rank 0 is the decode twin's
    d0, p0 = decode_twin.decode(twin, a, b, mk, lb, cs)
    assert logp[0] == d0 and np.array_equal(paths[0], p0)
    # the list does not exceed the sum
    assert np.logaddexp.reduce(logp[:found]) <= twin.logprob(a, b, mk, lb, cs) + 1e-12


def test_twin_fewer_than_k_paths_and_impossible():
    f, T, masks, labels, _ = _chain(3, 5, 3)
    twin = region_twin.RegionTwin(f, T, [0], [4])
    one = np.zeros((5, 3), dtype=bool); one[:, 1] = True; one[3, 2] = True      # one state everywhere, two at segment 3
    logp, paths = kbest_twin.kbest(twin, 2, 4, 8, one, None)
    want, every = kbest_twin.brute_force(f, T, 2, 4, 8, one, None)
    assert len(every) == 2 and np.isfinite(logp[:2]).all() and (logp[2:] == -np.inf).all() and np.abs(logp[:2] - want[:2]).max() <= 1e-12
    assert sorted(tuple(p) for p in paths[:2]) == [(1, 1, 1), (1, 2, 1)] and paths[2] is None
    masks = masks.copy(); masks[0, 3] = False
    logp, paths = kbest_twin.kbest(twin, 2, 4, 3, masks[0], None)
    assert (logp == -np.inf).all() and paths == [None] * 3
    # one segment: the K largest marginals, stable
    logp, paths = kbest_twin.kbest(twin, 2, 2, 3)
    post = np.array([twin.logprob(2, 2, np.arange(3)[None, :].repeat(5, axis=0) == s, None) for s in range(3)])
    assert [int(p[0]) for p in paths] == list(np.argsort(-post, kind='stable')) and np.abs(logp - np.sort(post)[::-1]).max() <= 1e-12


def test_twin_chain_end():
    rng = np.random.RandomState(5)
    N, S = 6, 3
    f, T = rng.normal(scale=2., size=(N, S)), rng.normal(scale=2., size=(N - 1, S, S))
    T[2] = 0.
    twin = region_twin.RegionTwin(f, T, [0, 3], [2, 5])
    for (a, b), (fs, Ts, a0) in (((3, 5), (f[3:], T[3:], 3)), ((1, 2), (f[:3], T[:2], 0))):
        logp, paths = kbest_twin.kbest(twin, a, b, 8)
        want, every = kbest_twin.brute_force(fs, Ts, a - a0, b - a0, 8)
        assert np.abs(logp - want).max() <= 1e-12 and len(set(tuple(p) for p in paths)) == 8
        marg = dict((k, v) for v, k in every)
        assert all(abs(marg[tuple(int(s) for s in p)] - logp[k]) <= 1e-12 for k, p in enumerate(paths))


def _combine_brute(logp, pieces, k):
    """Every tuple of ranks of the pieces, sums in piece order, sorted by (value descending, tuple ascending)."""
    every = []
    for t in itertools.product(*[range(logp.shape[1])] * len(pieces)):
        v = 0.
        for p, j in zip(pieces, t):
            v = v + logp[p, j]
        if v > -np.inf:
            every.append((v, t))
    every.sort(key=lambda c: (-c[0], c[1]))
    return every[:k]


@pytest.mark.parametrize('K,k', [(1, 1), (3, 3), (4, 2), (8, 8), (2, 5)])
def test_combine_kbest_against_brute_force(K, k):
    rng = np.random.RandomState(10 * K + k)
    # regions of 1 .. 4 pieces; quarter-integer values make ties, and their sums exact
    piece_region = np.array([0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 5])
    P, R = len(piece_region), 6
    logp = -np.sort(rng.randint(0, 6, size=(3, P, K)) / 4., axis=-1)
    logp[0, 2, K // 2 + 1:] = -np.inf              # padding
    logp[1, 4] = -np.inf                            # an impossible piece
    logp[2, :, 1:] = -np.inf                        # one rank everywhere
    values, choice = posteriors.combine_kbest(logp, piece_region, R, k)
    assert values.shape == (3, R, k) and choice.shape == (3, R, k, P)
    for i in range(3):
        for reg in range(R):
            pieces = np.flatnonzero(piece_region == reg)
            want = _combine_brute(logp[i], pieces, k) if len(pieces) else []
            assert np.array_equal(values[i, reg, :len(want)], [w[0] for w in want]) and (values[i, reg, len(want):] == -np.inf).all()
            for rank, (_, t) in enumerate(want):
                assert tuple(choice[i, reg, rank, pieces]) == t
                assert (np.delete(choice[i, reg, rank], pieces) == -1).all()
            assert (choice[i, reg, len(want):] == -1).all()
    assert (values[1, 2] == -np.inf).all() and (values[:, 4] == -np.inf).all()
    assert np.isfinite(values[2, :4, 0]).all() and (values[2, :, 1:] == -np.inf).all()
    # a NaN piece
    bad = logp.copy(); bad[0, 1, 0] = np.nan
    v2, c2 = posteriors.combine_kbest(bad, piece_region, R, k)
    assert np.isnan(v2[0, 1]).all() and (c2[0, 1] == -1).all() and np.array_equal(v2[0, 0], values[0, 0])
    with pytest.raises(ValueError):
        posteriors.combine_kbest(logp, piece_region, R, 0)


def _twin_batch(nr=2, seed=4):
    """tests/test_region_decode_cpu.py's twin batch: twelve model segments in two chains, six states of three clones."""
    from tests.test_region_decode_cpu import _twin_batch as make
    b, tel = make(nr, seed)
    kb = kbest_twin.KbestTwinBatch.__new__(kbest_twin.KbestTwinBatch)
    kb.__dict__.update(b.__dict__)
    return kb, tel


def test_region_alternatives_over_the_twin():
    b, tel = _twin_batch()
    fwd, orig = np.array([0, 1, 2, 4, 5, 6, 7, 9, 10, 11]), np.ones(12, dtype=bool)
    orig[[3, 8]] = False
    masks, labels = posteriors.event_tables(b.cn_classes)
    mk = masks[0][:, None, :].repeat(12, axis=1) != 0
    lb = labels[0][:, None, :].repeat(12, axis=1)
    nloh, tot = posteriors.MASK_NAMES.index('not_loh'), posteriors.LABEL_NAMES.index('total')
    # regions: inside chain 0 across the inserted segment 3; across the chain end; one segment; named
    regions = [(1, 3), (3, 6), (7, 7), ('tail', 8, 9)]
    runs = [[(1, 4)], [(4, 5), (6, 7)], [(9, 9)], [(10, 11)]]
    rng = np.random.RandomState(1)
    call = rng.randint(0, 6, size=(2, 12))
    K = 8
    for event, mi, li in ((None, -1, -1), (('not_loh', None), nloh, -1), ((None, 'total'), -1, tot), (('not_loh', 'total'), nloh, tot)):
        del b.calls[:]
        out = posteriors.batch_region_alternatives(b, 0, 2, regions, fwd, orig, tel, k=K, event=event, cn=call)
        assert [c[0] for c in b.calls] == ['region_kbest'] + (['region_logprob'] if event else []) and b.calls[0][1:] == (2, 5, K)
        assert len(out) == 2 and all(len(row) == 4 for row in out)
        m_, l_ = (None if mi < 0 else mk[mi]), (None if li < 0 else lb[li])
        for r in range(2):
            tw = b.twins[r]
            for g, pieces in enumerate(runs):
                res = out[r][g]
                assert sorted(res) == ['cn', 'coverage', 'duplicate_of', 'log_p_event', 'log_prob', 'log_prob_given_event', 'n_differ', 'rank_of_call']
                assert res['log_prob'].shape == (K,) and res['log_prob_given_event'].shape == (K,) and res['n_differ'].shape == (K,) and res['duplicate_of'].shape == (K,)
                found = len(res['cn'])
                assert found == np.isfinite(res['log_prob']).sum() and (np.diff(res['log_prob'][:found]) <= 0).all()
                seg = fwd[regions[g][-2]:regions[g][-1] + 1]
                assert all(c.shape == (len(seg), 3, 2) for c in res['cn'])
                # the values: the K largest sums of one entry per piece, by brute force over the pieces' twin lists
                lists = [kbest_twin.kbest(tw, a, z, K, m_, l_, orig) for a, z in pieces]
                sums = sorted((sum(lst[0][j] for lst, j in zip(lists, t)) for t in itertools.product(range(K), repeat=len(pieces))), reverse=True)
                sums = [v for v in sums if v > -np.inf][:K]
                assert found == len(sums) and np.abs(res['log_prob'][:found] - sums).max() <= 1e-12
                ev = min(sum(tw.logprob(a, z, m_, l_, orig) for a, z in pieces), 0.) if event else 0.
                assert abs(res['log_p_event'] - ev) <= 1e-12
                assert np.abs(res['log_prob_given_event'][:found] - (res['log_prob'][:found] - ev)).max() <= 1e-12
                assert 0 < res['coverage'] <= 1 + 1e-12 and abs(res['coverage'] - np.exp(res['log_prob'][:found] - ev).sum()) <= 1e-12
                # rank 0 is region_call's configuration
                dec = posteriors.batch_region_calls(b, r, 1, regions[g:g + 1], fwd, orig, tel, event=event)
                assert np.array_equal(res['cn'][0], dec['cn'][0][0]) and abs(res['log_prob'][0] - dec['log_prob'][0, 0]) <= 1e-12
                # n_differ, rank_of_call and duplicate_of from the copy numbers themselves
                cn_call = b.cn_classes[0, call[r, seg]]
                for rank in range(found):
                    assert res['n_differ'][rank] == sum(not np.array_equal(x, y) for x, y in zip(res['cn'][rank], cn_call))
                    same = [j for j in range(rank) if np.array_equal(res['cn'][j], res['cn'][rank])]
                    assert res['duplicate_of'][rank] == (same[0] if same else -1)
                    if mi >= 0:
                        st = [int(np.flatnonzero((b.cn_classes[0] == c).all(axis=(1, 2)))[0]) for c in res['cn'][rank]]
                        assert all(mk[mi][n, s] for n, s in zip(seg, st))
                assert (res['n_differ'][found:] == -1).all() and (res['duplicate_of'][found:] == -1).all()
                hits = [rank for rank in range(found) if res['n_differ'][rank] == 0]
                assert res['rank_of_call'] == (hits[0] if hits else -1)
                if g in (2, 3):      # no inserted segment inside: distinct paths are distinct copy numbers (the states of a class differ)
                    assert (res['duplicate_of'] == -1).all()
    # a duplicate across an inserted segment: region 0 holds model segment 3; with 6^4 paths over 6^3 configurations of its
    # original segments, some of the eight best paths agree on them in this batch
    out = posteriors.batch_region_alternatives(b, 0, 2, regions[:1], fwd, orig, tel, k=K)
    dup = [res[0]['duplicate_of'] for res in out]
    assert any((d >= 0).any() for d in dup), dup
    for res in out:
        for rank in np.flatnonzero(res[0]['duplicate_of'] >= 0):
            assert np.array_equal(res[0]['cn'][rank], res[0]['cn'][res[0]['duplicate_of'][rank]])
    # the call as rank 2 of a region: rank_of_call finds it
    res = posteriors.batch_region_alternatives(b, 0, 1, regions[3:], fwd, orig, tel, k=4)[0][0]
    st = call[:1].copy()
    st[0, 10:12] = kbest_twin.kbest(b.twins[0], 10, 11, 4, None, None, orig)[1][2]
    again = posteriors.batch_region_alternatives(b, 0, 1, regions[3:], fwd, orig, tel, k=4, cn=st)[0][0]
    assert again['rank_of_call'] == 2 and again['n_differ'][2] == 0 and (again['n_differ'][[0, 1, 3]] > 0).all()
    assert res['rank_of_call'] == -1 and (res['n_differ'] == -1).all() and np.array_equal(res['log_prob'], again['log_prob'])
    # no regions; an unknown event
    assert posteriors.batch_region_alternatives(b, 0, 2, [], fwd, orig, tel, cn=call) == [[], []]
    with pytest.raises(ValueError):
        posteriors.batch_region_alternatives(b, 0, 2, regions, fwd, orig, tel, event=('nonsense', None))


def test_declared_and_bound():
    from remixt_amd import _lib, bpmodel, cn_model, restarts
    # (rmx_region_decode's 13 arguments and K: the 14 of the prototype below)
    assert 'rmx_region_kbest' in _lib.SYMBOLS and len(_lib.SYMBOLS['rmx_region_kbest'][1]) == 14
    with open(os.path.join(ROOT, 'include', 'remixt_amd.h')) as fh:
        text = re.sub(r'\s+', ' ', fh.read())
    assert ('int rmx_region_kbest(rmx_batch *b, int32_t r0, int32_t nr, int32_t nq, const int32_t *queries, int32_t nmask, '
            'const uint8_t *masks, int32_t nlabel, const int16_t *labels, const uint8_t *constrain, int32_t K, int32_t max_len, '
            'int16_t *states_out, double *logp_out);') in text
    assert 'DESIGN 4.21' in text
    lib = _lib.load()
    # no profile id: both name lists and the three id ranges answer as on the parent
    names = [lib.rmx_kernel_name(i).decode() for i in range(lib.rmx_num_kernels())]
    assert len(names) == 32 and names[-2:] == ['k_region_extremes', 'k_restart_overlap']
    ids = lib.rmx_num_profile_ids()
    pnames = [lib.rmx_profile_name(i).decode() for i in range(ids)]
    assert ids == len(names) + 1 and pnames[:len(names)] == names and pnames[-1] == 'k_region_conditional'
    assert 'k_region_kbest' not in pnames and lib.rmx_profile_name(ids).decode() == ''
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_host.h')) as fh:
        host = fh.read()
    assert 'inline int kbest_plan(' in host and 'inline bool kbest_k_ok(' in host
    with open(os.path.join(ROOT, 'remixt_amd', 'csrc', 'rmx_kernels.h')) as fh:
        kern = fh.read()
    start = kern.index('void k_region_kbest(')
    assert start > kern.index('void k_region_conditional(')
    body = kern[start:]
    for piece in ('rgn_tabs(', 'rgn_adj(', 'rgn_compact(', 'rgn_D_exp(', 'rgd_block_max(', 'rgd_take_max('):
        assert piece in body, piece
    assert 'RGN_MAXS]' not in body and body.count('atomicOr(&flags[r]') == 1      # no RGN_MAXS-sized static arrays
    assert hasattr(bpmodel.RemixtBatch, 'region_kbest_raw') and hasattr(bpmodel.RemixtModel, 'region_kbest')
    for cls in (cn_model.BreakpointModel, restarts.RestartSet, restarts.RestartGroups, restarts.DatasetGroups):
        assert hasattr(cls, 'region_alternatives'), cls


def test_no_region_alternatives_without_the_kernel():
    from oracle import oracle
    from tests import helpers as H
    oracle.build()
    mo, ho, _ = H.make_model(oracle, N=30, M=3, max_cn=3)
    H.attach(mo, ho)
    mo.variational_update()
    with pytest.raises(NotImplementedError):
        mo.region_alternatives([(1, 2)])
