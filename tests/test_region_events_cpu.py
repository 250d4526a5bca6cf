"""Host side of the region event probabilities (remixt_amd/posteriors.py) and their numpy twin, without a GPU: the twin
against brute-force path enumeration, the mask / label tables against their definitions, experiment regions as model
runs, and the distributed record with and without config cn_regions."""
import itertools

import numpy as np

from remixt_amd import posteriors, restarts, synthetic
from remixt_amd.cn_model import BreakpointModel, create_cn_states
from tests import helpers as H
from tests import region_twin
from tests.test_cn_samples_records_cpu import _fake_result


def test_twin_against_enumeration():
    rng = np.random.RandomState(5)
    N, S = 5, 4
    f = rng.normal(scale=2., size=(N, S))
    T = rng.normal(scale=2., size=(N - 1, S, S))
    twin = region_twin.RegionTwin(f, T, [0], [N - 1])
    mask = rng.uniform(size=(N, S)) < 0.6
    mask[np.arange(N), rng.randint(0, S, size=N)] = True
    label = rng.randint(0, 2, size=(N, S))
    identity = np.tile(np.arange(S), (N, 1))
    holes = np.array([1, 0, 1, 1, 0], dtype=bool)
    cases = [dict(), dict(mask=mask), dict(label=label), dict(mask=mask, label=label), dict(mask=mask, constrain=holes),
             dict(label=identity)]
    finite = 0
    for a, b in itertools.combinations_with_replacement(range(N), 2):
        for kw in cases:
            want = region_twin.brute_force(f, T, a, b, **kw)
            got = twin.logprob(a, b, **kw)
            if want == -np.inf:      # (a random label table can leave no path)
                assert got == -np.inf, (a, b, sorted(kw), got)
                continue
            finite += 1
            assert abs(got - want) <= 1e-12 and abs(np.exp(got) - np.exp(want)) <= 1e-12, (a, b, sorted(kw), got, want)
        assert abs(twin.logprob(a, b)) <= 1e-15
    assert finite >= 80
    # an impossible event
    none = np.zeros((N, S), dtype=bool)
    assert twin.logprob(1, 2, mask=none) == -np.inf and region_twin.brute_force(f, T, 1, 2, mask=none) == -np.inf


def test_twin_with_two_chains():
    """Chains are independent: a twin over two chains gives each chain's own probabilities."""
    rng = np.random.RandomState(6)
    S = 3
    f = rng.normal(size=(7, S)); T = rng.normal(size=(6, S, S))
    T[3] = 0.      # (the adjacency across the chain end, as log_transmat holds it)
    both = region_twin.RegionTwin(f, T, [0, 4], [3, 6])
    first = region_twin.RegionTwin(f[:4], T[:3], [0], [3])
    second = region_twin.RegionTwin(f[4:], T[4:], [0], [2])
    label = rng.randint(0, 2, size=(7, S))
    assert abs(both.logprob(1, 3, label=label) - first.logprob(1, 3, label=label[:4])) <= 1e-15
    assert abs(both.logprob(4, 6, label=label) - second.logprob(0, 2, label=label[4:])) <= 1e-15


def _two_classes(M, max_cn):
    grid = create_cn_states(M, 2, max_cn, 1)
    classes = np.repeat(grid[None], 2, axis=0)
    classes[1, :, 0, :] = [1, 0]
    return classes


def test_event_tables_against_definitions():
    for M, max_cn in ((3, 3), (2, 4), (4, 2)):
        classes = _two_classes(M, max_cn)
        C, S = classes.shape[:2]
        masks, labels = posteriors.event_tables(classes)
        assert masks.shape == (C, 6, S) and masks.dtype == np.uint8 and labels.shape == (C, 3, S) and labels.dtype == np.int16
        names = posteriors.MASK_NAMES
        for c in range(C):
            for s in range(S):
                cn = classes[c, s]
                loh = any(sum(cn[m, a] for m in range(M)) == 0 for a in range(2))
                hdel = all(cn[m, a] == 0 for m in range(M) for a in range(2))
                sub = sum(1 for a in range(2) if len(set(cn[m, a] for m in range(1, M))) > 1) > 0
                want = {'loh': loh, 'not_loh': not loh, 'hdel': hdel, 'not_hdel': not hdel, 'subclonal': sub, 'not_subclonal': not sub}
                for i, k in enumerate(names):
                    assert bool(masks[c, i, s]) == want[k], (c, s, k)
        # the same as the reference's derived tables through feature_matrix
        W, lay = posteriors.feature_matrix(classes)
        assert np.array_equal(masks[:, names.index('loh')], W[:, :, lay['loh']]) and np.array_equal(masks[:, names.index('hdel')], W[:, :, lay['hdel']])
        assert np.array_equal(masks[:, names.index('subclonal')], W[:, :, lay['subclonal']])
        assert masks[1, names.index('loh')].any() and not masks[0, names.index('loh')].any()
        # labels: equal exactly when the definition says so, within and across classes
        flat = [(c, s) for c in range(C) for s in range(S)]
        ln = posteriors.LABEL_NAMES
        for (c1, s1), (c2, s2) in itertools.product(flat, flat):
            t1, t2 = classes[c1, s1, 1:], classes[c2, s2, 1:]
            same = np.array_equal(t1, t2)
            assert (labels[c1, ln.index('state'), s1] == labels[c2, ln.index('state'), s2]) == same
            assert (labels[c1, ln.index('total'), s1] == labels[c2, ln.index('total'), s2]) == np.array_equal(t1.sum(axis=1), t2.sum(axis=1))
            assert (labels[c1, ln.index('unphased'), s1] == labels[c2, ln.index('unphased'), s2]) == (same or np.array_equal(t1, t2[:, ::-1]))
    # a table whose phasings are not canonical: the unphased label joins what the state label separates
    cls = np.array([[[[1, 1], [2, 1]], [[1, 1], [1, 2]], [[1, 1], [2, 2]]]])
    _, lab = posteriors.event_tables(cls)
    assert lab[0, 0, 0] != lab[0, 0, 1] and lab[0, 2, 0] == lab[0, 2, 1] and lab[0, 2, 0] != lab[0, 2, 2] and lab[0, 1, 0] == lab[0, 1, 1]


def test_region_queries_and_combine():
    # experiment segments 0 .. 7 in a model of 12 segments: zero-length segments before segment 0, between 1 and 2,
    # between 4 and 5 and after 7; chains end at model segments 5, 9 and 11
    fwd = np.array([1, 2, 4, 5, 6, 8, 9, 10])
    orig = np.array([0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0], dtype=bool)
    tel = np.array([0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0])      # (the last segment ends a chain with or without the flag)
    cs, ce = posteriors.chains_from_telomeres(tel)
    assert cs.tolist() == [0, 6, 10] and ce.tolist() == [5, 9, 11]
    regions = [(1, 2), (2, 4), (0, 0), (0, 7), (7, 7), (4, 5)]
    runs, piece_region, constrain = posteriors.region_queries(regions, fwd, orig, cs, ce)
    assert runs.dtype == np.int32 and constrain.dtype == np.uint8 and np.array_equal(constrain, orig)
    got = [[tuple(r) for r in runs[piece_region == i].tolist()] for i in range(len(regions))]
    assert got == [[(2, 4)],                          # the zero-length segment 3 lies inside the run
                   [(4, 5), (6, 6)],                  # across a chain end: one piece per chain
                   [(1, 1)],                          # touching segment 0: the segment inserted before it is not part of it
                   [(1, 5), (6, 9), (10, 10)],
                   [(10, 10)],                        # touching segment N - 1
                   [(6, 8)]]
    assert np.array_equal(piece_region, np.sort(piece_region))
    logp = np.log(np.arange(1, len(runs) + 1) / 10.)
    tot = posteriors.combine(logp, piece_region, len(regions))
    for i in range(len(regions)):
        assert np.isclose(tot[i], logp[piece_region == i].sum(), rtol=1e-15)
    two = posteriors.combine(np.stack([logp, 2 * logp]), piece_region, len(regions))
    assert two.shape == (2, len(regions)) and np.allclose(two[1], 2 * tot)
    logp[1] = -np.inf
    assert posteriors.combine(logp, piece_region, len(regions))[1] == -np.inf
    regs, n = posteriors.adjacency_regions(fwd, tel)
    assert n.tolist() == [0, 1, 2, 4, 5] and regs.tolist() == [[0, 1], [1, 2], [2, 3], [4, 5], [5, 6]]
    for bad in ([(3, 2)], [(-1, 2)], [(0, 8)]):
        try:
            posteriors.region_queries(bad, fwd, orig, cs, ce)
        except ValueError:
            continue
        raise AssertionError(bad)
    empty = posteriors.region_queries([], fwd, orig, cs, ce)
    assert empty[0].shape == (0, 2) and len(empty[1]) == 0


def test_region_queries_on_a_model_remap():
    e = synthetic.make_experiment(60, num_clones=3, max_copy_number=3, num_chains=4, seed=3)
    brk = H.add_shared_boundary_breakpoints(e)
    m = BreakpointModel(e.x, e.l, e.adjacencies, brk, max_copy_number=3, max_depth=1e9, quiet=True)
    assert m.N1 > m.N and not m.seg_is_original.all()
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    assert len(cs) >= 4 and cs[0] == 0 and ce[-1] == m.N1 - 1 and np.array_equal(cs[1:], ce[:-1] + 1)
    rng = np.random.RandomState(0)
    first = rng.randint(0, m.N, size=40); last = np.minimum(first + rng.randint(0, 25, size=40), m.N - 1)
    regions = np.stack([first, last], axis=1)
    runs, piece_region, constrain = posteriors.region_queries(regions, m.seg_fwd_remap, m.seg_is_original, cs, ce)
    assert np.array_equal(constrain.astype(bool), m.seg_is_original)
    chain_of = np.searchsorted(ce, np.arange(m.N1), side='left')
    multi = 0
    for i, (a, b) in enumerate(regions):
        mine = runs[piece_region == i]
        multi += len(mine) > 1
        covered = np.concatenate([np.arange(x, y + 1) for x, y in mine])
        assert np.array_equal(covered, np.arange(m.seg_fwd_remap[a], m.seg_fwd_remap[b] + 1))
        for x, y in mine:
            assert chain_of[x] == chain_of[y]
        assert len(mine) == len(set(chain_of[covered]))
    assert multi > 0
    regs, n = posteriors.adjacency_regions(m.seg_fwd_remap, m.is_telomere)
    assert sorted(n.tolist()) == sorted(a for a, b in e.adjacencies)


def test_record_round_trip_and_unchanged_when_unset():
    e = synthetic.make_experiment(40, num_clones=3, max_copy_number=4, num_chains=3, seed=2)
    ps = synthetic.make_init_params(e, 3, 4)
    rng = np.random.RandomState(0)
    names = ['negbin_r_0', 'negbin_r_1', 'betabin_M_0', 'betabin_M_1']
    N, M = len(e.x), 3
    brk_ids = list(e.breakpoints.keys())
    cn_regions = [('geneA', 3, 5), ('arm', 0, 30), ('one', 7, 7)]
    region_names, regions = posteriors.parse_regions(cn_regions)
    assert region_names == ['geneA', 'arm', 'one'] and regions.tolist() == [[3, 5], [0, 30], [7, 7]]
    plain = [_fake_result(e, rng) for _ in ps]
    with_regions = []
    for res in plain:
        r2 = dict(res, stats=dict(res['stats']))
        events = dict((k, rng.uniform(size=len(cn_regions))) for k in posteriors.REGION_ARRAYS)
        with_regions.append(posteriors.add_region_events(r2, region_names, events))
        assert sorted(r2['region_events']) == sorted(posteriors.REGION_ARRAYS + ('names',))
    assert len(posteriors.REGION_ARRAYS) == 7
    for a, b in zip(plain, with_regions):
        fa, ia = restarts._pack(a, N, M, len(brk_ids), 4, brk_ids, names)
        fb, ib = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=None)
        assert fa.tobytes() == fb.tobytes() and ia.tobytes() == ib.tobytes()
        assert len(fa) == restarts._HDR + M + 4 + 4 * N
        fc, ic = restarts._pack(b, N, M, len(brk_ids), 4, brk_ids, names, region_names=region_names)
        assert len(fc) == len(fa) + 7 * len(cn_regions) and fc[:len(fa)].tobytes() == fa.tobytes() and ic.tobytes() == ia.tobytes()
    off = restarts.gather_result_records(with_regions, e, ps, M, names)
    base = restarts.gather_result_records(plain, e, ps, M, names)
    for i, res in off.items():
        assert 'region_events' not in res and sorted(res) == sorted(base[i])
    on = restarts.gather_result_records(with_regions, e, ps, M, names, region_names=region_names)
    for i, res in on.items():
        src = with_regions[i]['region_events']
        assert res['region_events']['names'] == region_names
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(res['region_events'][k], src[k]), k
        assert np.array_equal(res['cn'], with_regions[i]['cn']) and res['stats']['elbo'] == with_regions[i]['stats']['elbo']
        assert sorted(set(res) - {'region_events'}) == sorted(off[i])
    # next to the other optional blocks of the record
    from remixt_amd import sampling
    full = []
    for res in with_regions:
        r3 = dict(res, stats=dict(res['stats']))
        summary = dict((k, rng.uniform(size=(N, M) if k.startswith('total_cn') else (N,))) for k in posteriors.COMPACT_ARRAYS)
        summary['expected_alleles_subclonal'] = rng.uniform(0, 2, size=N)
        posteriors.add_posterior_summary(r3, summary, e.l)
        full.append(r3)
    both = restarts.gather_result_records(full, e, ps, M, names, cn_posterior=True, region_names=region_names)
    for i, res in both.items():
        for k in posteriors.COMPACT_ARRAYS:
            assert np.array_equal(res[k], full[i][k]), k
        for k in posteriors.REGION_ARRAYS:
            assert np.array_equal(res['region_events'][k], full[i]['region_events'][k]), k
        assert res['stats'][posteriors.SUMMARY_STATS[0]] == full[i]['stats'][posteriors.SUMMARY_STATS[0]]
    assert sampling.SUMMARY_STATS      # (the sample block keeps its place: covered by tests/test_cn_samples_records_cpu.py)
