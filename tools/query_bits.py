"""The raw outputs of the posterior queries on seeded scenarios, for comparing two builds of the library to the last bit:
sample_states, posterior_summary_raw, region_logprob_raw, region_counts_raw (1, 5 and 16 bins), call_logprob_raw,
region_moments_raw (nf 1 and 4), region_extent_raw, region_pattern_raw, region_decode_raw (log-probabilities and states),
region_kbest_raw (1, 3 and 8 ranks; log-probabilities and states), region_extremes_raw (1, 5 and 16 columns) and region_conditional_raw (log-probabilities and slots; chain windows), each with
and without a constrain vector that leaves segments unbound, locus_joint_raw (three table sizes and the profile form), and
region_automaton_raw (three automata padded to 16 states, with and without the constrain vector, in the 165-state and the
617-state scenario), path_entropy_raw (both arrays over all segments, in the same two scenarios) and region_sums_raw (a mask and
a copy-number table under three weightings, one saturating: 16 and 64 bins at 165 states, 16 bins in the 617-state scenario, the
16-tile form); a library without an entry point leaves its arrays out.
Scenarios: the three grids of tests/test_hip_sample_cn.py (60, 40 and 24 segments at 165, 355 and 457 states) and 16 segments at
max_copy_number 16 (more than 512 states: the <16> instantiations), three chains, four restarts after two sweeps, restarts 1 and 2
with their snapshot retaken under the other transition model (exp(trans_value) on plain adjacencies too).  Queries: a segment, a
pair, every whole chain, a run from a chain start and one to a chain end, a pair across every kind of adjacency the scenario has;
anchors at a chain's first, middle and last segment and on both sides of a breakend adjacency.
Usage: python tools/query_bits.py OUT.npz            (RMX_LIB_PATH selects the library, one fresh process per library)
       python tools/query_bits.py --compare A.npz B.npz   (A: the older build.  np.array_equal(equal_nan=True) per array both files hold;
                                                           arrays of one file alone are listed; exit status 1 if a shared array
                                                           differs or B lacks an array of A)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

GRIDS = [(60, 3, 8), (40, 3, 12), (24, 4, 6), (16, 3, 16)]
R = 4
CONSTRAINTS = ((-1, -1), (1, -1), (-1, 1), (5, 2), (0, 0))       # (mask, label) indices


def compare(fa, fb):
    a, b = np.load(fa), np.load(fb)
    # A is the older build: an array B adds is listed, an array B lacks fails the comparison
    same = not (set(a.files) - set(b.files))
    for f, x, y in ((fa, a, b), (fb, b, a)):
        if set(x.files) - set(y.files):
            print('only in %s: %s' % (f, sorted(set(x.files) - set(y.files))))
    for k in sorted(set(a.files) & set(b.files)):
        eq = a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f')
        fin = int(np.isfinite(a[k]).sum()) if a[k].dtype.kind == 'f' else a[k].size
        print('%-28s %-18s %7d finite or integer entries: %s' % (k, a[k].shape, fin, 'equal' if eq else 'DIFFERS'))
        same = same and eq
    print('every array of the first file equal in the second' if same else 'NOT EQUAL')
    return 0 if same else 1


def open_scenario(N, M, max_cn):
    """The fitted RestartSet of a scenario (the caller closes it)."""
    from remixt_amd import synthetic
    from remixt_amd.restarts import RestartSet
    e = synthetic.make_experiment(N, num_clones=M, max_copy_number=max_cn, num_chains=3, seed=0)
    ps = synthetic.make_init_params(e, R, max_cn, num_clones=M)
    fr = (0.6, 0.4) if M == 3 else (0.5, 0.3, 0.2)
    hs = [np.array([p['h_normal']] + [p['h_tumour'] * f for f in fr]) for p in ps]
    rs = RestartSet(e, ps, max_cn, num_clones=M, quiet=True, seeds=list(range(R)), h_init=hs)
    try:
        b = rs.batch
        # the sweeps run on the total read counts alone: a state and its allele swap tie, so probabilities are not all 0 or 1
        for r in range(R):
            b.set_array(r, 'allele_likelihood_mask', np.zeros(b.num_segments, dtype=np.int64))
        rs.variational_update(2)
        b.transition_model = 1
        b.update_p_cn(1, 3)
    except Exception:
        rs.close()
        raise
    return rs


def collect(rs, out, kbest=True):
    """Every query's raw outputs on an open scenario -> out (kbest=False: without region_kbest_raw's, the list of the builds
    before that call; tests/test_hip_region_kbest.py holds that a call leaves every one of them unchanged)."""
    from remixt_amd import posteriors
    b, m = rs.batch, rs.models[0]
    N1, S = b.num_segments, b.num_cn_states
    masks, labels = posteriors.event_tables(b.cn_classes)
    cs, ce = posteriors.chains_from_telomeres(m.is_telomere)
    bidx = np.asarray(m.breakpoint_idx)
    inner = np.ones(N1 - 1, dtype=bool); inner[ce[:-1]] = False
    plain, be = np.flatnonzero(inner & (bidx[:-1] < 0)), np.flatnonzero(inner & (bidx[:-1] >= 0))
    c = int(np.argmax(ce - cs))
    mid = int((cs[c] + ce[c]) // 2)
    runs = [(mid, mid), (mid, min(mid + 1, int(ce[c])))] + [(int(a), int(z)) for a, z in zip(cs, ce)]
    runs += [(int(cs[1]), int(min(cs[1] + 3, ce[1]))), (int(max(ce[0] - 2, cs[0])), int(ce[0]))]
    runs += [(int(n), int(n) + 1) for n in list(plain[:1]) + list(be[:2])]
    anchors = [int(cs[c]), mid, int(ce[c])] + [int(n) + k for n in be[:1] for k in (0, 1)]
    bound = np.asarray(m.seg_is_original, dtype=bool).copy()
    bound[2::5] = False
    qr = np.array([[a, z, mi, li] for a, z in runs for mi, li in CONSTRAINTS], dtype=np.int32)
    qc = np.array([[a, z, mi, li] for a, z in runs for mi, li in ((-1, 0), (1, 1), (5, 2))], dtype=np.int32)
    qp = np.array([[a, z, li, 0] for a, z in runs for li in (-1, 0, 1, 2)], dtype=np.int32)
    qx = np.array([[n0, mi, li, 0] for n0 in anchors for mi, li in CONSTRAINTS], dtype=np.int32)
    # patterns: every run alone, its two ends as one-segment pieces, and per chain three pieces with a gap and a touching pair
    pt = [[a, z, mi, li] for a, z in runs for mi, li in CONSTRAINTS]
    qt = [[i, 1, 0, 0] for i in range(len(pt))]
    for a, z in runs:
        if z > a:
            qt.append([len(pt), 2, 0, 0]); pt += [[a, a, 1, -1], [z, z, 5, 2]]
    for a, z in zip(cs, ce):
        a, z = int(a), int(z)
        if z - a >= 6:
            qt.append([len(pt), 3, 0, 0]); pt += [[a, a + 1, -1, 0], [a + 3, a + 4, 1, 1], [a + 5, z, 5, -1]]
    qt, pt = np.array(qt, dtype=np.int32), np.array(pt, dtype=np.int32)
    feats = posteriors.moment_features(b.cn_classes)
    weights = np.stack([np.asarray(m.l1, dtype=float), np.ones(N1)])
    qm1 = np.array([[a, z, f0, wi] for a, z in runs for f0, wi in ((0, 0), (feats.shape[1] - 1, 1))], dtype=np.int32)
    qm4 = np.array([[a, z, 0, wi] for a, z in runs for wi in (0, 1)], dtype=np.int32)
    key = lambda name: 'S%d_%s' % (S, name)
    out[key('sample_states')] = b.sample_states(0, R, 9, [11, 12, 13, 14])
    proj, stats, argmax = b.posterior_summary_raw(0, R, weights=np.ascontiguousarray(np.transpose(masks, (0, 2, 1)).astype(float)))
    out[key('summary_proj')], out[key('summary_stats')], out[key('summary_argmax')] = proj, stats, argmax
    paths = argmax.astype(np.int16)[:, None]
    for tag, con in (('all', None), ('unbound', bound)):
        out[key('region_logprob_' + tag)] = b.region_logprob_raw(0, R, qr, masks, labels, con)
        for K in (1, 5, 16):
            out[key('region_counts%d_%s' % (K, tag))] = b.region_counts_raw(0, R, qc, masks, labels, con, K)
        out[key('call_logprob_' + tag)] = b.call_logprob_raw(0, R, paths, qp, labels, con)
        out[key('region_extent_' + tag)] = b.region_extent_raw(0, R, qx, masks, labels, con, 6, 6)
        if hasattr(b, 'region_pattern_raw'):
            out[key('region_pattern_' + tag)] = b.region_pattern_raw(0, R, qt, pt, masks, labels, con)
        if hasattr(b, 'region_decode_raw'):
            out[key('region_decode_logp_' + tag)], out[key('region_decode_states_' + tag)] = b.region_decode_raw(0, R, qr, masks, labels, con)
        if kbest and hasattr(b, 'region_kbest_raw'):
            for K in (1, 3, 8):
                out[key('region_kbest%d_logp_%s' % (K, tag))], out[key('region_kbest%d_states_%s' % (K, tag))] = b.region_kbest_raw(0, R, qr, K, masks, labels, con)
        if hasattr(b, 'region_extremes_raw'):
            for K in (1, 5, 16):
                levels, names = posteriors.level_tables(b.cn_classes, K)
                qe = np.array([[a, z, mi, names.index(lv)] for a, z in runs
                               for mi, lv in ((-1, 'peak_total_1'), (1, 'peak_total_any'), (5, 'floor_total_1'), (-1, 'floor_minor_any'))], dtype=np.int32)
                out[key('region_extremes%d_%s' % (K, tag))] = b.region_extremes_raw(0, R, qe, masks, levels, con, K)
        if hasattr(b, 'region_conditional_raw'):
            cw, _ = posteriors.feature_matrix(b.cn_classes)
            win = np.array([(cs[np.searchsorted(ce, a)], ce[np.searchsorted(ce, a)]) for a in qr[:, 0]], dtype=np.int32)
            out[key('region_conditional_logp_' + tag)], out[key('region_conditional_' + tag)] = b.region_conditional_raw(
                0, R, qr, win, masks, labels, con, cw, argmax)
    if hasattr(b, 'locus_joint_raw'):
        lv, ln = posteriors.locus_level_tables(b.cn_classes, 16)
        ql = np.array([[a, z, ln.index(vr), ln.index(vc)] for a, z in runs
                       for vr, vc in (('peak_total_any', 'peak_total_any'), ('peak_total_1', 'peak_major_2'), ('loh', 'peak_total_any'))], dtype=np.int32)
        for nrow, ncol in ((1, 1), (5, 16), (16, 16)):
            out[key('locus_joint%dx%d' % (nrow, ncol))] = b.locus_joint_raw(0, R, ql, lv, nrow, ncol)
        out[key('locus_joint_profile')] = b.locus_joint_raw(0, R, ql, lv, 16, 16, int((ql[:, 1] - ql[:, 0]).max()) + 1)
    if hasattr(b, 'region_automaton_raw') and (S == 165 or S > 512):      # (the 3-tile and the 16-tile form)
        aus = (posteriors.automaton_runs(8), posteriors.automaton_run_of(3), posteriors.automaton_switches(7))
        dl = np.zeros((len(aus), 16, 3), dtype=np.uint8)
        for i, au in enumerate(aus):
            dl[i, :au.delta.shape[0], :au.alphabet] = au.delta
        sy = np.stack([posteriors.symbols_from(b.cn_classes, ['loh']), posteriors.symbols_from(b.cn_classes, ['subclonal']),
                       posteriors.symbols_from(b.cn_classes, [posteriors.level_mask(b.cn_classes, 'total', 'any', 0, 2), posteriors.level_mask(b.cn_classes, 'total', 'any', 3, 99)])], axis=1)
        qa = np.array([[a, z, i, i] for a, z in runs for i in range(len(aus))], dtype=np.int32)
        for tag, con in (('all', None), ('unbound', bound)):
            out[key('region_automaton_' + tag)] = b.region_automaton_raw(0, R, qa, sy, dl, np.zeros(len(aus), dtype=np.int32), con)
    if hasattr(b, 'path_entropy_raw') and (S == 165 or S > 512):      # (the 3-tile and the 16-tile form; restarts 1 and 2 on exp(Tval))
        out[key('path_entropy_marginal')], out[key('path_entropy_step')] = b.path_entropy_raw(0, R)
    if hasattr(b, 'region_sums_raw') and (S == 165 or S > 512):      # (three row tiles at 16 and 64 bins; the 16-tile form at 16 bins)
        lt = np.stack([masks[:, 1].astype(np.int16), posteriors._level_quantity(b.cn_classes, 'total').max(axis=-1).astype(np.int16)], axis=1)
        pool = np.concatenate([bound.astype(np.int32), np.arange(N1, dtype=np.int32) % 4, [2 ** 31 - 1]])
        # weights: seg_is_original with segments left out, 0 .. 3 by position, and the run's last segment on the saturating entry
        qs = np.array([[a, z, li, off] for a, z in runs for li in (0, 1) for off in (a, N1 + a, 2 * N1 - (z - a))], dtype=np.int32)
        for bins in sorted({16, posteriors.sums_max_bins(S)}):
            out[key('region_sums%d' % bins)] = b.region_sums_raw(0, R, qs, lt, pool, bins)
    out[key('region_moments1')] = b.region_moments_raw(0, R, qm1, feats, weights, 1)
    out[key('region_moments4')] = b.region_moments_raw(0, R, qm4, feats, weights, 4)
    print('%d states, %d model segments, %d chains, %d plain and %d breakend adjacencies, %d runs, %d anchors, %d of %d segments unbound' % (
        S, N1, len(cs), len(plain), len(be), len(runs), len(anchors), (~bound).sum(), N1), flush=True)


def scenario(N, M, max_cn, out):
    rs = open_scenario(N, M, max_cn)
    try:
        collect(rs, out)
    finally:
        rs.close()


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    out = {}
    for N, M, max_cn in GRIDS:
        scenario(N, M, max_cn, out)
    np.savez(sys.argv[1], **out)
    print('%d arrays -> %s' % (len(out), sys.argv[1]))
