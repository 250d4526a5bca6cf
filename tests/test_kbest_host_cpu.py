"""CPU: the host-only pieces of rmx_region_kbest (rmxh::kbest_k_ok and rmxh::kbest_plan in remixt_amd/csrc/rmx_host.h), built
with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program (tests/csrc/kbest_host.cpp) that runs as a child
process: the rank rule, and the chunk plan at its extremes -- the program checks the plan's invariants itself (both budgets, the
layout of the staging buffer, no overflow).  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
OUT_BUDGET, BP_BUDGET = 64 << 20, 1 << 30


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('kbest') / 'kbest_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'kbest_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def test_rank_rule(harness):
    for K in (1, 2, 7, 8):
        assert harness('k', K) == 'ok'
    for K in (0, -1, 9, 16, 2 ** 31 - 1, -2 ** 31):
        assert harness('k', K) == 'refused'


def _plan(harness, nr, nq, S, K, max_len):
    out = harness('plan', nr, nq, S, K, max_len).split()
    assert out[0] == 'plan', out
    return dict(zip(('nrc', 'qc', 'strip', 'bp', 'states_at', 'queries_at', 'out'), (int(x) for x in out[1:])))


@pytest.mark.parametrize('nr', [1, 70000])
@pytest.mark.parametrize('nq', [1, 2 ** 31 - 1])
@pytest.mark.parametrize('K', [1, 8])
@pytest.mark.parametrize('S,max_len', [(1, 1), (1, 16384), (1024, 1), (1024, 16384), (355, 2), (165, 300)])
def test_plans(harness, nr, nq, S, K, max_len):
    p = _plan(harness, nr, nq, S, K, max_len)
    # (the program has checked the invariants; here: never less than one (restart, query), no chunk over either budget, and the
    # chunk as large as the budgets allow)
    assert 1 <= p['nrc'] <= min(nr, 65535) and 1 <= p['qc'] <= nq
    assert p['bp'] * 2 <= BP_BUDGET and p['out'] * 8 <= OUT_BUDGET
    strip_bytes, per_out = 2 * S * K * max_len, K * (8 + 2 * max_len)
    assert p['strip'] * 2 == strip_bytes
    if p['qc'] < nq:        # one more query would break a budget
        assert p['nrc'] * (p['qc'] + 1) * strip_bytes > BP_BUDGET or (p['qc'] + 1) * (p['nrc'] * per_out + 16) + 8 > OUT_BUDGET
    if p['nrc'] < min(nr, 65535):      # one more restart would break a budget even with one query
        assert (p['nrc'] + 1) * strip_bytes > BP_BUDGET or (p['nrc'] + 1) * per_out + 24 > OUT_BUDGET


def test_plan_examples(harness):
    # the largest strip: 256 MiB, four of them
    p = _plan(harness, 100, 100, 1024, 8, 16384)
    assert (p['nrc'], p['qc']) == (4, 1) and p['strip'] * 2 == 256 << 20
    assert _plan(harness, 1, 100, 1024, 8, 16384)['qc'] == 4
    # K = 1 is the decode plan's chunking
    assert _plan(harness, 100, 100, 1024, 1, 16384)['nrc'] == 32
    # small calls are one chunk
    p = _plan(harness, 4, 33, 165, 3, 21)
    assert (p['nrc'], p['qc']) == (4, 33) and p['strip'] == 165 * 3 * 21 and p['bp'] == 4 * 33 * 165 * 3 * 21
    assert p['states_at'] == 396 and p['queries_at'] == 396 + (396 * 21 * 2 + 7) // 8 and p['out'] == p['queries_at'] + 66


@pytest.mark.parametrize('args', [(0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1025, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 9, 1), (1, 1, 1, -1, 1),
                                  (1, 1, 1, 1, 0), (1, 1, 1, 1, 16385), (-1, 1, 1, 1, 1), (1, -5, 1, 1, 1)])
def test_plan_refusals(harness, args):
    assert harness('plan', *args) == 'refused 5'
