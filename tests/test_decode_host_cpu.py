"""CPU: the host-only pieces of rmx_region_decode (rmxh::check_decode_lengths and rmxh::decode_plan in
remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/csrc/decode_host.cpp) that runs as a child process: every refusal of the length rules, and the chunk plan at its
extremes -- the program checks the plan's invariants itself (both budgets, the layout of the staging buffer, no overflow)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
OUT_BUDGET, BP_BUDGET = 64 << 20, 1 << 30


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('decode') / 'decode_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'decode_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def _flat(rows):
    return ','.join(str(int(x)) for row in rows for x in row) or '-'


def test_valid_lengths(harness):
    assert harness('check', 1, _flat([(3, 3, -1, -1)])) == 'ok'
    assert harness('check', 4, _flat([(0, 3, 0, 1), (7, 7, -1, 2), (5, 8, 1, -1)])) == 'ok'
    assert harness('check', 16384, _flat([(0, 16383, -1, -1), (100, 16483, 0, 0)])) == 'ok'
    assert harness('check', 5, '-') == 'ok'                         # no queries: nothing to refuse (the entry point refuses nq < 1)
    assert harness('check', 16384, _flat([(2 ** 31 - 1, 2 ** 31 - 1, 0, 0)])) == 'ok'


@pytest.mark.parametrize('max_len,queries,bad,reason', [
    (0, [(0, 0, -1, -1)], 0, 'max_len must be in [1, 16384]'),
    (-1, [(0, 0, -1, -1)], 0, 'max_len must be in [1, 16384]'),
    (16385, [(0, 0, -1, -1)], 0, 'max_len must be in [1, 16384]'),
    (2 ** 31 - 1, [(0, 0, -1, -1)], 0, 'max_len must be in [1, 16384]'),
    (-2 ** 31, [], 0, 'max_len must be in [1, 16384]'),
    (1, [(0, 1, -1, -1)], 0, 'longer than max_len'),
    (3, [(0, 2, -1, -1), (4, 7, 0, 0)], 1, 'longer than max_len'),
    (16384, [(0, 16384, -1, -1)], 0, 'longer than max_len'),
    (16384, [(-2 ** 31, 2 ** 31 - 1, -1, -1)], 0, 'longer than max_len'),      # b - a + 1 does not fit an int32
    (4, [(0, 1, 0, 0), (3, 2, 0, 0)], 1, 'first <= last'),
    (4, [(2 ** 31 - 1, -2 ** 31, 0, 0)], 0, 'first <= last'),
])
def test_refusals(harness, max_len, queries, bad, reason):
    out = harness('check', max_len, _flat(queries))
    assert out.startswith('bad %d ' % bad) and reason in out, out


def _plan(harness, nr, nq, S, max_len):
    out = harness('plan', nr, nq, S, max_len).split()
    assert out[0] == 'plan', out
    return dict(zip(('nrc', 'qc', 'strip', 'bp', 'states_at', 'queries_at', 'out'), (int(x) for x in out[1:])))


@pytest.mark.parametrize('nr', [1, 2, 64, 65535, 65536, 2 ** 31 - 1])
@pytest.mark.parametrize('nq', [1, 3, 20000, 2 ** 31 - 1])
@pytest.mark.parametrize('S,max_len', [(1, 1), (1, 16384), (1024, 1), (1024, 16384), (355, 2), (165, 300)])
def test_plans(harness, nr, nq, S, max_len):
    p = _plan(harness, nr, nq, S, max_len)
    # (the program has checked the invariants; here: the chunk is as large as the budgets allow, and never empty)
    assert 1 <= p['nrc'] <= min(nr, 65535) and 1 <= p['qc'] <= nq
    assert p['bp'] * 2 <= BP_BUDGET and p['out'] * 8 <= OUT_BUDGET
    strip_bytes, per_out = 2 * S * max_len, 8 + 2 * max_len
    if p['qc'] < nq:        # one more query would break a budget
        assert p['nrc'] * (p['qc'] + 1) * strip_bytes > BP_BUDGET or (p['qc'] + 1) * (p['nrc'] * per_out + 16) + 8 > OUT_BUDGET
    if p['nrc'] < min(nr, 65535):      # one more restart would break a budget even with one query
        assert (p['nrc'] + 1) * strip_bytes > BP_BUDGET or (p['nrc'] + 1) * per_out + 24 > OUT_BUDGET


def test_plan_examples(harness):
    # the largest strip: 32 MiB, 32 of them
    assert _plan(harness, 100, 100, 1024, 16384)['nrc'] == 32 and _plan(harness, 100, 100, 1024, 16384)['qc'] == 1
    assert _plan(harness, 1, 100, 1024, 16384)['qc'] == 32
    # small calls are one chunk
    p = _plan(harness, 4, 33, 165, 21)
    assert (p['nrc'], p['qc']) == (4, 33) and p['strip'] == 165 * 21 and p['bp'] == 4 * 33 * 165 * 21
    assert p['states_at'] == 132 and p['queries_at'] == 132 + (132 * 21 * 2 + 7) // 8 and p['out'] == p['queries_at'] + 66


@pytest.mark.parametrize('args', [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1025, 1), (1, 1, 1, 0), (1, 1, 1, 16385), (-1, 1, 1, 1), (1, -5, 1, 1)])
def test_plan_refusals(harness, args):
    assert harness('plan', *args) == 'refused 5'
