"""CPU: the host-only pieces of rmx_locus_joint (rmxh::locus_shape_ok and rmxh::check_locus_lengths in
remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/csrc/locus_host.cpp) that runs as a child process: the table and slot rule at its edges, and the length scan over
query arrays that hold exactly the entries given -- a read past the array is a heap overflow."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('locus') / 'locus_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'locus_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def _flat(queries):
    return ','.join(str(int(v)) for q in queries for v in q) or '-'


@pytest.mark.parametrize('n,want', [(0, 'bad'), (1, 'ok'), (16, 'ok'), (17, 'bad'), (IMIN, 'bad'), (IMAX, 'bad')])
def test_rows_and_columns(harness, n, want):
    assert harness('shape', n, 5, 0) == want and harness('shape', 5, n, 0) == want
    assert harness('shape', n, 5, 7) == want and harness('shape', 5, n, 7) == want
    assert harness('shape', n, n, 4096) == want


@pytest.mark.parametrize('nslot,want', [(-1, 'bad'), (0, 'ok'), (1, 'ok'), (4096, 'ok'), (4097, 'bad'), (IMIN, 'bad'), (IMAX, 'bad')])
def test_slots(harness, nslot, want):
    assert harness('shape', 1, 1, nslot) == want and harness('shape', 16, 16, nslot) == want


def test_the_product(harness):
    # the largest table, 4096 slots of 16 x 16, is 2^20 entries exactly; no int32 triple overflows on the way
    assert harness('shape', 16, 16, 4096) == 'ok' and 4096 * 16 * 16 == 2 ** 20
    assert harness('shape', 16, 16, 4097) == 'bad' and harness('shape', 17, 16, 4096) == 'bad' and harness('shape', 16, 17, 4096) == 'bad'
    assert harness('shape', IMAX, IMAX, IMAX) == 'bad' and harness('shape', IMIN, IMIN, IMIN) == 'bad' and harness('shape', IMAX, IMAX, 0) == 'bad'


def test_lengths(harness):
    ok = [(3, 3, 0, 1), (0, 6, 1, 0), (10, 16, 0, 0)]
    assert harness('lengths', 7, _flat(ok)) == 'ok'
    # one longer than nslot: t - a + 1 = 8
    assert harness('lengths', 7, _flat(ok + [(2, 9, 0, 0)])) == 'bad 3: a profile query is longer than nslot'
    assert harness('lengths', 7, _flat([(2, 9, 0, 0)] + ok)) == 'bad 0: a profile query is longer than nslot'      # the first one is reported
    assert harness('lengths', 8, _flat(ok + [(2, 9, 0, 0)])) == 'ok'
    assert harness('lengths', 1, _flat([(5, 5, 0, 0)])) == 'ok' and harness('lengths', 1, _flat([(5, 6, 0, 0)])).startswith('bad 0')
    # the pair form has no slots to fit
    assert harness('lengths', 0, _flat(ok + [(0, IMAX, 0, 0)])) == 'ok'
    assert harness('lengths', 0, _flat([(4, 3, 0, 0)])) == 'bad 0: a query needs first <= last'
    assert harness('lengths', 4096, _flat([(IMIN, IMAX, 0, 0)])) == 'bad 0: a profile query is longer than nslot'      # (no overflow)
    assert harness('lengths', 4096, _flat([(0, 4095, 0, 0)])) == 'ok' and harness('lengths', 4096, _flat([(0, 4096, 0, 0)])).startswith('bad 0')
    assert harness('lengths', -1, _flat(ok)) == 'bad 0: nslot must be in [0, 4096]' and harness('lengths', 4097, _flat(ok)).startswith('bad 0: nslot')
    # no queries: nothing to refuse
    assert harness('lengths', 7, '-') == 'ok'
    # a query array that holds exactly the entries given: 3000 queries, the last one too long
    many = [(i, i + i % 7, 0, 0) for i in range(3000)]
    assert harness('lengths', 7, _flat(many)) == 'ok'
    assert harness('lengths', 7, _flat(many[:-1] + [(2999, 3006, 0, 0)])) == 'bad 2999: a profile query is longer than nslot'
