"""CPU: the host-only checks of rmx_restart_overlap (rmxh::check_pairs and rmxh::check_permutations in
remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/csrc/overlap_host.cpp) that runs as a child process: the pair check at the edges of both batches, and the bijection
check over tables whose array holds exactly the entries given -- a read past the table, or a mark written at an entry equal
to S, is a heap overflow."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('overlap') / 'overlap_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'overlap_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def _flat(values):
    return ','.join(str(int(v)) for v in values) or '-'


def test_pair_check(harness):
    assert harness('pairs', 3, 2, _flat([0, 0, 2, 1, 1, 1])) == 'ok'
    assert harness('pairs', 1, 1, '0,0') == 'ok'
    assert harness('pairs', 3, 2, _flat([0, 0, 3, 1])) == 'bad 1'          # A's index equal to its batch's count
    assert harness('pairs', 3, 2, _flat([0, 2, 0, 0])) == 'bad 0'          # B's
    assert harness('pairs', 3, 2, _flat([0, 0, 0, 1, -1, 0])) == 'bad 2' and harness('pairs', 3, 2, _flat([2, -1])) == 'bad 0'
    assert harness('pairs', 3, 2, _flat([2 ** 31 - 1, 0])) == 'bad 0' and harness('pairs', 3, 2, _flat([0, -2 ** 31])) == 'bad 0'
    # the B side is checked against B's count, not A's
    assert harness('pairs', 2, 5, _flat([1, 4])) == 'ok' and harness('pairs', 5, 2, _flat([1, 4])) == 'bad 0'
    # no pair, or no restarts, describes no list
    assert harness('pairs', 3, 2, '-') == 'refused' and harness('pairs', -1, 2, '0,0') == 'refused' and harness('pairs', 0, 0, '0,0') == 'bad 0'


def test_bijection_check(harness):
    # S = 1: the one permutation
    assert harness('perms', 1, 1, 1, '0') == 'ok' and harness('perms', 3, 2, 1, _flat([0] * 6)) == 'ok'
    assert harness('perms', 1, 1, 1, '1') == 'bad 0' and harness('perms', 1, 1, 1, '-1') == 'bad 0'      # an index equal to S
    assert harness('perms', 2, 1, 1, '0,1') == 'bad 1'
    # small tables: a repeated index, an index equal to S, in the last row of the last table
    assert harness('perms', 2, 2, 3, _flat([0, 1, 2, 2, 0, 1, 1, 2, 0, 2, 1, 0])) == 'ok'
    assert harness('perms', 2, 2, 3, _flat([0, 1, 2, 2, 0, 1, 1, 2, 0, 2, 1, 1])) == 'bad 3'
    assert harness('perms', 2, 2, 3, _flat([0, 1, 2, 2, 0, 1, 1, 2, 0, 2, 1, 3])) == 'bad 3'
    assert harness('perms', 2, 2, 3, _flat([0, 0, 2, 2, 0, 1, 1, 2, 0, 2, 1, 3])) == 'bad 0'             # the first one is reported
    assert harness('perms', 1, 1, 3, _flat([0, 1, -32768])) == 'bad 0' and harness('perms', 1, 1, 3, _flat([32767, 1, 0])) == 'bad 0'
    # nothing to check describes no table
    for args in ((0, 1, 3), (1, 0, 3), (1, 1, 0), (-1, 1, 3), (1, -1, 3), (1, 1, -3)):
        assert harness('perms', *args, '-') == 'refused', args
    # S = 1024, two maps, two classes: the cyclic shifts; one entry repeated, one equal to S, each at the table's very end
    assert harness('shift', 2, 2, 1024, -1, 0, 0) == 'ok'
    assert harness('shift', 2, 2, 1024, 3, 1023, 5) == 'bad 3'             # repeats an index of its row (1023 + 3 mod 1024 = 2 was there)
    assert harness('shift', 2, 2, 1024, 3, 1023, 1024) == 'bad 3'          # an index equal to S
    assert harness('shift', 2, 2, 1024, 0, 0, 1024) == 'bad 0' and harness('shift', 2, 2, 1024, 1, 512, -1) == 'bad 1'
    assert harness('shift', 1, 1, 1024, 0, 1023, 1023) == 'ok'             # (the identity's own entry)
