"""CPU: the host-only pieces of rmx_region_extremes (rmxh::extremes_ncol_ok and rmxh::check_levels in
remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/csrc/extremes_host.cpp) that runs as a child process: the column rule at its edges, and the level scan over tables
whose array holds exactly the entries given -- a read past the table is a heap overflow."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('extremes') / 'extremes_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'extremes_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def _flat(values):
    return ','.join(str(int(v)) for v in values) or '-'


@pytest.mark.parametrize('ncol,want', [(1, 'ok'), (5, 'ok'), (16, 'ok'), (0, 'bad'), (17, 'bad'), (-1, 'bad'), (2 ** 31 - 1, 'bad'), (-2 ** 31, 'bad')])
def test_column_rule(harness, ncol, want):
    assert harness('ncol', ncol) == want


def test_level_scan(harness):
    assert harness('levels', 2, 3, 4, _flat(range(24))) == 'ok'
    assert harness('levels', 1, 1, 1, '0') == 'ok' and harness('levels', 1, 1, 1, '32767') == 'ok'
    assert harness('levels', 1, 1, 1, '-1') == 'bad 0'
    assert harness('levels', 2, 3, 4, _flat([0] * 23 + [-1])) == 'bad 23'              # the last entry of the last table
    assert harness('levels', 2, 3, 4, _flat([0] * 7 + [-32768] + [-1] * 16)) == 'bad 7'  # the first one is reported
    # a table without entries has nothing to refuse; negative extents describe no table
    assert harness('levels', 0, 3, 4, '-') == 'ok' and harness('levels', 2, 0, 4, '-') == 'ok' and harness('levels', 2, 3, 0, '-') == 'ok'
    assert harness('levels', -1, 3, 4, '-') == 'refused' and harness('levels', 2, -3, 4, '-') == 'refused' and harness('levels', 2, 3, -4, '-') == 'refused'
    # 1024 states, 16 tables, two classes
    n = 2 * 16 * 1024
    assert harness('levels', 2, 16, 1024, _flat([i % 16 for i in range(n)])) == 'ok'
    assert harness('levels', 2, 16, 1024, _flat([i % 16 if i != n - 2 else -5 for i in range(n)])) == 'bad %d' % (n - 2)
