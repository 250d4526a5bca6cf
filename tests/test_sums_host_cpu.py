"""CPU: the host-only pieces of rmx_region_sums (rmxh::sums_max_bins, sums_lds_bytes, sum_increment, check_weights and
check_sum_spans in remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone
program (tests/csrc/sums_host.cpp) that runs as a child process: the bin table at its edges and against its Python mirror, the
saturating increment where a 32-bit product overflows, and the scans over arrays that hold exactly the entries given -- a read
past one is a heap overflow."""
import os
import subprocess

import pytest

from remixt_amd import posteriors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('sums') / 'sums_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'sums_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def _flat(values):
    return ','.join(str(int(v)) for v in values) or '-'


def test_bin_table_and_its_python_mirror(harness):
    for S, want in ((1, 64), (16, 64), (165, 64), (304, 64), (305, 32), (355, 32), (457, 32), (608, 32), (609, 16), (1024, 16), (1025, 0), (0, 0), (-1, 0),
                    (IMIN, 0), (IMAX, 0)):
        assert harness('bins', S) == str(want), S
        assert posteriors.sums_max_bins(S) == want, S
    for S in list(range(280, 330, 3)) + list(range(590, 630, 3)) + [1000, 1023]:
        assert int(harness('bins', S)) == posteriors.sums_max_bins(S), S


def test_lds_plan(harness):
    # SR (128 CT + 12) bytes, CT = 1, 2, 4 column tiles of 16 bins; 160 KiB with 64 bytes of static LDS hold the table's largest plans
    assert harness('lds', 165, 64) == str(176 * 524) and harness('lds', 165, 33) == str(176 * 524) and harness('lds', 165, 32) == str(176 * 268)
    assert harness('lds', 165, 17) == str(176 * 268) and harness('lds', 165, 16) == str(176 * 140) and harness('lds', 165, 1) == str(176 * 140)
    assert int(harness('lds', 304, 64)) + 64 <= 160 * 1024 < int(harness('lds', 305, 64)) + 64
    assert int(harness('lds', 608, 32)) + 64 <= 160 * 1024 < int(harness('lds', 609, 32)) + 64
    assert int(harness('lds', 1024, 16)) == 1024 * 140
    for S, nbins in ((165, 0), (165, 65), (165, -1), (0, 16), (1025, 16), (IMAX, IMAX), (IMIN, IMIN), (IMAX, 1), (1, IMAX)):
        assert harness('lds', S, nbins) == '0', (S, nbins)


def test_increment_saturates_in_64_bits(harness):
    assert harness('increment', 0, 5, 8) == '0' and harness('increment', 3, 0, 8) == '0' and harness('increment', 2, 3, 8) == '6'
    assert harness('increment', 7, 1, 8) == '7' and harness('increment', 4, 2, 8) == '7' and harness('increment', 1, 7, 8) == '7'
    assert harness('increment', 9, 9, 1) == '0' and harness('increment', 0, 0, 1) == '0'
    assert harness('increment', IMAX, 32767, 64) == '63' and harness('increment', IMAX, 1, 64) == '63' and harness('increment', 65536, 32767, 64) == '63'
    assert harness('increment', 65536, 32768, 64) == '63'               # 2^31: a 32-bit product would be negative
    assert harness('increment', IMAX, IMAX, IMAX) == str(IMAX - 1) and harness('increment', 46341, 46341, IMAX) == str(IMAX - 1)
    assert harness('increment', 46340, 46340, IMAX) == str(46340 * 46340)


def test_weights(harness):
    assert harness('weights', 5, '0,1,2,3,%d' % IMAX) == '-1'
    assert harness('weights', 5, '0,-1,2,-3,4') == '1' and harness('weights', 5, '0,1,2,3,%d' % IMIN) == '4' and harness('weights', 1, '-1') == '0'
    assert harness('weights', 0, '-') == '-1' and harness('weights', 3, '-') == '-2' and harness('weights', -1, '-') == '-2' and harness('weights', -1, '1') == '-2'
    many = list(range(5000))
    assert harness('weights', 5000, _flat(many)) == '-1' and harness('weights', 5000, _flat(many[:-1] + [-7])) == '4999'


def test_spans(harness):
    q = [0, 3, 0, 0, 2, 2, 1, 4, 5, 9, 0, 5]                          # spans 0 .. 3, 4 .. 4, 5 .. 9
    assert harness('spans', 3, 10, _flat(q)) == '-1'
    assert harness('spans', 3, 9, _flat(q)) == '2' and harness('spans', 3, 4, _flat(q)) == '1' and harness('spans', 3, 3, _flat(q)) == '0'
    bad = list(q)
    bad[7] = -1
    assert harness('spans', 3, 10, _flat(bad)) == '1'
    bad = list(q)
    bad[0], bad[1] = 3, 0
    assert harness('spans', 3, 10, _flat(bad)) == '0'                   # a > b
    # no overflow at the ends of int32
    assert harness('spans', 1, IMAX, _flat([0, IMAX, 0, IMAX])) == '0' and harness('spans', 1, IMAX, _flat([IMIN, IMAX, 0, IMAX])) == '0'
    assert harness('spans', 1, IMAX, _flat([5, 5, 0, IMAX - 1])) == '-1' and harness('spans', 1, IMAX, _flat([5, 5, 0, IMAX])) == '0'
    assert harness('spans', 1, 2 ** 40, _flat([0, IMAX, 0, IMAX])) == '-1'
    assert harness('spans', 1, 0, _flat([0, 0, 0, 0])) == '0'
    assert harness('spans', 0, 10, '-') == '-1' and harness('spans', 2, 10, '-') == '-2' and harness('spans', -1, 10, '-') == '-2' and harness('spans', 1, -1, _flat([0, 0, 0, 0])) == '-2'
    many = [v for i in range(2000) for v in (i, i + 3, 0, 4 * i)]
    assert harness('spans', 2000, 4 * 1999 + 4, _flat(many)) == '-1' and harness('spans', 2000, 4 * 1999 + 3, _flat(many)) == '1999'
