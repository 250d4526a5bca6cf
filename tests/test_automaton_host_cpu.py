"""CPU: the host-only pieces of rmx_region_automaton (rmxh::automaton_shape_ok, rmxh::check_automata and rmxh::check_symbols in
remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/csrc/automaton_host.cpp) that runs as a child process: the shape rule at its edges, and the scans over tables that
hold exactly the entries given -- a read past a table is a heap overflow."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('automaton') / 'automaton_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'automaton_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def _flat(values):
    return ','.join(str(int(v)) for v in values) or '-'


@pytest.mark.parametrize('n,want', [(0, 'bad'), (1, 'ok'), (16, 'ok'), (17, 'bad'), (-1, 'bad'), (IMIN, 'bad'), (IMAX, 'bad')])
def test_states_and_symbols(harness, n, want):
    assert harness('shape', 1, n, 5) == want and harness('shape', 64, 5, n) == want and harness('shape', 3, n, n) == want


@pytest.mark.parametrize('nauto,want', [(0, 'bad'), (1, 'ok'), (64, 'ok'), (65, 'bad'), (-1, 'bad'), (IMIN, 'bad'), (IMAX, 'bad')])
def test_number_of_automata(harness, nauto, want):
    assert harness('shape', nauto, 1, 1) == want and harness('shape', nauto, 16, 16) == want


def test_automata(harness):
    # two automata of three states over two symbols
    delta = [0, 1, 2, 0, 1, 1, 2, 2, 2, 2, 0, 0]
    assert harness('automata', 2, 3, 2, _flat(delta), '0,2') == '-1'
    for i in (0, 5, 11):                    # the first, one in the middle, the very last entry: Q itself is outside
        bad = list(delta)
        bad[i] = 3
        assert harness('automata', 2, 3, 2, _flat(bad), '0,2') == str(i)
    two = list(delta)
    two[4] = two[9] = 255
    assert harness('automata', 2, 3, 2, _flat(two), '0,2') == '4'                      # the first one is reported
    # start states: reported behind the transitions
    assert harness('automata', 2, 3, 2, _flat(delta), '3,0') == '12' and harness('automata', 2, 3, 2, _flat(delta), '0,-1') == '13'
    assert harness('automata', 2, 3, 2, _flat(delta), '%d,%d' % (IMAX, IMIN)) == '12'
    # the largest tables, every entry the largest state
    assert harness('automata', 64, 16, 16, _flat([15] * (64 * 256)), _flat([15] * 64)) == '-1'
    assert harness('automata', 64, 16, 16, _flat([15] * (64 * 256 - 1) + [16]), _flat([15] * 64)) == str(64 * 256 - 1)
    assert harness('automata', 64, 16, 16, _flat([15] * (64 * 256)), _flat([15] * 63 + [16])) == str(64 * 256 + 63)
    # Q = 1: only state 0
    assert harness('automata', 1, 1, 1, '0', '0') == '-1' and harness('automata', 1, 1, 1, '1', '0') == '0' and harness('automata', 1, 1, 1, '0', '1') == '1'
    # a shape outside the rule or a missing pointer describes no tables: nothing is read
    for shape in ((0, 3, 2), (65, 3, 2), (2, 0, 2), (2, 17, 2), (2, 3, 0), (2, 3, 17), (IMAX, IMAX, IMAX), (IMIN, 1, 1)):
        assert harness('automata', *shape, _flat(delta), '0,2') == '-2', shape
    assert harness('automata', 2, 3, 2, '-', '0,2') == '-2' and harness('automata', 2, 3, 2, _flat(delta), '-') == '-2'


def test_symbols(harness):
    sym = [0, 1, 2, 3, 3, 2, 1, 0, 0, 0, 3, 3]                       # 2 classes x 2 tables x 3 states
    assert harness('symbols', 2, 2, 3, 4, _flat(sym)) == '-1'
    assert harness('symbols', 2, 2, 3, 3, _flat(sym)) == '3'          # A itself is outside; the first one is reported
    for i in (0, 7, 11):
        bad = list(sym)
        bad[i] = -1
        assert harness('symbols', 2, 2, 3, 4, _flat(bad)) == str(i)
        bad[i] = 32767
        assert harness('symbols', 2, 2, 3, 16, _flat(bad)) == str(i)
    assert harness('symbols', 2, 2, 3, 16, _flat([15] * 12)) == '-1' and harness('symbols', 2, 2, 3, 16, _flat([15] * 11 + [16])) == '11'
    assert harness('symbols', 2, 2, 3, 1, _flat([0] * 12)) == '-1'
    # no entries: nothing to refuse; extents or an alphabet that describe no table
    assert harness('symbols', 0, 2, 3, 4, '-') == '-1' and harness('symbols', 2, 0, 3, 4, '-') == '-1'
    assert harness('symbols', 2, 2, 3, 4, '-') == '-2' and harness('symbols', -1, 2, 3, 4, '-') == '-2' and harness('symbols', 2, 2, 3, 0, _flat(sym)) == '-2'
    # a table that holds exactly the entries given: 3 x 5 x 457 symbols, the last one bad
    many = [i % 16 for i in range(3 * 5 * 457)]
    assert harness('symbols', 3, 5, 457, 16, _flat(many)) == '-1'
    assert harness('symbols', 3, 5, 457, 16, _flat(many[:-1] + [16])) == str(len(many) - 1)
