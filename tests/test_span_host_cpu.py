"""CPU: the host-only pieces of rmx_region_span (rmxh::span_window_ok, rmxh::span_spread_nan in remixt_amd/csrc/rmx_host.h), built
with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program (tests/csrc/span_host.cpp): the window rule at
and around the cap and at the ends of int32, and NaN spread over the queries of the flagged restarts only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('span') / 'span_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'span_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-2000:]
        return out.stdout.splitlines()
    return run


def test_window_rule(harness):
    ok = [(0, 0), (127, 127), (0, 16383), (16383, 0), (7, 2047), (1, 8191)]
    bad = [(-1, 0), (0, -1), (127, 128), (128, 127), (0, 16384), (1, 8192), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0), (-2 ** 31, -2 ** 31)]
    for wl, wr in ok:
        assert harness('window', wl, wr) == ['ok 1'], (wl, wr)
    for wl, wr in bad:
        assert harness('window', wl, wr) == ['ok 0'], (wl, wr)


@pytest.mark.parametrize('seed,nr,nq,per', [(1, 1, 1, 1), (2, 5, 7, 19), (3, 4, 3, 114), (4, 2, 9, 16384)])
def test_spread_nan(harness, seed, nr, nq, per):
    lines = harness('spread', seed, nr, nq, per)
    counts = dict(((int(a), int(b)), int(c)) for a, b, c in (ln.split() for ln in lines[1:-1]))
    assert len(counts) == nr * nq and lines[-1] == 'null 0'
    filled = 0
    for (ri, i), n in counts.items():
        if ri % 2 == 0:       # a flagged restart: a query is whole or NaN in every entry
            assert n in (0, per), (ri, i, n)
            filled += n == per
        else:                 # not flagged: what was sown stays one entry
            assert n in (0, 1), (ri, i, n)
    assert lines[0] == 'filled %d' % filled
