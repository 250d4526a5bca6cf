"""CPU: the host-only pieces of rmx_path_entropy (rmxh::entropy_range_ok, rmxh::entropy_tiles and rmxh::entropy_chunk in
remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/csrc/entropy_host.cpp) that runs as a child process: the range rule at its edges, the work lists over tables that hold
exactly the entries of the range -- a read past a table or a write past a counted list is a heap overflow -- and the chunk rule."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1
LMAX = 2 ** 63 - 1


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('entropy') / 'entropy_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'entropy_host.cpp')])

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, (out.returncode, out.stdout, out.stderr[-2000:])
        return out.stdout.strip()
    return run


def _flat(values):
    return ','.join(str(int(v)) for v in values) or '-'


def _tiles(harness, n0, n1, TC, tclass, brk):
    """(tiles as (class, [indices]), singles) of the program's answer."""
    lines = harness('tiles', n0, n1, TC, _flat(tclass[:n1]), _flat(brk[:n1])).split('\n')
    nt, ns = (int(v) for v in lines[0].split())
    assert len(lines) == 1 + nt + 1
    tiles = []
    for line in lines[1:1 + nt]:
        c, idx = line.split(':')
        tiles.append((int(c), [int(v) for v in idx.split(',')]))
    singles = [] if lines[-1] == '-' else [int(v) for v in lines[-1].split(',')]
    assert len(singles) == ns
    return tiles, singles


def _expected(n0, n1, TC, tclass, brk):
    tiles = []
    for c in range(TC):
        idx = [n for n in range(n0, n1) if tclass[n] == c and brk[n] < 0]
        for k in range(0, len(idx), 16):
            part = idx[k:k + 16]
            tiles.append((c, part + [-1] * (16 - len(part))))
    return tiles, [n for n in range(n0, n1) if tclass[n] >= 0 and brk[n] >= 0]


@pytest.mark.parametrize('N,n0,n1,want', [(1, 0, 1, 'ok'), (1, 0, 0, 'bad'), (1, 1, 1, 'bad'), (1, 0, 2, 'bad'), (1, -1, 1, 'bad'), (0, 0, 0, 'bad'),
                                          (10, 9, 10, 'ok'), (10, 0, 10, 'ok'), (10, 10, 11, 'bad'), (10, 5, 4, 'bad'), (IMAX, 0, IMAX, 'ok'),
                                          (IMAX, IMIN, IMAX, 'bad'), (LMAX, LMAX - 1, LMAX, 'ok'), (-1, 0, 1, 'bad')])
def test_range(harness, N, n0, n1, want):
    assert harness('range', N, n0, n1) == want


def test_tiles_at_their_edges(harness):
    # N = 1: the only segment ends its chain: nothing in either list
    assert _tiles(harness, 0, 1, 1, [-1], [-1]) == ([], [])
    # a class with exactly 16 and one with 17 adjacencies (class 1 first in the range; classes come out ascending), a breakend in between
    tclass = [1] * 17 + [0] * 8 + [0] + [0] * 8 + [-1]
    brk = [-1] * 25 + [0] + [-1] * 9
    for n0, n1 in ((0, 35), (0, 34), (1, 35), (0, 17), (16, 18), (25, 26), (34, 35), (3, 4)):
        assert _tiles(harness, n0, n1, 2, tclass, brk) == _expected(n0, n1, 2, tclass, brk), (n0, n1)
    tiles, singles = _tiles(harness, 0, 35, 2, tclass, brk)
    assert [t[0] for t in tiles] == [0, 1, 1] and tiles[0][1].count(-1) == 0 and tiles[2][1] == [16] + [-1] * 15 and singles == [25]
    # a range of one segment: a plain adjacency, a breakend, a chain end
    assert _tiles(harness, 3, 4, 2, tclass, brk) == ([(1, [3] + [-1] * 15)], [])
    assert _tiles(harness, 25, 26, 2, tclass, brk) == ([], [25])
    assert _tiles(harness, 34, 35, 2, tclass, brk) == ([], [])
    # a range with no plain adjacency; a range that is all chain ends
    assert _tiles(harness, 0, 4, 3, [2, 2, -1, 0], [0, 1, -1, 2]) == ([], [0, 1, 3])
    assert _tiles(harness, 0, 5, 3, [-1] * 5, [-1] * 5) == ([], [])
    assert _tiles(harness, 0, 5, 0, [-1] * 5, [-1] * 5) == ([], [])
    # an empty range reads nothing
    assert harness('tiles', 4, 4, 2, _flat([0] * 4), _flat([-1] * 4)).split('\n')[0] == '0 0'
    # many classes, some without a member; 457 segments with a class change every 7
    tc = [(n // 7) % 5 if n % 50 != 49 else -1 for n in range(457)]
    bk = [n if n % 11 == 3 else -1 for n in range(457)]
    assert _tiles(harness, 0, 457, 9, tc, bk) == _expected(0, 457, 9, tc, bk)
    assert _tiles(harness, 100, 333, 9, tc, bk) == _expected(100, 333, 9, tc, bk)


def test_tiles_refuse_what_describes_no_range(harness):
    first = lambda *a: harness('tiles', *a).split('\n')[0]
    assert first(-1, 3, 1, '0,0,0', '-1,-1,-1') == '-1 -1' and first(3, 2, 1, '0,0', '-1,-1') == '-1 -1'
    assert first(0, 2, 1, '-', '-1,-1') == '-1 -1' and first(0, 2, 1, '0,0', '-') == '-1 -1' and first(0, 2, -1, '0,0', '-1,-1') == '-1 -1'
    # a class at or beyond TC
    assert first(0, 3, 2, '0,2,1', '-1,-1,-1') == '-1 -1' and first(0, 3, 2, '0,%d,1' % IMAX, '-1,-1,-1') == '-1 -1'
    assert first(0, 3, 0, '-1,0,-1', '-1,-1,-1') == '-1 -1'


@pytest.mark.parametrize('nr,nseg,budget,want', [
    (16, 4000, 64 << 20, 4000),            # the bench: one chunk
    (16, 4000, 16 * 16 * 100, 100),        # a budget of exactly 100 segments
    (16, 4000, 16 * 16 * 100 - 1, 99),
    (16, 4000, 16 * 16, 1), (16, 4000, 16 * 16 - 1, 1), (16, 4000, 1, 1), (16, 4000, 0, 1), (16, 4000, -5, 1),      # below one segment: still 1
    (1, 1, 64 << 20, 1), (65535, IMAX, 64 << 20, 64), (IMAX, IMAX, 64 << 20, 1), (LMAX, LMAX, LMAX, 1), (1, LMAX, LMAX, LMAX // 16),
    (0, 5, 100, 1), (5, 0, 100, 1), (-1, -1, -1, 1)])
def test_chunk(harness, nr, nseg, budget, want):
    assert harness('chunk', nr, nseg, budget) == str(want)
