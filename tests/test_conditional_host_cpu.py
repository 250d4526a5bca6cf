"""CPU: the host-only pieces of rmx_region_conditional (rmxh::check_conditional, conditional_q_ok and conditional_pairs in
remixt_amd/csrc/rmx_host.h), built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program
(tests/csrc/conditional_host.cpp): every refusal of the entry point's runs and windows, the valid edge cases, and the
chunk caps."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']
# 12 segments, chains [0, 5] and [6, 11]; 2 masks, 3 labels; 8 slots
MODEL = (12, 2, 3, 8, '5,11')


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('conditional') / 'conditional_host')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas'] + SAN + ['-o', path, os.path.join(ROOT, 'tests', 'csrc', 'conditional_host.cpp')])
    return path


def _run(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
    assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-2000:]
    return out.stdout.strip()


@pytest.fixture(scope='module')
def harness(exe):
    def run(queries, windows, model=MODEL):
        flat = lambda rows: ','.join(str(int(x)) for row in rows for x in row) or '-'
        return _run(exe, list(model) + [flat(queries), flat(windows)])
    return run


def test_valid(harness):
    assert harness([(2, 3, 0, 1)], [(0, 5)]) == 'ok'
    # lo = a = b = hi
    assert harness([(4, 4, -1, -1)], [(4, 4)]) == 'ok'
    # a whole chain as run and window, of either chain; a window exactly nslot long would be (0, 7), which crosses chains
    assert harness([(0, 5, 1, 2), (6, 11, 1, 2)], [(0, 5), (6, 11)]) == 'ok'
    # windows at both ends of the model
    assert harness([(0, 0, 0, 0), (11, 11, 1, 2)], [(0, 3), (8, 11)]) == 'ok'
    # a window as long as nslot, in a model of one chain
    assert harness([(3, 4, -1, -1)], [(2, 9)], model=(12, 2, 3, 8, '11')) == 'ok'
    # no queries: nothing to refuse (the entry point refuses nq < 1 itself); a model of one segment
    assert harness([], []) == 'ok'
    assert harness([(0, 0, -1, -1)], [(0, 0)], model=(1, 0, 0, 1, '-')) == 'ok'
    # the longest run and window the rules take
    assert harness([(0, 4095, -1, -1)], [(0, 16383)], model=(16384, 0, 0, 16384, '16383')) == 'ok'


@pytest.mark.parametrize('queries,windows,model,bad,reason', [
    ([(2, 3, 0, 1)], [(0, 5)], (12, 2, 3, 0, '5,11'), 0, 'nslot must be in [1, 16384]'),
    ([(2, 3, 0, 1)], [(0, 5)], (12, 2, 3, 16385, '5,11'), 0, 'nslot must be in [1, 16384]'),
    ([(3, 2, 0, 1)], [(0, 5)], MODEL, 0, '0 <= first <= last < num_segments'),
    ([(-1, 2, 0, 1)], [(0, 5)], MODEL, 0, '0 <= first <= last < num_segments'),
    ([(2, 3, 0, 1), (10, 12, 0, 1)], [(0, 5), (6, 11)], MODEL, 1, '0 <= first <= last < num_segments'),
    ([(2 ** 31 - 1, 2 ** 31 - 1, 0, 1)], [(0, 5)], MODEL, 0, '0 <= first <= last < num_segments'),
    ([(2, 3, 0, 1)], [(3, 5)], MODEL, 0, 'lo <= first and last <= hi'),
    ([(2, 3, 0, 1)], [(0, 2)], MODEL, 0, 'lo <= first and last <= hi'),
    ([(2, 3, 0, 1)], [(-1, 5)], MODEL, 0, 'lo <= first and last <= hi'),
    ([(8, 9, 0, 1)], [(6, 12)], MODEL, 0, 'lo <= first and last <= hi'),
    ([(8, 9, 0, 1)], [(6, 2 ** 31 - 1)], MODEL, 0, 'lo <= first and last <= hi'),
    ([(2, 3, 0, 1), (4, 5, 0, 1)], [(0, 5), (4, 6)], MODEL, 1, 'crosses a chain end'),
    ([(4, 7, 0, 1)], [(4, 7)], MODEL, 0, 'crosses a chain end'),
    ([(3, 4, -1, -1)], [(1, 9)], (12, 2, 3, 8, '11'), 0, 'longer than nslot'),
    ([(0, 4096, -1, -1)], [(0, 4096)], (16384, 0, 0, 16384, '16383'), 0, 'longer than 4096'),
    ([(2, 3, 2, 1)], [(0, 5)], MODEL, 0, 'mask index out of range'),
    ([(2, 3, -2, 1)], [(0, 5)], MODEL, 0, 'mask index out of range'),
    ([(2, 3, 1, 3)], [(0, 5)], MODEL, 0, 'label index out of range'),
    ([(2, 3, 1, 2), (2, 3, 1, -2)], [(0, 5), (0, 5)], MODEL, 1, 'label index out of range'),
])
def test_refusals(harness, queries, windows, model, bad, reason):
    out = harness(queries, windows, model)
    assert out.startswith('bad %d ' % bad) and reason in out, out


def test_q_rule_and_chunk_caps(exe):
    assert [_run(exe, ['q', Q]) for Q in (-1, 0, 1, 64, 65)] == ['0', '0', '1', '1', '0']
    MiB = 1 << 20
    # the largest output (16384 slots of 67 doubles and log P) and the largest strip (4096 x 1024 doubles) each leave room for a pair
    per, strip = 16384 * 67 + 1, 4096 * 1024
    assert int(_run(exe, ['pairs', per, strip])) == min(64 * MiB // (per * 8 + 16), 256 * MiB // (strip * 8)) == 7
    assert int(_run(exe, ['pairs', per, 1])) == 64 * MiB // (per * 8 + 16) == 7
    assert int(_run(exe, ['pairs', 12, strip])) == 8
    # a small query: the outputs' cap binds, or the workspace's
    assert int(_run(exe, ['pairs', 60 * 15 + 1, 3 * 165])) == min(64 * MiB // ((60 * 15 + 1) * 8 + 16), 256 * MiB // (3 * 165 * 8))
    assert int(_run(exe, ['pairs', 12, 64 * 355])) == 256 * MiB // (64 * 355 * 8)
    # never less than one pair, and no division by a strip of 0
    assert int(_run(exe, ['pairs', 1 << 40, 1 << 40])) == 1 and int(_run(exe, ['pairs', 1, 0])) == 64 * MiB // 24
