"""CPU: rmxh::lt_classes (remixt_amd/csrc/rmx_host.h), the total-copy classes of a state table that the cell cache keeps its
read-depth planes by, built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone harness
(tests/csrc/lt_classes_host.cpp) and checked on the state grids of the benchmark and the test shapes.  The expected class
counts are the numbers of distinct total-copy tuples of the reference's create_cn_states grids (cn_diff_max 1)."""
import os
import subprocess

import numpy as np
import pytest

from remixt_amd.cn_model import create_cn_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer', '-g', '-O1']


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ltc')
    exe = str(tmp / 'lt_classes_host')
    subprocess.check_call(['g++', '-std=c++17', '-ffp-contract=off', '-Wno-unknown-pragmas'] + SAN +
                          ['-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'lt_classes_host.cpp')])

    def run(tables):
        """tables: (C, S, M, 2) int64 -> (NT, [count], ltcls (C, S), ltrep (C, S))"""
        tables = np.ascontiguousarray(tables, dtype=np.int64)
        C, S, M, _ = tables.shape
        path = str(tmp / 'tables.bin')
        with open(path, 'wb') as f:
            f.write(np.array([C, S, M], dtype=np.int64).tobytes())
            f.write(tables.tobytes())
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120,
                             env=dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1'))
        assert out.returncode == 0 and 'Sanitizer' not in out.stderr and 'runtime error' not in out.stderr, out.stderr[-2000:]
        lines = out.stdout.splitlines()
        head = lines[0].split()
        assert head[0] == 'rc' and head[1] == '0'
        assert lines[-1] == 'args 5 5'
        counts, cls, rep = [], [], []
        for c in range(C):
            counts.append(int(lines[1 + 3 * c].split()[1]))
            cls.append([int(v) for v in lines[2 + 3 * c].split()[1:]])
            rep.append([int(v) for v in lines[3 + 3 * c].split()[1:]])
        return int(head[3]), counts, np.array(cls), np.array(rep)
    return run


def _keys(table):
    """(S, M + 1): total copy number per clone, then the hdel bit"""
    tot = table.sum(axis=2)
    hdel = (table == 0).all(axis=(1, 2)).astype(np.int64)
    return np.concatenate([tot, hdel[:, None]], axis=1)


def _check(tables, nt, counts, cls, rep):
    C, S = tables.shape[:2]
    assert nt == max(counts)
    for c in range(C):
        keys = _keys(tables[c])
        k = counts[c]
        assert cls[c].min() == 0 and cls[c].max() == k - 1
        assert (rep[c][:k] >= 0).all() and (rep[c][k:] == -1).all()
        # every state's class representative has the state's key
        assert np.array_equal(keys[rep[c][cls[c]]], keys)
        # distinct classes have distinct keys
        assert len(set(map(tuple, keys[rep[c][:k]]))) == k == len(set(map(tuple, keys)))
        # numbered by first appearance: the representative is the first state of its class, and a new class takes the next number
        seen = 0
        for s in range(S):
            if cls[c][s] == seen:
                assert rep[c][seen] == s
                seen += 1
            else:
                assert cls[c][s] < seen and rep[c][cls[c][s]] < s
        assert seen == k


@pytest.mark.parametrize('clones,max_cn,states,classes', [(3, 8, 165, 39), (3, 12, 355, 59), (4, 4, 207, 65), (3, 4, 47, 19)])
def test_class_counts_of_the_state_grids(harness, clones, max_cn, states, classes):
    table = create_cn_states(clones, 2, max_cn, 1)
    assert table.shape == (states, clones, 2)
    nt, counts, cls, rep = harness(table[None])
    assert nt == classes and counts == [classes]
    _check(table[None], nt, counts, cls, rep)


def test_two_tables_whose_normal_row_differs(harness):
    """A second state table as a sex chromosome of a male genome gets it: the normal clone has one copy.  The classes are
    found per table; the tumour clones' tuples are the same, so both tables have the same count and the same numbering."""
    auto = create_cn_states(3, 2, 8, 1)
    sex = auto.copy()
    sex[:, 0, :] = (1, 0)
    tables = np.stack([auto, sex])
    nt, counts, cls, rep = harness(tables)
    assert nt == 39 and counts == [39, 39]
    _check(tables, nt, counts, cls, rep)
    assert np.array_equal(cls[0], cls[1]) and np.array_equal(rep[0], rep[1])


def test_hdel_state_is_a_class_of_its_own_without_a_normal_clone(harness):
    """Without a normal clone the all-zero state is homozygously deleted: its key carries the hdel bit, and the tables of
    different sizes give different counts (NT is the largest)."""
    tum = create_cn_states(3, 2, 4, 1)[:, 1:, :]                        # (47, 2, 2): no normal row
    small = tum.copy()
    small[:, 1, :] = small[:, 0, :]                                       # both clones equal: fewer distinct total-copy tuples
    tables = np.stack([tum, small])
    nt, counts, cls, rep = harness(tables)
    _check(tables, nt, counts, cls, rep)
    assert counts[1] < counts[0] == nt
    hd = int(np.flatnonzero((tum == 0).all(axis=(1, 2)))[0])
    assert (cls[0] == cls[0][hd]).sum() == 1
