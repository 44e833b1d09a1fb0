"""GPU parity of the shadow search's streaming pipeline (k_pass_mf): a wave keeps
TCI_MF_INFLIGHT chunk buffers in flight, the first of them pre-assigned (h_i = rep + i kMfReps), the
rest handed out by the slice's counter. The shapes reach the pipeline's edges at small sizes: fewer
chunks than buffers, a chunk count that is no multiple of the depth, buffers in flight across a staged
group's boundary, partial row slices, rows past the shadow's leading dimension, the refresh / EXT
instances, the two-K-step instances that stay at depth 2, and examination lists that fill mid-stream.
The small and mid paths are off and the shadow is on; row and column permutations, L, U, npivot and
error must equal the oracle's bit for bit, left- and right-orthogonal.

The depth is whatever the library was built with: 2 on the default build, where the loop matches the
one before the knob. The depths above 2 (the late prefetch of buffers 2.., their pre-assigned turns
after the seed, the counter's start at D kMfReps) run only when this file is run against a variant
library (make variant ... VFLAGS=-DTCI_MF_INFLIGHT=D, TCI_HIP_LIB=...).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensorcrossinterpolation.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

ORIENTATIONS = [True, False]  # leftorthogonal


def rand(m, n, seed):
    return O.fill_uniform(m * n, seed=seed).reshape((m, n), order="F")


def tie_pattern(m, n):
    i = np.arange(1, m + 1)[:, None]
    j = np.arange(1, n + 1)[None, :]
    return ((i * j) % 7 - 3).astype(np.float64)


_inputs = {}
_refs = {}


def matrix(kind, m, n):
    key = (kind, m, n)
    if key not in _inputs:
        A = tie_pattern(m, n) if kind == "ties" else rand(m, n, 7 * m + n)
        A.setflags(write=False)
        _inputs[key] = A
    return _inputs[key]


def reference(kind, m, n, **kw):
    """The oracle's factorisation, computed once per input and arguments."""
    key = (kind, m, n, tuple(sorted(kw.items())))
    if key not in _refs:
        _refs[key] = O.OracleLU(matrix(kind, m, n), **kw)
    return _refs[key]


def assert_same(got, ref):
    assert got.npivot == ref.npivot
    assert np.array_equal(got.rowpermutation - 1, ref.rowpermutation)
    assert np.array_equal(got.colpermutation - 1, ref.colpermutation)
    assert np.array_equal(got.L, ref.L)
    assert np.array_equal(got.U, ref.U)
    assert got.error == ref.error


def pass_context(T):
    """The pass pipeline for every size, shadow search on (reads TCI_PASS_GRIDDIV when created)."""
    c = T.Context(0)
    c.check(c.lib.tci_set_rrlu_small(c.h, 0))
    c.check(c.lib.tci_set_rrlu_mid(c.h, 0))
    c.check(c.lib.tci_set_rrlu_shadow(c.h, 1))
    return c


def run_case(T, kind, m, n, **kw):
    c = pass_context(T)
    try:
        return T.rrlu(matrix(kind, m, n), ctx=c, **kw)
    finally:
        c.close()


@pytest.fixture
def T():
    return pytest.importorskip("tci_amd")


@pytest.mark.gpu
@pytest.mark.parametrize("leftorth", ORIENTATIONS)
def test_one_chunk_per_group(T, monkeypatch, leftorth):
    """600 x 1000 on the default grid: one 8-column tile per workgroup, i.e. one chunk per group --
    fewer chunks than buffers, and most waves idle."""
    monkeypatch.delenv("TCI_PASS_GRIDDIV", raising=False)
    kw = dict(maxrank=60, leftorthogonal=leftorth)
    assert_same(run_case(T, "rand", 600, 1000, **kw), reference("rand", 600, 1000, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("leftorth", ORIENTATIONS)
def test_chunk_count_no_multiple_of_depth(T, monkeypatch, leftorth):
    """1100 x 900 on a sixteenth of the grid: about 23 tiles per workgroup, 184 staged columns, 12
    chunks with the last half empty."""
    monkeypatch.setenv("TCI_PASS_GRIDDIV", "16")
    kw = dict(maxrank=120, leftorthogonal=leftorth)
    assert_same(run_case(T, "rand", 1100, 900, **kw), reference("rand", 1100, 900, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("leftorth", ORIENTATIONS)
def test_buffers_cross_group_boundary(T, monkeypatch, leftorth):
    """300 x 8300 on a sixteenth of the grid: 65 column tiles per workgroup against 64 per staged
    group, so a second group of one tile follows a full one."""
    monkeypatch.setenv("TCI_PASS_GRIDDIV", "16")
    kw = dict(maxrank=40, leftorthogonal=leftorth)
    assert_same(run_case(T, "rand", 300, 8300, **kw), reference("rand", 300, 8300, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n", [(70, 40), (1030, 530)])
@pytest.mark.parametrize("leftorth", ORIENTATIONS)
def test_partial_row_slices(T, monkeypatch, m, n, leftorth):
    """Partial row slices, and rows past the shadow's leading dimension."""
    monkeypatch.setenv("TCI_PASS_GRIDDIV", "16")
    kw = dict(maxrank=30, leftorthogonal=leftorth)
    assert_same(run_case(T, "rand", m, n, **kw), reference("rand", m, n, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("nb,epochs", [(10, 2), (10, 3), (15, 2)])
@pytest.mark.parametrize("leftorth", ORIENTATIONS)
def test_schedules(T, monkeypatch, nb, epochs, leftorth):
    """Refresh and EXT instances, and (nb = 15) the two-K-step instances that stay at depth 2."""
    monkeypatch.delenv("TCI_PASS_GRIDDIV", raising=False)
    kw = dict(maxrank=120, leftorthogonal=leftorth)
    c = pass_context(T)
    try:
        c.check(c.lib.tci_set_rrlu_flush(c.h, nb))
        c.check(c.lib.tci_set_rrlu_epochs(c.h, epochs))
        got = T.rrlu(matrix("rand", 1100, 900), ctx=c, **kw)
    finally:
        c.close()
    assert_same(got, reference("rand", 1100, 900, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("leftorth", ORIENTATIONS)
def test_integer_tie_pattern(T, monkeypatch, leftorth):
    """((i j) mod 7) - 3: the maximum is attained all over the matrix, so nearly every 4-row block of a
    chunk (up to 256 per chunk) goes to the wave's examination list (128 entries). On a sixteenth of
    the grid a workgroup has 16 tiles = 128 columns = 8 chunks per slice, about 4 per wave, so the
    list overflows mid-stream (flush(false_type)) while more chunks are in flight. (On the default grid
    a workgroup has one 8-column tile: at most 128 entries, which never overflow.)"""
    monkeypatch.setenv("TCI_PASS_GRIDDIV", "16")
    kw = dict(maxrank=60, leftorthogonal=leftorth)
    assert_same(run_case(T, "ties", 600, 1000, **kw), reference("ties", 600, 1000, **kw))
    # reltol = 0, as in test_shadow_integer_pattern_ties: past the pattern's rank the pivots are 0 and
    # the reference raises; the device must raise the same
    kw = dict(maxrank=60, reltol=0.0, leftorthogonal=leftorth)
    with pytest.raises(O.OracleError) as ref:
        reference("ties", 600, 1000, **kw)
    with pytest.raises(T.TCIError) as got:
        run_case(T, "ties", 600, 1000, **kw)
    assert str(ref.value) in str(got.value) or str(got.value) in str(ref.value)


@pytest.mark.skipif(not (os.path.exists(HIPCC) and shutil.which("make")), reason="needs hipcc and make")
def test_make_lists_rrlu_source():
    """The library's makefile compiles tci_rrlu.hip (a dry run: nothing is built)."""
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC], capture_output=True, text=True, check=True).stdout
    assert "tci_rrlu.hip" in out
