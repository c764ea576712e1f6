"""MDE_pBX on the device, host half (no GPU): tblup_mde_windows / tblup_mde_resolve against numpy's
np.random.choice and python's random for the reference's loop (tblup/evolver.py:550-687), the
window-overflow status, and the argument checks of the new entries."""
import ctypes
import random

import numpy as np
import pytest

from tblup_amd import _native
from tblup_amd.evolver import exclusive_randrange

U32P = ctypes.POINTER(ctypes.c_uint32)
I32P = ctypes.POINTER(ctypes.c_int32)
I64P = ctypes.POINTER(ctypes.c_int64)


def _p(a, t):
    return a.ctypes.data_as(t)


def windows(pop, nq, npar, slack=-1):
    lib = _native.load()
    lo, hi = np.empty(pop, np.int32), np.empty(pop, np.int32)
    off = np.empty(pop + 1, np.int64)
    n = ctypes.c_int64()
    _native.check("tblup_mde_windows", lib.tblup_mde_windows(pop, nq, npar, slack, _p(lo, I32P), _p(hi, I32P),
                                                             _p(off, I64P), ctypes.byref(n)))
    assert n.value == off[pop]
    return lo, hi, off


def window_words(stream, L, lo, hi, off):
    """The compact buffer the device half fills: stream words [2Li + lo_i, 2Li + hi_i) per individual."""
    words = np.zeros(max(int(off[-1]), 1), np.uint32)
    for i in range(len(lo)):
        words[off[i]:off[i + 1]] = stream[2 * L * i + lo[i]:2 * L * i + hi[i]]
    return words


def resolve(pop, L, q_arr, p_arr, words, n_words, slack=-1):
    """tblup_mde_resolve on python's current `random` state; the state is set to the result's."""
    lib = _native.load()
    version, internal, gauss = random.getstate()
    mt = np.array(internal[:624], dtype=np.uint32)
    idx = np.array([internal[624]], dtype=np.int32)
    parent = np.empty(pop, np.int32)
    donors = np.empty((pop, 3), np.int32)
    fixed = np.empty(pop, np.int64)
    cw = np.empty(pop, np.int64)
    ovf = ctypes.c_int32(-1)
    q_arr = np.ascontiguousarray(q_arr, np.int32)
    p_arr = np.ascontiguousarray(p_arr, np.int32)
    _native.check("tblup_mde_resolve", lib.tblup_mde_resolve(
        pop, L, _p(q_arr, I32P), len(q_arr), _p(p_arr, I32P), len(p_arr), slack, _p(words, U32P), n_words,
        _p(mt, U32P), _p(idx, I32P), _p(parent, I32P), _p(donors, I32P), _p(fixed, I64P), _p(cw, I64P),
        ctypes.byref(ovf)))
    random.setstate((version, tuple(mt.tolist()) + (int(idx[0]),), gauss))
    return ovf.value, parent, donors, fixed, cw


def reference_loop(pop, L, q_arr, p_arr):
    """The reference's per-individual draws on numpy's and python's global states; C_i from numpy's
    position (every individual takes fewer than 624 words here)."""
    parent, donors, fixed, cw = [], [], [], []
    used = 0
    prev = np.random.get_state()[2] % 624
    for i in range(pop):
        best = int(np.random.choice(q_arr, 1).item())
        par = int(np.random.choice(p_arr, 1).item())
        a = exclusive_randrange(0, pop, [par, best])
        b = exclusive_randrange(0, pop, [par, best, a])
        fixed.append(random.randrange(0, L))
        np.random.rand(L)
        cur = np.random.get_state()[2] % 624
        used += (cur - prev) % 624
        prev = cur
        parent.append(par)
        donors.append((best, a, b))
        cw.append(used - 2 * L * (i + 1))
    return np.array(parent), np.array(donors), np.array(fixed), np.array(cw)


SIZES = [(1, 1), (1, 2), (2, 1), (2, 3), (3, 33), (33, 3), (38, 153), (153, 38), (1, 153), (33, 1)]


@pytest.mark.parametrize("pre", [0, 1, 623, 624])
@pytest.mark.parametrize("nq,npar", SIZES)
def test_resolve_equals_numpy_choice_and_python_random(nq, npar, pre):
    pop, L = 300, 7
    assert 2 * L + 64 < 624
    rng = np.random.default_rng(nq * 1000 + npar)
    q_arr = rng.permutation(pop)[:nq].astype(np.int32)
    p_arr = rng.permutation(pop)[:npar].astype(np.int32)
    random.seed(nq + 7 * npar + pre)
    np.random.seed(31 * nq + npar)
    np.random.bytes(4 * pre)
    py0, np0 = random.getstate(), np.random.get_state()
    stream = np.frombuffer(np.random.bytes(4 * (2 * L * pop + 16 * pop)), dtype="<u4")
    np.random.set_state(np0)
    want = reference_loop(pop, L, q_arr, p_arr)
    py_want = random.getstate()
    lo, hi, off = windows(pop, nq, npar)
    assert np.all(want[3] < hi) and np.all(np.concatenate([[0], want[3][:-1]]) >= lo)
    random.setstate(py0)
    ovf, parent, donors, fixed, cw = resolve(pop, L, q_arr, p_arr, window_words(stream, L, lo, hi, off), int(off[-1]))
    assert ovf == 0
    np.testing.assert_array_equal(cw, want[3])
    np.testing.assert_array_equal(parent, want[0])
    np.testing.assert_array_equal(donors, want[1])
    np.testing.assert_array_equal(fixed, want[2])
    assert random.getstate() == py_want
    if nq == 1 and npar == 1:
        assert not cw.any()


def test_windows_are_triangular_not_worst_case():
    lo, hi, off = windows(1024, 153, 512)
    assert lo[0] == 0 and np.all(np.diff(lo) == 2) and np.all(hi > lo)
    assert off[-1] == np.sum(hi - lo) and off[-1] * 4 < 8 << 20   # a few MB at pop 1024
    lo, hi, off = windows(1024, 1, 1)
    assert not lo.any() and off[-1] <= 16 * 1024


def test_resolve_forced_small_window_reports_overflow_and_keeps_states():
    pop, L, nq, npar = 200, 5, 3, 33
    q_arr, p_arr = np.arange(nq, dtype=np.int32), np.arange(npar, dtype=np.int32)
    random.seed(3)
    np.random.seed(4)
    py0, np0 = random.getstate(), np.random.get_state()
    stream = np.frombuffer(np.random.bytes(4 * (2 * L * pop + 16 * pop)), dtype="<u4")
    np.random.set_state(np0)
    lo, hi, off = windows(pop, nq, npar, slack=0)
    ovf = resolve(pop, L, q_arr, p_arr, window_words(stream, L, lo, hi, off), int(off[-1]), slack=0)[0]
    assert ovf == 1
    assert random.getstate() == py0
    st = np.random.get_state()
    assert np.array_equal(st[1], np0[1]) and st[2] == np0[2]
    # the same draws with the default slack resolve
    lo, hi, off = windows(pop, nq, npar)
    assert resolve(pop, L, q_arr, p_arr, window_words(stream, L, lo, hi, off), int(off[-1]))[0] == 0
    assert random.getstate() != py0


def test_mde_entries_reject_bad_arguments():
    lib = _native.load()
    n = ctypes.c_int64()
    assert lib.tblup_mde_windows(3, 1, 1, -1, None, None, None, ctypes.byref(n)) == -1
    assert b"pop" in lib.tblup_last_error()
    assert lib.tblup_mde_windows(8, 9, 1, -1, None, None, None, ctypes.byref(n)) == -1
    assert b"choice-array" in lib.tblup_last_error()
    assert lib.tblup_mde_windows(8, 2, 0, -1, None, None, None, ctypes.byref(n)) == -1
    assert lib.tblup_mde_windows(8, 2, 3, -1, None, None, None, None) == -1
    assert lib.tblup_mde_windows(8, 2, 3, -1, None, None, None, ctypes.byref(n)) == 0 and n.value > 0

    pop, L = 8, 5
    lo, hi, off = windows(pop, 2, 3)
    words = np.zeros(int(off[-1]), np.uint32)
    q_arr, p_arr = np.array([1, 2], np.int32), np.array([0, 3, 7], np.int32)
    internal = random.Random(1).getstate()[1]
    mt = np.array(internal[:624], dtype=np.uint32)
    idx = np.array([internal[624]], np.int32)
    parent, donors = np.empty(pop, np.int32), np.empty((pop, 3), np.int32)
    fixed, cw = np.empty(pop, np.int64), np.empty(pop, np.int64)
    ovf = ctypes.c_int32()

    def call(pop=pop, L=L, q=q_arr, p=p_arr, n_words=int(off[-1]), w=words, index=idx):
        return lib.tblup_mde_resolve(pop, L, _p(q, I32P), len(q), _p(p, I32P), len(p), -1,
                                     None if w is None else _p(w, U32P), n_words, _p(mt, U32P), _p(index, I32P),
                                     _p(parent, I32P), _p(donors, I32P), _p(fixed, I64P), _p(cw, I64P),
                                     ctypes.byref(ovf))
    assert call() == 0
    assert call(pop=3) == -1 and b"pop" in lib.tblup_last_error()
    assert call(L=0) == -1 and b"L" in lib.tblup_last_error()
    assert call(w=None) == -1 and b"null" in lib.tblup_last_error()
    assert call(n_words=int(off[-1]) + 1) == -1 and b"n_words" in lib.tblup_last_error()
    assert call(q=np.array([1, 8], np.int32)) == -1 and b"best index" in lib.tblup_last_error()
    assert call(p=np.array([0, -1, 7], np.int32)) == -1 and b"parent index" in lib.tblup_last_error()
    assert call(index=np.array([625], np.int32)) == -1 and b"py_index" in lib.tblup_last_error()
    # the device halves without a context
    assert lib.tblup_mde_draws(None, pop, L, 2, 3, -1, _p(mt, U32P), 0, _p(words, U32P), int(off[-1]), None) != 0
    f = np.zeros(pop)
    assert lib.tblup_mde_step_device_async(None, _p(f, ctypes.POINTER(ctypes.c_double)),
                                           _p(f, ctypes.POINTER(ctypes.c_double)), None, pop, L, L, _p(parent, I32P),
                                           _p(donors, I32P), _p(fixed, I64P), _p(cw, I64P), 1, 4.0, _p(mt, U32P), 0,
                                           None, L, None) != 0
