"""CPU: the shortlist re-ranking (mi_refine, mi_refine_device) is declared, exported and bound, answers bad
arguments before touching a device, and its numpy truth (tests/_refine_truth.py) does what it says on hand-made cases.  The shape
sweep of the GPU test is checked here for coverage and for the gap between distinct candidates that pins its ids."""
import ctypes as C
import os

import numpy as np
import pytest

import _refine_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi_refine", "mi_refine_device"]


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_declared_exported_and_bound(built_lib):
    lib, _lib = built_lib
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    for name in NEW:
        assert "int %s(" % name in hdr, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype == C.c_int
    assert len(_lib.SIGNATURES["mi_refine_device"][1]) == 11
    assert len(_lib.SIGNATURES["mi_refine"][1]) == 14
    for meth in ("refine", "refine_device"):
        assert hasattr(_lib.Gallery, meth)
    import inspect
    for cls in (_lib.PQIndex, _lib.IVFPQIndex, _lib.BinaryGallery, _lib.LSHIndex):
        p = inspect.signature(cls.search).parameters
        assert p["refine"].default is None and p["k_factor"].default == 1, cls
    from isehr_amd import knn, nnsearch
    assert inspect.signature(knn.ANN.__init__).parameters["refine_k_factor"].default == 0
    for fn in (nnsearch.matching_PQ_Net_bucket_hip, nnsearch.matching_LSH_hip):
        p = inspect.signature(fn).parameters
        assert p["refine_rows"].default is None and p["k_factor"].default == 10


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 4), np.float32)
    cand = np.zeros((2, 8), np.int64)
    idx = np.zeros(16, np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def dev(g=fake, qp=P(q), nq=2, cp=P(cand), kc=8, stride=8, k=4, op=P(idx)):
        return lib.mi_refine_device(g, qp, nq, cp, kc, stride, k, op, None, None, None)

    def host(g=fake, qp=P(q), nq=2, dtype=0, cp=P(cand), kc=8, stride=8, k=4, op=P(idx)):
        return lib.mi_refine(g, qp, nq, dtype, 4, 1, cp, kc, stride, k, op, None, None, None)

    for call in (dev, host):
        for kwargs, word in [(dict(g=None), b"null handle"), (dict(kc=0), b"kc must"), (dict(kc=8193, stride=8193), b"kc must"),
                             (dict(k=0), b"k must"), (dict(k=9), b"k must"), (dict(nq=-1), b"nq"), (dict(stride=7), b"cand_stride"),
                             (dict(qp=None), b"queries"), (dict(cp=None), b"candidates"), (dict(op=None), b"out_idx")]:
            assert call(**kwargs) == _lib.MI_ERR_INVALID, (call.__name__, kwargs)
            assert word in lib.mi_last_error(), (call.__name__, kwargs, lib.mi_last_error())
        assert call(nq=0, qp=None, cp=None, op=None) == 0         # nq == 0: MI_OK, nothing read, nothing written
    assert host(dtype=9) == _lib.MI_ERR_INVALID and b"dtype" in lib.mi_last_error()
    assert (idx == 0).all()
    with pytest.raises(ValueError):
        _lib.refine_kc(10, 0, 100)
    assert _lib.refine_kc(10, 10, 5000) == 100 and _lib.refine_kc(10, 10, 50) == 50 and _lib.refine_kc(2048, 10, 10 ** 6) == 8192
    assert _lib.refine_kc(10, 1, 3) == 10                         # never below k: the index pads, the refine pads again


def test_truth_on_hand_made_cases():
    rows = np.array([[0, 0], [3, 4], [1, 0], [0, 1], [6, 8]], np.float32)
    q = np.array([[0, 0]], np.float32)
    # repeats, padding below and beyond the shard, a tie (rows 2 and 3 at distance 1) broken by the lower id
    cand = np.array([[4, 3, 3, 2, -1, 5, 1, 1, 2, 99]], np.int64)
    ids, val = T.refine_truth(rows, q, cand, 6, True)
    assert ids.tolist() == [[2, 3, 1, 4, -1, -1]]
    assert val.tolist() == [[1.0, 1.0, 25.0, 100.0, np.inf, np.inf]]
    q2 = np.array([[1, 1]], np.float32)
    ids, val = T.refine_truth(rows, q2, cand, 3, False)
    assert ids.tolist() == [[4, 1, 2]] and val.tolist() == [[14.0, 7.0, 1.0]]
    # a row offset: the same rows are ids 10 .. 14, and what was in range is padding now
    ids, val = T.refine_truth(rows, q, cand + 10, 2, True, row_offset=10)
    assert ids.tolist() == [[12, 13]]
    ids, val = T.refine_truth(rows, q, cand, 2, True, row_offset=10)
    assert ids.tolist() == [[-1, -1]] and np.isinf(val).all()
    # all padding; k larger than the number of distinct candidates
    ids, val = T.refine_truth(rows, q2, np.full((1, 4), -1), 4, False)
    assert ids.tolist() == [[-1] * 4] and (val == -np.inf).all()
    ids, val = T.refine_truth(rows, q, np.array([[0, 0, 0, 0]]), 4, True)
    assert ids.tolist() == [[0, -1, -1, -1]] and val[0, 0] == 0.0 and np.isinf(val[0, 1:]).all()
    b = T.value_bound(rows, q2, np.array([[4, -1]]), 2)
    assert b[0, 0] == 6 * 2.0 ** -53 * (2.0 + 100.0) and b[0, 1] == 0.0


def test_sweep_covers_every_axis():
    cases = T.sweep_cases()
    assert len(cases) == 44
    for axis, want in enumerate([T.KCS, T.DS, T.NS, T.NQS, T.KMODES, [True, False], [0, 1000003]]):
        assert {c[axis] for c in cases} == set(want), axis
    for l2 in (True, False):                      # both LDS tiers (kc <= 2048 < kc) under both metrics
        assert {c[0] > 2048 for c in cases if c[5] == l2} == {True, False}


def test_sweep_inputs_are_tie_free():
    """What lets the GPU test demand EQUAL ids: for these seeds no two distinct candidates of a query lie within twice the
    rounding bound (d + 4) 2^-53 (||q||^2 + ||g||^2) of each other in float64."""
    for case in T.sweep_cases():
        rows, q, cand = T.case_inputs(case)
        assert T.min_gap_over_bound(rows, q, cand, case[5], case[6]) > 2.0, case
