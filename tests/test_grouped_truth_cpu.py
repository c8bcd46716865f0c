"""CPU: the truth of the grouped top-K tests (tests/_grouped_truth.py) on hand-written rankings, the surface of the new entry
points (include/mi355_retrieval.h, _lib.py, knn.py, mining.py) as far as it answers without a device, and csrc/group_plan.h, the host
half of mi_gallery_set_groups, as a stand-alone program (tests/group_plan_check.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _grouped_truth as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"mi_gallery_set_groups": 4, "mi_gallery_get_groups": 2, "mi_gallery_group_count": 2, "mi_knn_search_grouped": 13}


def _walk(order, scores, labels, k, exclude=None, row_offset=0):
    ids, sc, lab = gt.grouped_truth(np.array([order], np.int64) + row_offset, np.array([scores], np.float32), labels, k,
                                    None if exclude is None else [exclude], row_offset)
    return ids[0].tolist(), sc[0].tolist(), lab[0].tolist()


def test_walk_ties_between_and_inside_groups():
    """Group A = rows {5, 10}, group B = {7}; rows 10 and 7 are identical and score highest, so the complete ranking is
    7, 10, 5, ...: B (row 7) precedes A (row 10), and A is reported by row 10, its best, not by row 5"""
    labels = np.full(12, -1)
    labels[[5, 10]] = 40
    labels[7] = 41
    order = [7, 10, 5, 0, 1, 2, 3, 4, 6, 8, 9, 11]
    scores = [9, 9, 8, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    ids, sc, lab = _walk(order, scores, labels, 4)
    assert ids == [7, 10, 0, 1] and sc == [9, 9, 1, 1] and lab == [41, 40, -1, -1]
    # a group of identical rows: the lowest id, which the ranking lists first
    labels[[0, 1, 2]] = 42
    assert _walk(order, scores, labels, 4)[0] == [7, 10, 0, 3]
    # a tie class that straddles rank k: rows 0 .. 4 tie at 1, k = 3 cuts through them in id order
    assert _walk(order, scores, np.full(12, -1), 5)[0] == [7, 10, 5, 0, 1]


def test_walk_exclusion_padding_and_singletons():
    labels = np.array([3, 3, -1, 8, 8, -1, 2 ** 31 - 1])
    order = [1, 0, 3, 2, 6, 4, 5]
    scores = [7, 6, 5, 4, 3, 2, 1]
    assert _walk(order, scores, labels, 3) == ([1, 3, 2], [7, 5, 4], [3, 8, -1])
    assert _walk(order, scores, labels, 3, exclude=3) == ([3, 2, 6], [5, 4, 3], [8, -1, 2 ** 31 - 1])
    assert _walk(order, scores, labels, 3, exclude=-1) == _walk(order, scores, labels, 3)       # -1 excludes nothing,
    assert _walk(order, scores, labels, 3, exclude=99) == _walk(order, scores, labels, 3)       # nor does a label no row has
    ids, sc, lab = _walk(order, scores, labels, 6, exclude=8)                                   # 4 eligible groups: padding
    assert ids == [1, 2, 6, 5, -1, -1] and lab == [3, -1, 2 ** 31 - 1, -1, -1, -1] and sc[4:] == [-np.inf, -np.inf]
    # every row a singleton: the ranking itself
    assert _walk(order, scores, np.full(7, -1), 7)[0] == order
    # one group: one row
    assert _walk(order, scores, np.zeros(7, int), 2) == ([1, -1], [7, -np.inf], [0, -1])
    # ids are global
    assert _walk(order, scores, labels, 3, row_offset=10 ** 6)[0] == [10 ** 6 + 1, 10 ** 6 + 3, 10 ** 6 + 2]


def test_reference_loop_matches_the_walk():
    rng = np.random.default_rng(5)
    P, Q, nnum = 60, 7, 6
    clusters = rng.integers(0, 12, P)
    qclusters = rng.integers(0, 12, Q)
    ranks = np.stack([rng.permutation(P) for _ in range(Q)], axis=1)
    want = gt.reference_negatives(ranks, clusters, qclusters, nnum)
    got = gt.grouped_truth(ranks.T, np.zeros((Q, P), np.float32), clusters, nnum, qclusters)[0]
    assert np.array_equal(got, want)
    short = gt.reference_negatives(ranks, np.zeros(P, int), np.ones(Q, int), 3)                  # one cluster in the pool
    assert (short[:, 0] == ranks[0]).all() and (short[:, 1:] == -1).all()


def test_surface_without_a_device():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib, knn, mining
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    for name, nargs in NEW.items():
        assert name + "(" in hdr and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "mi_group_info" in hdr and [f for f, _ in _lib.GroupInfo._fields_] == ["groups", "path", "kprime", "rerun_queries",
                                                                                 "excluded_found"]
    assert C.sizeof(_lib.GroupInfo) == 32
    # argument checks answer before a device is touched
    out = C.c_int64()
    assert lib.mi_gallery_set_groups(None, None, 0, 0) == _lib.MI_ERR_INVALID and b"null" in lib.mi_last_error()
    assert lib.mi_gallery_group_count(None, C.byref(out)) == _lib.MI_ERR_INVALID
    assert lib.mi_gallery_get_groups(None, None) == _lib.MI_ERR_INVALID
    assert lib.mi_knn_search_grouped(None, None, 0, 0, 0, 0, 1, None, None, None, None, None, None) == _lib.MI_ERR_INVALID
    val = C.c_double()
    assert lib.mi_get_global_option(b"group_overfetch", C.byref(val)) == 0 and val.value == 4
    assert lib.mi_get_global_option(b"group_dense_bytes", C.byref(val)) == 0 and val.value == 2 ** 30
    assert lib.mi_set_global_option(b"group_overfetch", C.c_double(4096.0)) == _lib.MI_ERR_INVALID
    with pytest.raises(ValueError):
        _lib.group_labels([0.5, 1.0])
    with pytest.raises(ValueError):
        _lib.group_labels([0, 2 ** 31])
    assert _lib.group_labels([3, -1, 2 ** 31 - 1]).dtype == np.int32
    for name in ("set_groups", "groups", "group_count", "search_grouped"):
        assert callable(getattr(_lib.Gallery, name))
    assert callable(knn.KNN.set_groups) and callable(knn.KNN.search_grouped) and callable(mining.hard_negatives_hip)
    with pytest.raises(ValueError):
        mining.hard_negatives_hip(np.zeros((4, 2), np.float32), np.zeros((5, 3), np.float32), [0, 0, 0], [0, 0], 1)


def test_group_plan_under_sanitizers(tmp_path):
    """tests/group_plan_check.cpp: relabelling, CSR and chunk partition of csrc/group_plan.h against their definitions, compiled
    with the host compiler under AddressSanitizer and UBSan and run as a program of its own; nothing is loaded into Python."""
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "group_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", os.path.join(here, "group_plan_check.cpp"), "-o", exe]
    sanitize = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    r = subprocess.run(base + sanitize + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base + sanitize, capture_output=True, text=True)
    if r.returncode != 0:                          # the sanitizer runtimes are a package of their own: the program's checks still run
        assert "sanitizer" in r.stderr or "asan" in r.stderr or "ubsan" in r.stderr, r.stderr[-3000:]
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout[-2000:], run.stderr[-4000:])
    assert run.returncode == 0 and "group_plan_check ok" in run.stdout
