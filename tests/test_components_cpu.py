"""CPU: the host truth of the connected components on hand-written cases, and the error returns of mi_components_* that answer
before a device is touched."""
import ctypes as C

import numpy as np
import pytest

from _components_truth import components_truth, csr_pairs


def test_truth_chain():
    labels, groups = components_truth(6, [4, 0, 2, 1], [5, 1, 1, 2])
    assert labels.dtype == np.int32 and labels.tolist() == [0, 0, 0, 3, 4, 4] and groups == 3
    labels, groups = components_truth(5, [3, 2, 1, 0], [4, 3, 2, 1])            # a path given from its far end
    assert labels.tolist() == [0] * 5 and groups == 1


def test_truth_star_with_the_hub_at_the_largest_id():
    labels, groups = components_truth(7, [6] * 5, [1, 2, 3, 4, 5])
    assert labels.tolist() == [0, 1, 1, 1, 1, 1, 1] and groups == 2


def test_truth_two_triangles_joined_by_the_last_edge():
    i, j = [0, 1, 2, 3, 4, 5], [1, 2, 0, 4, 5, 3]
    labels, groups = components_truth(7, i, j)
    assert labels.tolist() == [0, 0, 0, 3, 3, 3, 6] and groups == 3
    labels, groups = components_truth(7, i + [5], j + [2])
    assert labels.tolist() == [0, 0, 0, 0, 0, 0, 6] and groups == 2


def test_truth_self_loops_and_repeated_edges():
    labels, groups = components_truth(4, [0, 1, 2, 3], [0, 1, 2, 3])
    assert labels.tolist() == [0, 1, 2, 3] and groups == 4
    labels, groups = components_truth(4, [3, 1, 3, 1, 3, 2], [1, 3, 1, 3, 1, 2])
    assert labels.tolist() == [0, 1, 2, 1] and groups == 3
    labels, groups = components_truth(3, [], [])
    assert labels.tolist() == [0, 1, 2] and groups == 3
    labels, groups = components_truth(0, [], [])
    assert labels.shape == (0,) and groups == 0


def test_truth_csr_pairs():
    i, j = csr_pairs(10, [0, 2, 2, 3], [11, 12, 12])
    assert i.tolist() == [10, 10, 12] and j.tolist() == [11, 12, 12]


@pytest.fixture(scope="module")
def built():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_null_handles_are_refused_with_a_message(built):
    lib, _lib = built
    buf = (C.c_int64 * 4)()
    calls = {
        "reset": lambda: lib.mi_components_reset(None),
        "add_pairs": lambda: lib.mi_components_add_pairs(None, buf, buf, 1, _lib.MI_HOST),
        "add_csr": lambda: lib.mi_components_add_csr(None, 0, buf, buf, 1, _lib.MI_HOST),
        "add_hamming_self": lambda: lib.mi_components_add_hamming_self(None, None, 0, 0, 0),
        "labels": lambda: lib.mi_components_labels(None, buf, _lib.MI_HOST, None),
        "info": lambda: lib.mi_components_info(None, None, None),
    }
    for name, call in calls.items():
        lib.mi_set_global_option(b"no_such_option", 1.0)                 # another message in between
        assert call() == _lib.MI_ERR_INVALID, name
        assert b"null" in lib.mi_last_error(), name
    with pytest.raises(RuntimeError):
        _lib.check(lib.mi_components_labels(None, buf, _lib.MI_HOST, None))


def test_create_checks_n_before_any_device_call(built):
    lib, _lib = built
    h = C.c_void_p()
    # the device number is one no machine has: a call that reached the device layer would fail with another code
    for n in (-1, -2 ** 40, 2 ** 31, 2 ** 40):
        assert lib.mi_components_create(n, 12345, C.byref(h)) == _lib.MI_ERR_INVALID
        assert b"n must be in" in lib.mi_last_error() and not h.value
    assert lib.mi_components_create(10, 0, None) == _lib.MI_ERR_INVALID and b"null" in lib.mi_last_error()
    with pytest.raises(RuntimeError):
        _lib.Components(-1)


def test_destroy_null_is_ok(built):
    lib, _ = built
    assert lib.mi_components_destroy(None) == 0


def test_python_ids_are_checked_without_a_device(built):
    _, _lib = built
    assert _lib.component_ids([3, 1, 2]).dtype == np.int64
    a = np.arange(10, dtype=np.int32)[::3]
    got = _lib.component_ids(a)
    assert got.flags.c_contiguous and got.tolist() == [0, 3, 6, 9]
    assert _lib.component_ids([]).shape == (0,)
    for bad in (np.zeros((2, 2), np.int64), np.array([0.5, 1.0]), np.array([2 ** 63], dtype=np.uint64)):
        with pytest.raises(ValueError):
            _lib.component_ids(bad)
