"""CPU: the truth module of the Minkowski search against a naive float64 evaluation, the argument checks of the binding that need
no device, and the matcher table.  tests/test_gpu_minkowski.py holds the device to tests/_minkowski_truth.py."""
import inspect
import math
from fractions import Fraction

import numpy as np
import pytest

import _minkowski_truth as T


def _data(seed, n, d, nq):
    """Gaussian values over 48 binades: sums of float32 values of one magnitude are exact in float64, and then no order shows"""
    rng = np.random.default_rng([seed, n, d])
    wide = lambda m: (rng.standard_normal((m, d)) * 2.0 ** rng.integers(-24, 24, (m, d))).astype(np.float32)
    return wide(n), wide(nq)


def test_fma_is_one_rounding():
    """T.fma against exact rational arithmetic: squares of float64 differences of float32 values onto running sums (what the
    p == 2 chain feeds it), and products built to land on rounding ties."""
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(4000).astype(np.float32).astype(np.float64) - rng.standard_normal(4000).astype(np.float32).astype(np.float64))
    c = np.abs(rng.standard_normal(4000)) * rng.choice([1e-6, 1.0, 1e3, 1e9], 4000)
    x = np.concatenate([a, [1.0 + 2.0 ** -26, 1.0 + 2.0 ** -26, 3.0, 1.0 + 2.0 ** -30]])
    z = np.concatenate([c, [1.0, 2.0 ** 53, 2.0 ** 54, 2.0 ** -60]])
    got = T.fma(x, x, z)
    for xi, zi, gi in zip(x.tolist(), z.tolist(), got.tolist()):
        assert gi == float(Fraction(xi) * Fraction(xi) + Fraction(zi))


@pytest.mark.parametrize("d", [1, 3, 4, 255, 256, 257, 259, 700])
def test_truth_agrees_with_naive_float64(d):
    """Linf exactly (a max does not round); sums within (d + 2) 2^-52 relative: every term is non-negative, each of the at most
    d - 1 additions of either order rounds once (2^-53 relative to a partial sum that never exceeds the total), the terms
    themselves round once on both sides (sqrt, pow: numpy's against numpy's, the same bits; the squares of p == 2 round inside
    the fused add here and before the add there), so the two sums differ by less than 2 (d + 1) 2^-53 of the total."""
    rows, q = _data(1, 37, d, 5)
    assert np.array_equal(T.values(rows, q, "linf"), T.naive_values(rows, q, "linf"))
    for metric, p in (("l1", None), ("lp", 1), ("lp", 2), ("lp", 0.5), ("lp", 1.5), ("lp", 3)):
        v, nv = T.values(rows, q, metric, p), T.naive_values(rows, q, "l1" if p == 1 else metric, p)
        rel = float((np.abs(v - nv) / nv).max())
        print("d=%d %s p=%s: max relative difference %.3g (bound %.3g)" % (d, metric, p, rel, (d + 2) * 2.0 ** -52))
        assert rel <= (d + 2) * 2.0 ** -52
    assert np.array_equal(T.values(rows, q, "lp", 1).view(np.uint64), T.values(rows, q, "l1").view(np.uint64))


def test_truth_p2_is_the_fma_chain():
    """lane_sums(op "sq") against the chain written out with exact rational fused multiply-adds, one row."""
    rows, q = _data(2, 1, 259, 1)
    lanes = T.lane_sums(rows, q[0], "sq")[0]
    diff = (q[0].astype(np.float64) - rows[0].astype(np.float64)).tolist()
    for lane in (0, 1, 63):
        acc = 0.0
        for c in [c for c in range(259) if (c % 256) // 4 == lane]:
            acc = float(Fraction(diff[c]) * Fraction(diff[c]) + Fraction(acc))
        assert acc == lanes[lane]


def test_truth_exact_zero_and_topk_order():
    rows = np.array([[1, 0], [0, 0], [1, 0], [-1, 0], [0, 0]], dtype=np.float32)
    q = np.array([[0, 0]], dtype=np.float32)
    v = T.values(rows, q, "l1")
    assert v.tolist() == [[1.0, 0.0, 1.0, 1.0, 0.0]] and not np.signbit(v).any()
    ids, val = T.topk(v, 7, row_offset=10)
    assert ids.tolist() == [[11, 14, 10, 12, 13, -1, -1]] and val[0, 5:].tolist() == [math.inf, math.inf]
    ids, _ = T.topk(v, 2, allow=np.array([1, 0, 1, 1, 0], dtype=bool))
    assert ids.tolist() == [[0, 2]]


def test_lp_reference_topk_is_the_exhaustive_one():
    rows, q = _data(3, 300, 40, 2)
    ids, val = T.lp_reference_topk(rows, q, 1.5, 16)
    for i in range(2):
        full = T.lp_reference(rows, q[i], 1.5, np.arange(300))
        order = np.lexsort((np.arange(300), full))[:17]
        assert np.array_equal(ids[i], order) and np.array_equal(val[i], full[order])


def test_binding_checks_raise_before_any_device_call():
    from isehr_amd import _lib
    from isehr_amd.knn import KNN
    assert _lib.minkowski_args("l1", None, 1) == (_lib.MINK_L1, 0.0)
    assert _lib.minkowski_args("linf", 7.0, 2048) == (_lib.MINK_LINF, 0.0)
    assert _lib.minkowski_args("lp", 0.5, 5) == (_lib.MINK_LP, 0.5)
    for metric, p, k in (("l2", None, 1), ("lp", 0.0, 1), ("lp", -1.0, 1), ("lp", float("nan"), 1), ("lp", float("inf"), 1),
                         ("lp", None, 1), ("l1", None, 0), ("l1", None, 2049), ("linf", None, -3)):
        with pytest.raises(ValueError):
            _lib.minkowski_args(metric, p, k)
    # the entry points of the binding run those checks first: no handle is read (there is none), no library is loaded
    g = _lib.Gallery.__new__(_lib.Gallery)
    g._h = None
    for kw in (dict(metric="cityblock"), dict(metric="lp", p=0), dict(metric="lp", p=float("nan")), dict(k=0), dict(k=2049)):
        args = dict(k=3, metric="l1", p=None)
        args.update(kw)
        with pytest.raises(ValueError):
            g.search_minkowski(np.zeros((1, 4), np.float32), **args)
        with pytest.raises(ValueError):
            g.search_minkowski_device(0, 1, args["k"], 0, metric=args["metric"], p=args["p"])
    x = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError):
        KNN(x, "lp", p=-0.5)
    with pytest.raises(ValueError):
        KNN(x, "lp")
    with pytest.raises(NotImplementedError):
        KNN(x, "chebyshev")


def test_header_values_match_the_binding():
    import os
    import re
    from isehr_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355_retrieval.h")).read()
    got = {name: int(v) for name, v in re.findall(r"#define (MI_MINK_[A-Z0-9]+) (\d+)", hdr)}
    assert got == {"MI_MINK_L1": _lib.MINK_L1, "MI_MINK_LINF": _lib.MINK_LINF, "MI_MINK_LP": _lib.MINK_LP}
    assert "mi_knn_search_minkowski" in _lib.SIGNATURES and "mi_knn_search_minkowski_device" in _lib.SIGNATURES


def test_matcher_table_and_default_p():
    from isehr_amd import nnsearch
    assert nnsearch.MATCHING_METHODS["Lp"] is nnsearch.matching_Lp_hip
    assert inspect.signature(nnsearch.matching_Lp_hip).parameters["p"].default == 0.5
    assert inspect.signature(nnsearch.matching_fractional_dis_hip).parameters["p"].default == 2
    assert list(inspect.signature(nnsearch.matching_Lp_hip).parameters)[:3] == ["K", "embedded_features_train",
                                                                               "embedded_features_test"]
    assert nnsearch.MATCHING_METHODS["L2"] is nnsearch.matching_L2_hip          # the existing keys stay
