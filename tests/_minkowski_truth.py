"""numpy truth of the Minkowski search (csrc/minkowski.hip): the value contract restated, no device, no library.

With t_j = |float64(q_j) - float64(g_j)| over the d columns of a stored float32 row g and a float32 query q:

    "l1"            sum t_j            "linf"   max t_j
    "lp", p == 1    the bits of "l1"   "lp", p == 2   sum t_j^2, each term one fused multiply-add (the bits of l2_direct_wave)
    "lp", p == 0.5  sum sqrt(t_j)      "lp", other p  sum pow(t_j, p)            (none raised to 1 / p)

The sums run in ONE order: lane l of 64 adds the columns 4 l + 256 i + {0, 1, 2, 3} in ascending order into one accumulator that
starts at +0; the 64 accumulators are combined by an xor butterfly (lane l adds lane l ^ 32, then l ^ 16, ... l ^ 1).  lane_sums
and butterfly below do exactly that in float64, so "l1" and p == 2 come out bit for bit, and p == 0.5 / other p up to the
device's sqrt and pow.  lp_reference is the high-accuracy value (math.fsum of Python-float t ** p: every term rounded once, the
sum exact), topk the exact top-k by (value, id) with padding."""
import math

import numpy as np

QT = 8                      # queries of a scan tile at d <= 2560 (kernels.h mink_query_tile)
SLAB = 2048                 # rows of a selection slab; rows per select workgroup = a multiple of it (kernels.h mink_part_rows)
BLOCK_ROWS = 256            # rows per scan workgroup
MAX_K = 2048


# ---------------------------------------------------------------------------------------------- exact fused multiply-add
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    c = 134217729.0 * a                                   # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """round_f64(a * b + c) with ONE rounding, elementwise on float64 arrays (Boldo and Melquiond, "Emulation of a FMA and
    correctly rounded sums", 2008: the exact product as hi + lo, TwoSum of c and hi, the two small parts added with rounding to
    odd, one final rounding to nearest).  Finite values away from overflow and underflow, which is all the tests feed it;
    test_minkowski_cpu.py checks it against exact rational arithmetic."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    v, err = _two_sum(tl, ul)
    # rounding to odd: where tl + ul was inexact and v's last mantissa bit is even, move v one ulp towards the lost part
    even = (v.view(np.uint64) & np.uint64(1)) == 0
    fix = (err != 0) & even
    v = np.where(fix, np.nextafter(v, np.where(err > 0, np.inf, -np.inf)), v)
    return th + v


# ---------------------------------------------------------------------------------------------- the value contract
def op_of(metric, p=None):
    if metric == "l1" or (metric == "lp" and p == 1):
        return "l1"
    if metric == "linf":
        return "linf"
    assert metric == "lp" and p is not None and math.isfinite(p) and p > 0
    return {2: "sq", 0.5: "sqrt"}.get(p, "pow")


def _terms(rows_f32, q_f32):
    """q - g in float64, [n, d] for one query"""
    assert rows_f32.dtype == np.float32 and q_f32.dtype == np.float32
    return q_f32.astype(np.float64)[None, :] - rows_f32.astype(np.float64)


def lane_sums(rows_f32, q_f32, op, p=None):
    """-> float64 [n, 64]: the accumulator of every lane for one query, columns taken in the lane's order."""
    n, d = rows_f32.shape
    diff = _terms(rows_f32, q_f32)
    steps = -(-d // 256)
    pad = np.zeros((n, steps * 256), dtype=np.float64)           # a column beyond d adds t = 0: the accumulator keeps its bits
    pad[:, :d] = diff
    t = pad.reshape(n, steps, 64, 4)
    acc = np.zeros((n, 64), dtype=np.float64)
    for i in range(steps):
        for j in range(4):
            x = t[:, i, :, j]
            if op == "sq":
                acc = fma(x, x, acc)
            elif op == "l1":
                acc = acc + np.abs(x)
            elif op == "sqrt":
                acc = acc + np.sqrt(np.abs(x))
            else:
                acc = acc + np.abs(x) ** float(p)
    return acc


def butterfly(acc):
    """[n, 64] -> [n]: lane l adds lane l ^ o for o = 32, 16, ... 1; every lane ends with the same bits."""
    lanes = np.arange(64)
    x = np.array(acc, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[:, lanes ^ o]
    assert (x == x[:, :1]).all()
    return x[:, 0].copy()


def values(rows_f32, queries_f32, metric, p=None):
    """-> float64 [nq, n]: the contract's value of every (query, row) pair."""
    rows_f32, queries_f32 = np.asarray(rows_f32), np.asarray(queries_f32)
    op = op_of(metric, p)
    out = np.empty((queries_f32.shape[0], rows_f32.shape[0]), dtype=np.float64)
    for i, q in enumerate(queries_f32):
        if op == "linf":
            out[i] = np.abs(_terms(rows_f32, q)).max(axis=1) if rows_f32.shape[0] else 0.0
        else:
            out[i] = butterfly(lane_sums(rows_f32, q, op, p))
    return out


def naive_values(rows_f32, queries_f32, metric, p=None):
    """The same values by a plain float64 numpy evaluation, in numpy's own order."""
    t = np.abs(np.asarray(queries_f32, dtype=np.float64)[:, None, :] - np.asarray(rows_f32, dtype=np.float64)[None, :, :])
    if metric == "linf":
        return t.max(axis=-1)
    return (t if metric == "l1" else t ** float(p)).sum(axis=-1)


def lp_reference(rows_f32, q_f32, p, which):
    """-> float64 [len(which)]: sum_j t_j ** p of one query for the rows `which`, every term a Python-float power (rounded once),
    the sum by math.fsum (exact, rounded once): within 2^-52 relative of the real value."""
    diff = np.abs(_terms(np.asarray(rows_f32)[which], np.asarray(q_f32)))
    p = float(p)
    return np.array([math.fsum(t ** p for t in row) for row in diff.tolist()], dtype=np.float64)


def lp_reference_topk(rows_f32, queries_f32, p, k):
    """The high-accuracy top-(k + 1) of every query -> (ids int64 [nq, k + 1], values float64 [nq, k + 1]).  The whole gallery is
    ranked by the vectorised float64 value, whose relative error is below (d + 4) 2^-52 < 1e-12 for d < 4000; every row within
    1e-12 relative of the (k + 1)-th of them is then evaluated by lp_reference, so the true first k + 1 are among those."""
    rows_f32, queries_f32 = np.asarray(rows_f32), np.asarray(queries_f32)
    n, d = rows_f32.shape
    assert d < 4000 and k + 1 <= n
    rough = naive_values(rows_f32, queries_f32, "lp", p)
    ids = np.empty((queries_f32.shape[0], k + 1), dtype=np.int64)
    val = np.empty((queries_f32.shape[0], k + 1), dtype=np.float64)
    for i, q in enumerate(queries_f32):
        cut = np.partition(rough[i], k)[k] * (1.0 + 4e-12)
        which = np.flatnonzero(rough[i] <= cut)
        ref = lp_reference(rows_f32, q, p, which)
        order = np.lexsort((which, ref))[:k + 1]
        ids[i], val[i] = which[order], ref[order]
    return ids, val


def min_relative_gap(sorted_values):
    """The smallest (v[i + 1] - v[i]) / v[i + 1] over adjacent entries of every row of ascending positive values."""
    v = np.asarray(sorted_values, dtype=np.float64)
    return float(((v[:, 1:] - v[:, :-1]) / v[:, 1:]).min())


# ---------------------------------------------------------------------------------------------- exact top-k
def topk(vals, k, allow=None, row_offset=0):
    """vals float64 [nq, n]; allow None or a bool mask [n] -> (ids int64 [nq, k], values float64 [nq, k]): (value asc, id asc)
    over the admitted rows, ids row_offset + local row; fewer than k: ids -1, values +inf."""
    vals = np.asarray(vals, dtype=np.float64)
    nq, n = vals.shape
    rows = np.arange(n) if allow is None else np.flatnonzero(np.asarray(allow, dtype=np.bool_))
    ids = np.full((nq, k), -1, dtype=np.int64)
    out = np.full((nq, k), np.inf, dtype=np.float64)
    m = min(k, rows.size)
    for i in range(nq):
        order = rows[np.argsort(vals[i, rows], kind="stable")[:m]]         # stable: ties keep the ascending ids
        ids[i, :m] = order + row_offset
        out[i, :m] = vals[i, order]
    return ids, out


def fractional_distance(test_f32, train_f32, p):
    """The reference's fractional_distance (src/utils/nnsearch.py:46-56) in float64: (sum |x - y| ** p) ** (1 / p), [Q, N]."""
    return naive_values(train_f32, test_f32, "lp", p) ** (1.0 / float(p))


def unit_rows(a):
    """x / ||x|| per row as the reference's matchers normalise (:715-720), as stored float32 rows."""
    a = np.asarray(a)
    return np.ascontiguousarray(a / np.expand_dims(np.linalg.norm(a, axis=1), axis=1), dtype=np.float32)
