"""Exact host truth for the small kernels every multi-shard and every query-expansion answer goes through, and the inputs
their tests share (plain Python / numpy, no GPU):

  merge_kernel<true|false>      csrc/select.hip   merge_truth, sorted_shard_lists, MERGE_SIZES / MERGE_KINDS
  kth_of_gathered_kernel        csrc/select.hip   kth_truth, kth_inputs, KTH_SIZES / KTH_KINDS
  aqe_partial / rows / combine  csrc/aqe.hip      weighted_gather_truth (a chain of correctly rounded fma in j order)
  aqe_weight                    csrc/aqe.hip      weight_truth (((k-j)/k)^w at 80 decimal digits)
  aqe_finish_kernel             csrc/aqe.hip      finish_truth
  column_sum_kernel             csrc/aqe.hip      column_sum_truth (math.fsum)

tests/test_shard_aux_truth_cpu.py pins these helpers to the oracle and checks the generators; tests/test_gpu_shard_merge.py and
tests/test_gpu_query_expansion_sums.py compare the kernels with them.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64


# ------------------------------------------------------------------------------------------------ merge
def _merge_key(s, i):
    """(NaN last, score descending with -0.0 == +0.0, id ascending): -s compares -0.0 and +0.0 as equal."""
    nan = s != s
    return (nan, 0.0 if nan else -s, i)


def merge_truth(score64, idx, k):
    """score64 [S,Q,k] float64, idx [S,Q,k] int64 -> (idx int64 [Q,k], score float32 [Q,k]): entries with idx < 0 dropped
    whatever their score, the rest ordered by _merge_key, the first k kept, the tail padded with -1 / -inf."""
    score64, idx = np.asarray(score64, dtype=np.float64), np.asarray(idx, dtype=np.int64)
    nq = score64.shape[1]
    out_i = np.full((nq, k), -1, dtype=np.int64)
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    for q in range(nq):
        s, i = score64[:, q, :].reshape(-1), idx[:, q, :].reshape(-1)
        ent = sorted((_merge_key(float(a), int(b)) + (float(a),) for a, b in zip(s, i) if b >= 0))[:k]
        for p, (_, _, b, a) in enumerate(ent):
            out_i[q, p] = b
            with np.errstate(over="ignore"):
                out_s[q, p] = np.float32(a)
    return out_i, out_s


# (nshards, k): one entry per thread at 256, the last size staged in LDS (3072 entries = 48 KiB), the first and the last
# that are searched in global memory
MERGE_SIZES = [(1, 1), (1, 100), (2, 7), (3, 64), (8, 32), (3, 100), (3, 1024), (3, 1025), (8, 1024)]
MERGE_NQ = (1, 5)
MERGE_KINDS = ("distinct", "ties", "short", "special")
_SPECIAL = [np.inf, -np.inf, 0.0, -0.0, 1e39, -1e39, 1e300, 1e-300, -1e-300, 1e-40, 3.5, -3.5, 1.0]


def sorted_shard_lists(kind, nshards, nq, k, seed=0):
    """-> (score64 [S,Q,k], idx [S,Q,k], NaNs planted): every list sorted by _merge_key with its padding (idx -1) at the tail,
    ids disjoint across the shards of a query -- the merge's stated precondition.
      distinct  full lists of distinct random scores
      ties      full lists, scores from three values, id % nshards == shard: nearly every tie is decided by id across lists
      short     valid counts per shard from {0, 1, k // 2, k}; query q % 5 == 0: only shard 0 holds entries, k // 2 of
                them (total below k); q % 5 == 1: every shard empty
      special   +-inf, +-0.0, values beyond the float32 range on both sides, up to two NaN at the end of a list's valid
                part; odd shards are one entry short and carry +inf, not -inf, as their padding's score"""
    assert kind in MERGE_KINDS
    rng = np.random.default_rng([seed, MERGE_KINDS.index(kind), nshards, nq, k])
    score = np.full((nshards, nq, k), -np.inf, dtype=np.float64)
    idx = np.full((nshards, nq, k), -1, dtype=np.int64)
    planted = 0
    for q in range(nq):
        if kind == "ties":
            ids = [rng.permutation(2 * k)[:k] * nshards + s for s in range(nshards)]
        else:
            perm = rng.permutation(2 * nshards * k) + 1000 * q
            ids = [perm[s * k:(s + 1) * k] for s in range(nshards)]
        for s in range(nshards):
            c = k
            if kind == "short":
                c = int(rng.choice([0, 1, k // 2, k]))
                if q % 5 == 0:
                    c = k // 2 if s == 0 else 0
                elif q % 5 == 1:
                    c = 0
            elif kind == "special":
                c = k - (s % 2 if k > 1 else 0)
                score[s, q, :] = np.inf if s % 2 else -np.inf
            if kind == "ties":
                v = rng.choice([0.25, 0.5, 0.75], size=c)
            else:
                v = rng.standard_normal(c)
            if kind == "special":
                v = np.where(rng.random(c) < 0.5, rng.choice(_SPECIAL, size=c), v)
                nn = min(c, (s + q) % 3)
                if nn:
                    v[rng.permutation(c)[:nn]] = np.nan
                    planted += nn
            ent = sorted(_merge_key(float(a), int(b)) + (float(a),) for a, b in zip(v, ids[s][:c]))
            for p, (_, _, b, a) in enumerate(ent):
                score[s, q, p], idx[s, q, p] = a, b
    return score, idx, planted


def lists_meet_precondition(score64, idx):
    """True when every list is strictly ascending in _merge_key over a prefix of valid entries, with nothing but padding behind
    it, and no id occurs twice among the lists of one query."""
    S, Q, k = idx.shape
    for q in range(Q):
        seen = set()
        for s in range(S):
            valid = idx[s, q] >= 0
            c = int(valid.sum())
            if not valid[:c].all():
                return False
            keys = [_merge_key(float(a), int(b)) for a, b in zip(score64[s, q, :c], idx[s, q, :c])]
            if any(not keys[i] < keys[i + 1] for i in range(c - 1)):
                return False
            ids = set(int(b) for b in idx[s, q, :c])
            if len(ids) != c or seen & ids:
                return False
            seen |= ids
    return True


# ------------------------------------------------------------------------------------------------ K-th
def f2key(x):
    """csrc/common.h f2key on a float32 array: order-preserving uint32 keys, NaN -> 0 (lowest), -0.0 one below +0.0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    key = np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(x), np.uint32(0), key).astype(np.uint32)


def key2bits(key):
    """csrc/common.h key2f, as the float's bit pattern (key 0 gives 0xFFFFFFFF, a NaN)."""
    key = np.asarray(key, dtype=np.uint32)
    return np.where(key >> 31 != 0, key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)


def kth_truth(gathered, k):
    """gathered float32 [S,Q,k] -> uint32 [Q]: the bit pattern of the k-th largest of the S*k values of every query under the
    total order of f2key.  A NaN pattern means 'any NaN'."""
    g = np.asarray(gathered, dtype=np.float32)
    out = np.empty(g.shape[1], dtype=np.uint32)
    for q in range(g.shape[1]):
        keys = np.sort(f2key(g[:, q, :].reshape(-1)))[::-1]
        out[q] = key2bits(keys[k - 1:k])[0]
    return out


def _kth_sizes():
    out = []
    for n in (1, 63, 64, 65, 255, 256, 257, 1000, 4097, 8192):
        out += [(s, n // s) for s in (1, 3, 8) if n % s == 0]
    return out


KTH_SIZES = _kth_sizes()            # (nshards, k) with nshards * k = n around the 256-thread trips of the select
KTH_NQ = 3
KTH_KINDS = ("normal", "equal", "byte0", "byte1", "byte2", "halfsign", "zeros", "denormal", "neginf", "nan", "peel")


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def _kth_values(kind, rng, nshards, k, q):
    """-> (float32 [S,k], NaNs planted) for one query."""
    n = nshards * k
    planted = 0
    if kind == "normal":
        v = rng.standard_normal(n).astype(np.float32)
    elif kind == "equal":
        v = np.full(n, 1.5 + q, dtype=np.float32)
    elif kind in ("byte0", "byte1", "byte2"):       # keys that agree everywhere but in one byte
        sh = 8 * int(kind[-1])
        v = _bits(np.uint32(0x3F000000 + (q << 24 if sh != 24 else 0)) | (rng.integers(0, 256, n).astype(np.uint32) << sh))
    elif kind == "halfsign":
        v = np.full(n, 2.75 + q, dtype=np.float32)
        v[rng.permutation(n)[:n // 2]] *= -1
    elif kind == "zeros":
        v = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    elif kind == "denormal":
        v = _bits(rng.integers(1, 0x800000, n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 31))
    elif kind == "neginf":                          # fewer than k finite values in all shards together: the K-th is -inf
        v = np.full((nshards, k), -np.inf, dtype=np.float32)
        real = k // (2 * nshards)
        v[:, :real] = rng.standard_normal((nshards, real))
        return v, 0
    elif kind == "nan":
        v = rng.standard_normal(n).astype(np.float32)
        planted = min(3, n)
        v[rng.permutation(n)[:planted]] = _bits(rng.choice([0x7FC00000, 0xFFC00001, 0x7F800001], size=planted))
    else:                                           # peel: eight top-byte digits among the lanes of every wave, ~8 lanes each
        assert kind == "peel"
        v = (rng.choice([1.0, 4.0, 16.0, 64.0, 256.0, 1024.0, 4096.0, 16384.0], size=n) * (1.0 + rng.random(n)) *
             rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    return v.reshape(nshards, k), planted


def kth_inputs(first_kind, nshards, k, seed=0):
    """-> (gathered float32 [S, KTH_NQ, k], NaNs planted).  Query q holds the content KTH_KINDS[(first_kind + q) % 11], so a
    mix-up between queries shows."""
    rng = np.random.default_rng([seed, first_kind, nshards, k])
    g = np.empty((nshards, KTH_NQ, k), dtype=np.float32)
    planted = 0
    for q in range(KTH_NQ):
        v, p = _kth_values(KTH_KINDS[(first_kind + q) % len(KTH_KINDS)], rng, nshards, k, q)
        g[:, q, :] = v
        planted += p
    return g, planted


# ------------------------------------------------------------------------------------------------ weighted gather
def _fma(x, w, acc):
    """round_f64(x * w + acc), one rounding: float(Fraction) is a correctly rounded integer division."""
    prod = Fraction(x) * Fraction(w)
    exact = prod + Fraction(acc)
    if exact == 0:
        if prod == 0 and acc == 0:                  # a sum of zeros is -0 only when both are
            pneg = math.copysign(1.0, x) * math.copysign(1.0, w) < 0
            return -0.0 if pneg and math.copysign(1.0, acc) < 0 else 0.0
        return 0.0                                  # exact cancellation: +0 in round-to-nearest
    return float(exact)


def weighted_gather_truth(rows_f32, ranks, weights_f64, row_offset=0, n=None):
    """rows_f32 [n,d] (the shard's rows; global id = row_offset + local row), ranks int64 [k,Q] global ids, weights [k]
    -> float64 [Q,d]: acc = fma(x, w_j, acc) in j order from +0, ids outside [row_offset, row_offset + n) skipped --
    csrc/aqe.hip aqe_step, bit for bit."""
    rows = np.asarray(rows_f32)
    assert rows.dtype == np.float32
    n = rows.shape[0] if n is None else n
    ranks = np.asarray(ranks, dtype=np.int64)
    w = [float(v) for v in np.asarray(weights_f64, dtype=np.float64)]
    k, nq = ranks.shape
    out = np.zeros((nq, rows.shape[1]), dtype=np.float64)
    for q in range(nq):
        own = [(j, int(ranks[j, q]) - row_offset) for j in range(k)]
        own = [(j, r) for j, r in own if 0 <= r < n]
        for c in range(rows.shape[1]):
            acc = 0.0
            for j, r in own:
                acc = _fma(float(rows[r, c]), w[j], acc)
            out[q, c] = acc
    return out


W_GRID = (0.0, 0.5, 1.0, 2.0, 2.5, 3.0, 4.0, 8.0)
K_QE_GRID = tuple(range(1, 33))


def weight_truth(k_qe, w, other=None):
    """-> (float64 [k_qe] = ((k_qe - j) / k_qe) ** w rounded once from 80 decimal digits, error of `other` in ulps of those
    values against the unrounded ones -- float64 [k_qe], or None without `other`)."""
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        exact = []
        for j in range(k_qe):
            base = decimal.Decimal(k_qe - j) / decimal.Decimal(k_qe)
            exact.append(decimal.Decimal(1) if (w == 0 or j == 0) else base ** decimal.Decimal(float(w)))
        w64 = np.array([float(v) for v in exact], dtype=np.float64)
        err = None
        if other is not None:
            other = np.asarray(other, dtype=np.float64)
            assert other.shape == (k_qe,) and np.all(np.isfinite(other))
            err = np.array([float(abs(decimal.Decimal(float(o)) - v) / decimal.Decimal(float(np.spacing(t))))
                            for o, v, t in zip(other, exact, w64)])
    return w64, err


# ------------------------------------------------------------------------------------------------ finish
def finish_truth(sum64, eps):
    """sum64 [Q,d] float64 -> float64 [Q,d] = sum / (norm + eps): the norm is the square root of the exact sum of squares
    (Fraction), taken at 80 digits and rounded once; the add and the divide are float64 operations."""
    s = np.asarray(sum64, dtype=np.float64)
    out = np.empty_like(s)
    with decimal.localcontext() as ctx:
        ctx.prec = 80
        for q in range(s.shape[0]):
            ss = sum((Fraction(float(v)) ** 2 for v in s[q]), Fraction(0))
            nrm = float((decimal.Decimal(ss.numerator) / decimal.Decimal(ss.denominator)).sqrt())
            out[q] = s[q] / np.float64(nrm + eps)
    return out


# ------------------------------------------------------------------------------------------------ column sums
def column_sum_truth(X):
    """float64 [d]: math.fsum of every column (exactly rounded sum)."""
    X = np.asarray(X)
    return np.array([math.fsum(float(v) for v in X[:, c]) for c in range(X.shape[1])], dtype=np.float64)


def integer_matrix(n, d, dtype, seed=0):
    """Integers in [-2^20, 2^20]: every partial sum of up to 2^32 of them is exact in float64, in any order."""
    rng = np.random.default_rng([seed, n, d])
    return rng.integers(-(1 << 20), (1 << 20) + 1, size=(n, d)).astype(dtype)


def in_layout(X, layout, poison=np.nan):
    """X [n,d] -> a view with the same values: 'contiguous'; 'rows' (row stride d + 3, the gap poisoned); 'transposed' (row
    stride 1, column stride n + 2: the [D,N] array of the reference, the gap poisoned)."""
    n, d = X.shape
    if layout == "contiguous":
        return np.ascontiguousarray(X)
    if layout == "rows":
        big = np.full((n, d + 3), poison, dtype=X.dtype)
        big[:, :d] = X
        return big[:, :d]
    assert layout == "transposed"
    big = np.full((d, n + 2), poison, dtype=X.dtype)
    big[:, :n] = X.T
    return big[:, :n].T


LAYOUTS = ("contiguous", "rows", "transposed")
