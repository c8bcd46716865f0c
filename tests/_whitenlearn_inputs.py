"""Inputs and distance measures shared by scripts/make_whitenlearn_golden.py (which records the reference's answers in
tests/golden/whitenlearn.npz) and the whitening-learning tests (which regenerate the inputs from the recorded parameters).

Every input is a pure function of (kind, seed) built from synth.py's integer-exact generator with integer arithmetic only, so
that the [D, N] matrix is the same bits on every machine, whatever BLAS numpy was built with:
  graded  an orthogonal mix (a 64 x 64 Hadamard matrix / 8) of coordinates with geometrically spaced scales 1 ... 0.05
          (rounded to 1 / 256), plus a non-zero mean;
  gem     non-negative columns (|z| times the same scales), L2-normalised: the shape of GeM descriptors.
The last N_PAIRS columns are noisy copies of seeded earlier columns: the (q, p) pairs of the supervised learner.
"""
import numpy as np

from isehr_amd.synth import splitmix64, synth_rows

D, N, N_PAIRS = 64, 3000, 800
KINDS = ("graded", "gem")
U = 2.0 ** -53


def _int_rows(seed, nrows):
    """synth_rows as exact integers (value * 2^15), int64 [nrows, D]."""
    return np.rint(synth_rows(seed, 0, nrows, D).astype(np.float64) * 2.0 ** 15).astype(np.int64)


def _hadamard():
    h = np.array([[1]], dtype=np.int64)
    while h.shape[0] < D:
        h = np.block([[h, h], [h, -h]])
    return h


def _scales():
    return np.rint(np.geomspace(1.0, 0.05, D) * 256).astype(np.int64)          # 256 ... 13


def make_input(kind, seed):
    """-> (X float64 [D, N], qidxs int64 [N_PAIRS], pidxs int64 [N_PAIRS])."""
    nb = N - N_PAIRS
    z = _int_rows(seed, N)                                   # [N, D], |z| < 2^18
    s = _scales()
    qidxs = (splitmix64(np.arange(N_PAIRS, dtype=np.uint64) + np.uint64(seed * 7919)) % np.uint64(nb)).astype(np.int64)
    pidxs = np.arange(nb, N, dtype=np.int64)
    if kind == "graded":
        base = (z * s[None, :]) @ _hadamard().T                # exact: < 2^18 * 2^8 * 2^6
        noise = (_int_rows(seed + 1, N_PAIRS) * s[None, :]) @ _hadamard().T
        base[nb:] = 4 * base[qidxs] + noise                   # p = q + noise / 4, in units of a quarter
        base[:nb] *= 4
        mean = (np.arange(D, dtype=np.int64) % 7 - 2) * 2 ** 26      # (i % 7 - 2) / 4 in the unit 2^-28
        X = (base + mean[None, :]).astype(np.float64) * 2.0 ** -28   # unit: 2^-15 / 256 / 8 / 4
    elif kind == "gem":
        base = np.abs(z) * s[None, :]
        noise = np.abs(_int_rows(seed + 1, N_PAIRS)) * s[None, :]
        base[nb:] = 4 * base[qidxs] + noise
        base[:nb] *= 4
        ss = (base * base).sum(axis=1)                         # exact in int64: 64 * 2^56
        X = base.astype(np.float64) / np.sqrt(ss.astype(np.float64))[:, None]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(X.T), qidxs, pidxs


def as_dtype(X, dtype):
    """The f32 cases: the input rounded to float32 (what the device is given); the reference sees it promoted back."""
    return X.astype(np.float32) if dtype == "f32" else X


def chunked_scatter(X, centre, chunk=37):
    """float64 scatter matrix of the columns of X [D, N] about centre [D], accumulated over chunks of `chunk` columns."""
    Xc = np.asarray(X, dtype=np.float64) - np.asarray(centre, dtype=np.float64).reshape(-1, 1)
    C = np.zeros((X.shape[0], X.shape[0]))
    for c0 in range(0, X.shape[1], chunk):
        b = Xc[:, c0:c0 + chunk]
        C += b @ b.T
    return (C + C.T) / 2


def chunked_pair_scatter(X, q, p, chunk=37):
    df = np.asarray(X[:, q], dtype=np.float64) - np.asarray(X[:, p], dtype=np.float64)
    return chunked_scatter(df, np.zeros(X.shape[0]), chunk)


def rows_distance(P, P_ref):
    """max |sign-fixed P - P_ref| / max |P_ref|: every row of P is multiplied by sign(<P_row, P_ref_row>)."""
    sgn = np.sign(np.sum(P * P_ref, axis=1))
    sgn[sgn == 0] = 1.0
    return float(np.max(np.abs(P * sgn[:, None] - P_ref)) / np.max(np.abs(P_ref)))


def gram_distance(P, P_ref):
    g, gr = P.T @ P, P_ref.T @ P_ref
    return float(np.max(np.abs(g - gr)) / np.max(np.abs(gr)))


def whitenapply_numpy(X, m, P, dims):
    Y = P[:dims] @ (np.asarray(X, dtype=np.float64) - m)
    return Y / (np.linalg.norm(Y, ord=2, axis=0, keepdims=True) + 1e-6)


def whitened_gram(Y):
    return Y.T @ Y


def top10_sets(G, G_ref, guard=1e-9):
    """Top-10 of every column against all others by G and by G_ref -> (columns compared, columns whose sets differ, share of
    columns left out because the reference's own 10th and 11th scores differ by <= guard)."""
    n = G.shape[0]
    a, b = G.copy(), G_ref.copy()
    np.fill_diagonal(a, -np.inf)
    np.fill_diagonal(b, -np.inf)
    order_ref = np.argsort(-b, axis=1, kind="stable")[:, :11]
    sref = np.take_along_axis(b, order_ref, axis=1)
    keep = (sref[:, 9] - sref[:, 10]) > guard
    top = np.argsort(-a, axis=1, kind="stable")[:, :10]
    differ = 0
    for i in np.nonzero(keep)[0]:
        if set(top[i]) != set(order_ref[i, :10]):
            differ += 1
    return int(keep.sum()), differ, float(1.0 - keep.mean())


def relative_gaps(eigval):
    ev = np.sort(np.asarray(eigval, dtype=np.float64))[::-1]
    return np.abs(np.diff(ev)) / np.abs(ev[:-1])
