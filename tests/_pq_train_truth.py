"""Pure-numpy truth of mi_pq_train (tests only): the contract of DESIGN.md 5.14b on top of _pq_truth.encode_truth, and the
clustered problems the CPU and GPU tests share."""
import numpy as np

from _pq_truth import encode_truth


def default_init(x, M, Ks):
    """C_0 of a NULL init: codeword c of every book is the book's slice of row floor(c * n / Ks), rounded to float32."""
    x = np.asarray(x)
    n, d = x.shape
    L = d // M
    rows = (np.arange(Ks, dtype=np.int64) * n) // Ks
    return np.ascontiguousarray(x[rows].reshape(Ks, M, L).transpose(1, 0, 2)).astype(np.float32)


def rows_init(x, M, init_rows):
    """C_0 of init_rows [M, Ks]: codeword c of book j is book j's slice of row init_rows[j, c], rounded to float32."""
    x = np.asarray(x)
    L = x.shape[1] // M
    return np.stack([x[np.asarray(init_rows)[j], j * L:(j + 1) * L] for j in range(M)]).astype(np.float32)


def update_truth(x, codes, C):
    """One centroid update: per (book, codeword) the float64 sum of the members in ASCENDING row order from +0.0 (np.add.accumulate
    over a block that starts with a zero row adds row by row), one float64 divide, one rounding to float32; a codeword
    without members keeps its value."""
    x = np.asarray(x)
    M, Ks, L = C.shape
    out = np.array(C, np.float32, copy=True)
    for j in range(M):
        xj = x[:, j * L:(j + 1) * L].astype(np.float64)
        for c in range(Ks):
            members = np.flatnonzero(codes[:, j] == c)              # ascending
            if members.size == 0:
                continue
            block = np.concatenate([np.zeros((1, L), np.float64), xj[members]])
            s = np.add.accumulate(block, axis=0)[-1]
            out[j, c] = (s / np.float64(members.size)).astype(np.float32)
    return out


def train_truth(x, M, Ks, iters, C0):
    """-> (C float32 [M, Ks, L], moved int64 [iters]): assign with encode_truth, count the moves (moved[0] = n * M; a zero
    after the first iteration stops the training and the rest stays zero), update."""
    x = np.asarray(x)
    C = np.ascontiguousarray(C0, dtype=np.float32).copy()
    assert C.shape == (M, Ks, x.shape[1] // M)
    moved = np.zeros(iters, np.int64)
    prev = None
    for t in range(iters):
        codes = encode_truth(x, C)
        moved[t] = codes.size if prev is None else int((codes != prev).sum())
        if t > 0 and moved[t] == 0:
            break
        C = update_truth(x, codes, C)
        prev = codes
    return C, moved


def clustered(rng, n, M, Ks, L):
    """The generator of the issue, in its order of draws: centres 3 * randn, labels, ONE randn call for the noise, then the
    initial rows of every book.  -> (x float32 [n, M * L], init_rows [M, Ks])"""
    cent = rng.randn(M, Ks, L) * 3
    lab = rng.randint(0, Ks, (n, M))
    noise = rng.randn(n, M, L)
    x = (cent[np.arange(M)[None, :], lab] + 0.5 * noise).reshape(n, M * L).astype(np.float32)
    init = np.stack([rng.choice(n, Ks, replace=False) for _ in range(M)])
    return x, init
