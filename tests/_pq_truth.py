"""Pure-numpy truth of the PQ index (tests only): float64 table entries rounded once to float32, float32 sums in book order,
order by (distance, id); the tie-aware comparison against the reference's matching_PQ_Net for the golden fixture."""
import numpy as np


def dtable64(x, C):
    """x [Q, M * L] float32/float64, C [M, Ks, L] float32 -> (acc float64 [Q, M, Ks], acc.astype(float32)).
    acc[q, m, c] = sum_j (double(x[q, m L + j]) - double(C[m, c, j]))^2, ascending j, one multiply and one add per term."""
    x = np.asarray(x)
    C = np.asarray(C, np.float32)
    M, Ks, L = C.shape
    nq = x.shape[0]
    xt = np.ascontiguousarray(x.astype(np.float64).reshape(nq, M, L).transpose(2, 0, 1))[..., None]      # [L][Q, M, 1]
    Ct = np.ascontiguousarray(C.astype(np.float64).transpose(2, 0, 1))[:, None]                          # [L][1, M, Ks]
    acc = np.zeros((nq, M, Ks), np.float64)
    step = max(1, (1 << 17) // (M * Ks))                # rows per block: the three arrays of a block stay in cache
    for r in range(0, nq, step):
        a = acc[r:r + step]
        d = np.empty_like(a)
        for j in range(L):
            np.subtract(xt[j, r:r + step], Ct[j], out=d)
            np.multiply(d, d, out=d)
            a += d
    with np.errstate(over="ignore"):
        return acc, acc.astype(np.float32)


def encode_truth(x, C, prune=True):
    """-> uint8 [N, M]: np.argmin of the float64 sums of dtable64, ties to the lower codeword.
    prune=False is that sentence as it stands.  prune=True gives the same codes in a fraction of the time: a float64 matrix
    product (||x||^2 - 2 x.c + ||c||^2) ranks the codewords of a book approximately, and only those within `eps` of the
    approximate minimum get the sequential sum, among which the (sum, index) minimum is taken.  The product form and the
    sequential sum are both within L * 2^-50 * (||x||^2 + ||c||^2) of the real value; eps is 2^20 times that, so the true
    argmin (and every codeword tied with it) is always among the candidates."""
    x = np.asarray(x)
    C = np.asarray(C, np.float32)
    M, Ks, L = C.shape
    out = np.empty((x.shape[0], M), np.uint8)
    if not prune:
        for r in range(0, out.shape[0], 256):
            out[r:r + 256] = np.argmin(dtable64(x[r:r + 256], C)[0], axis=-1)
        return out
    x64 = x.astype(np.float64).reshape(x.shape[0], M, L)
    C64 = C.astype(np.float64)
    cn = (C64 * C64).sum(-1)                                            # [M, Ks]
    for m in range(M):
        xm = x64[:, m]                                                  # [N, L]
        xn = (xm * xm).sum(-1)[:, None]
        approx = xn - 2.0 * (xm @ C64[m].T) + cn[m][None]
        eps = L * 2.0 ** -30 * (xn + cn[m].max() + 1e-300)
        rows, cols = np.nonzero(approx <= approx.min(-1, keepdims=True) + eps)
        acc = np.zeros(rows.size, np.float64)
        for j in range(L):
            d = xm[rows, j] - C64[m, cols, j]
            acc += d * d
        order = np.lexsort((cols, acc, rows))                           # per row: smallest sum first, then the lower codeword
        first = np.ones(rows.size, bool)
        first[1:] = rows[order][1:] != rows[order][:-1]
        out[rows[order][first], m] = cols[order][first]
    return out


def adc_truth(T32, codes):
    """T32 float32 [Q, M, Ks], codes integer [N, M] -> float32 [Q, N]: sequential float32 sums in ascending book order."""
    T32 = np.asarray(T32, np.float32)
    codes = np.asarray(codes).astype(np.int64)
    acc = np.zeros((T32.shape[0], codes.shape[0]), np.float32)
    for m in range(codes.shape[1]):
        acc = acc + T32[:, m, codes[:, m]]
    return acc


def pq_truth(x, C, codes, k, row_offset=0, allowed=None):
    """-> (ids int64 [Q, k], dist float32 [Q, k]) by (distance asc, id asc) over the rows `allowed` (bool [N]) admits, padded
    with -1 / +inf."""
    dist_all = adc_truth(dtable64(x, C)[1], codes)
    nq, n = dist_all.shape
    ids = np.full((nq, k), -1, np.int64)
    dist = np.full((nq, k), np.inf, np.float32)
    rows = np.arange(n, dtype=np.int64) if allowed is None else np.flatnonzero(np.asarray(allowed, bool)).astype(np.int64)
    for i in range(nq):
        d = dist_all[i, rows]
        order = np.lexsort((rows, d))[:k]
        ids[i, :order.size] = rows[order] + int(row_offset)
        dist[i, :order.size] = d[order]
    return ids, dist


def books_of(codewords, n_books):
    """The reference's Codewords [Ks, M * L] -> codebooks [M, Ks, L]."""
    cw = np.asarray(codewords)
    return np.ascontiguousarray(cw.reshape(cw.shape[0], n_books, cw.shape[1] // n_books).transpose(1, 0, 2))


def tie_aware_vs_reference(idx_ref, idx_ours, codewords, query, n_books, codes):
    """The comparison against the reference's unstable argsort over float32 sums.  With d64 the float64 ADC distances and
    tau = (L + 2 M + 4) * 2^-24 (the reference rounds L products and sums per entry and then M - 1 adds; the contract rounds
    once per entry and then M - 1 adds; four units of slack): at every output position the float64 distances of the
    reference's id and of ours differ by at most tau * d64, and per query the sets of ids whose float64 distance lies below
    (1 - tau) times the K-th distance are equal.  -> list of complaints."""
    C = books_of(codewords, n_books)
    M, _, L = C.shape
    tau = (L + 2 * M + 4) * 2.0 ** -24
    acc = dtable64(query, C)[0]
    codes = np.asarray(codes).astype(np.int64)
    bad = []
    for q in range(acc.shape[0]):
        d64 = np.zeros(codes.shape[0], np.float64)
        for m in range(M):
            d64 += acc[q, m, codes[:, m]]
        dr, do = d64[idx_ref[q]], d64[idx_ours[q]]
        if not (np.abs(dr - do) <= tau * np.minimum(dr, do)).all():
            bad.append("query %d: float64 distances differ by up to %g (relative)" % (q, (np.abs(dr - do) / np.minimum(dr, do)).max()))
            continue
        cut = (1.0 - tau) * min(dr[-1], do[-1])
        if set(idx_ref[q][dr < cut].tolist()) != set(idx_ours[q][do < cut].tolist()):
            bad.append("query %d: ids below the K-th distance differ" % q)
    return bad
