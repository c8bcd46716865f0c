"""Sparse, staged restatement of k-reciprocal re-ranking (src/utils/Reranking.py:447-624; csrc/kr_rerank.hip),
the inputs of tests/test_gpu_kr_rerank_edges.py and the assertions they share.  test_kr_rerank_cpu.py pins this module to
oracle.kr_reranking bit for bit and proves what the GPU cases claim (exposed shares, the k2 = 1 discriminator).

Plain numpy, the reference's operation order, and no dense all x all V: every row of V and V_qe is kept as (ascending columns,
values), so 16.5k images cost seconds.  Stages, in the order of the five kernels behind the exact scorer and dense_topk:

    S             all x all inner products, float32 (kept up to KEEP_S images)
    initial_rank  the k1 + 1 nearest of every image among all images by dist / column max, stable    (:502, :555)
    R[i]          k-reciprocal set, expanded where len(intersect1d) > 2./3 * len(candidate), np.unique  (:565-575)
    V[i]          float32 softmax(-dist(i, R[i]) / dmax[i]); dmax[i] = max_j dist(i, j)               (:514-525)
    V_qe[i]       k2 != 1: float16(np.mean(V[initial_rank[i, :k2]], axis=0)), rows added one after the other in float32,
                  then divided by k2; k2 == 1: V[i] itself, float32 (`if k2 != 1:`, :580)               (:580-589)
    final, order  (1 - lambda) jaccard + lambda dist / column max over the gallery columns; jaccard = 1 - m / (2 - m),
                  m = float32 sum over the ascending non-zero columns c of query i of min(V_qe[i, c], V_qe[j, c]); stable
                  argsort                                                                               (:602-618)

Two ways to form the inner products: s_form "f32" is the oracle's float32 matmul, call by call (bit-identical results);
"f64" is a float64 matmul rounded to float32, under which exact duplicate rows are exact ties, as they are for the kernel's
k-ordered chain, so the lower-index tie rule is comparable.

exposed[Q, N]: a V_qe entry whose float32 value before the float16 rounding lies within relative NEAR of a rounding boundary
can legitimately round the other way on the GPU (its S differs in the last bit); (i, j) is exposed if such an entry of row i or
row j sits in a column their Jaccard sum visits.  One flip moves a weight by ulp16(v) <= 2^-11, m by as much, and the Jaccard
distance 1 - m / (2 - m) by up to twice that (its slope 2 / (2 - m)^2 is <= 2 on m <= 1).  With k2 == 1 nothing is rounded and
nothing is exposed."""
import functools
import types

import numpy as np

TOL = 2e-6                  # what tests/test_gpu_kr_rerank.py holds for the same quantity; float32 noise is <= 1e-7
NEAR = 1e-6                 # relative distance to a float16 rounding boundary that counts as exposed
KEEP_S = 4096


def entry_bound(exposed, lambda_value):
    """TOL, plus one float16 ulp of a weight <= 1 through the Jaccard slope on exposed entries."""
    return TOL + exposed * (2.0 * (1.0 - lambda_value) * 2.0 ** -11)


def stable_smallest(d, k):
    """np.argsort(d, axis=1, kind="stable")[:, :k] without sorting whole rows: the k-th smallest of the minima of 16-element
    chunks of a row is an upper bound of the row's k-th smallest value, and only the few elements up to it are sorted."""
    m, n = d.shape
    if n <= 2048:
        return np.argsort(d, axis=1, kind="stable")[:, :k]
    cols, whole = d.T, n - n % 16
    mins = cols[:whole].reshape(-1, 16, m).min(axis=1)
    if whole < n:
        mins = np.concatenate([mins, cols[whole:].min(axis=0)[None]])
    upper = np.partition(mins, k - 1, axis=0)[k - 1]
    r, j = np.nonzero(d <= upper[:, None])                  # row-major: r ascending
    by = np.lexsort((j, d[r, j], r))                        # row, then value, then index
    r, j = r[by], j[by]
    return j[np.searchsorted(r, np.arange(m))[:, None] + np.arange(k)]


def near_f16_boundary(m):
    """float32 values -> True where the value is within relative NEAR of the midpoint of two neighbouring float16 values."""
    m = np.asarray(m, dtype=np.float32)
    with np.errstate(over="ignore"):
        h = m.astype(np.float16)
        up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    h, m = h.astype(np.float64), m.astype(np.float64)
    gap = np.minimum(np.abs(m - (h + up) / 2), np.abs(m - (h + dn) / 2))
    return gap <= NEAR * np.abs(m)


def kr_truth(qvecs, vecs, k1=20, k2=6, lambda_value=0.3, s_form="f32", block=6000, force_f16=False):
    """qvecs [D, Q], vecs [D, N] as the reference takes them -> namespace of every stage (module docstring).  force_f16 rounds
    V through float16 at k2 == 1 too: what the kernels did before they followed `if k2 != 1:`."""
    probe = np.asarray(qvecs.T, dtype=np.float32)           # torch.tensor(qvecs.T, dtype=torch.float32)
    gal = np.asarray(vecs.T, dtype=np.float32)
    nq = probe.shape[0]
    feat = np.concatenate([probe, gal])
    n_all = feat.shape[0]
    if s_form == "f32":
        def dots(a, b):
            return feat[a] @ feat[b].T
    elif s_form == "f64":
        feat64 = feat.astype(np.float64)

        def dots(a, b):
            return (feat64[a] @ feat64[b].T).astype(np.float32)
    else:
        dots = s_form                                        # callable (row slice, row slice) -> float32 block
    everything = slice(0, n_all)

    def euclid(a, b):
        return (2 - 2 * dots(a, b)).astype(np.float32)

    def normalised_block(cols):                              # [all, nj] / column max -> [nj, all]
        d = np.concatenate([euclid(slice(i, i + block), cols) for i in range(0, n_all // block * block + 1, block)
                            if i < n_all], axis=0)
        d = d / d.max(axis=0)
        return d.T

    initial_rank = np.concatenate(
        [stable_smallest(normalised_block(slice(j, j + block)), k1 + 1)
         for j in range(0, n_all // block * block + 1, block) if j < n_all], axis=0)

    def k_reciprocal_neigh(i, k):
        fwd = initial_rank[i, :k + 1]
        back = initial_rank[fwd, :k + 1]
        return fwd[np.where(back == i)[0]]

    khalf = int(np.around(k1 / 2))
    R = []
    for i in range(n_all):
        kr = k_reciprocal_neigh(i, k1)
        exp_idx = kr
        for c in kr:
            ckr = k_reciprocal_neigh(c, khalf)
            if len(np.intersect1d(ckr, kr)) > 2. / 3 * len(ckr):
                exp_idx = np.append(exp_idx, ckr)
        R.append(np.unique(exp_idx))

    V, dmax = [], np.empty(n_all, dtype=np.float32)
    for i in range(n_all):
        d = euclid(slice(i, i + 1), everything)
        dmax[i] = d.max()
        d = (d / d.max()).reshape(-1)[R[i]]
        w = np.exp(-d)
        V.append((w / w.sum()).astype(np.float32))

    rounded = k2 != 1 or force_f16
    qe_cols, qe_vals, qe_near = [], [], []
    for i in range(n_all):
        if k2 != 1:
            rows = initial_rank[i, :k2]
            cols = np.unique(np.concatenate([R[j] for j in rows]))
            m = np.zeros((k2, len(cols)), dtype=np.float32)
            for t, j in enumerate(rows):
                m[t, np.searchsorted(cols, R[j])] = V[j]
            m = np.mean(m, axis=0)                           # row after row in float32, then / k2
        else:
            cols, m = R[i], V[i]
        if rounded:
            h = m.astype(np.float16)
            keep = h != 0
            cols, near, m = cols[keep], near_f16_boundary(m[keep]), h[keep]
        else:
            near = np.zeros(len(cols), dtype=bool)
        qe_cols.append(cols)
        qe_vals.append(m)
        qe_near.append(near)

    # column -> (rows ascending, values): inv_index of :598-600 with the values beside it
    row_of = np.repeat(np.arange(n_all), [len(c) for c in qe_cols])
    col_of = np.concatenate(qe_cols)
    by_col = np.argsort(col_of, kind="stable")
    c_rows, c_vals, c_near = row_of[by_col], np.concatenate(qe_vals)[by_col], np.concatenate(qe_near)[by_col]
    ptr = np.searchsorted(col_of[by_col], np.arange(n_all + 1))

    jaccard = np.zeros((nq, n_all), dtype=np.float32)
    exposed = np.zeros((nq, n_all), dtype=bool)
    for i in range(nq):
        temp_min = np.zeros(n_all, dtype=np.float32)
        for c, v, nr in zip(qe_cols[i], qe_vals[i], qe_near[i]):
            seg = slice(ptr[c], ptr[c + 1])
            rows = c_rows[seg]
            temp_min[rows] = temp_min[rows] + np.minimum(v, c_vals[seg])
            exposed[i, rows] |= nr | c_near[seg]
        jaccard[i] = 1 - temp_min / (2. - temp_min)
    original = normalised_block(slice(0, nq))
    final = jaccard * (1 - lambda_value) + original * lambda_value
    final = final[:nq, nq:]
    return types.SimpleNamespace(
        S=dots(everything, everything) if n_all <= KEEP_S else None, initial_rank=initial_rank, R=R, V=V, dmax=dmax,
        Vqe_cols=qe_cols, Vqe_vals=qe_vals, final=final, order=np.argsort(final, axis=1, kind="stable"),
        exposed=exposed[:, nq:], lambda_value=lambda_value)


def check_result(t, got, dist):
    """The assertions every GPU case makes on (indices, distances) of kr_reranking_hip(..., return_dist=True) against truth t."""
    nq, n = t.final.shape
    assert got.shape == dist.shape == (nq, n) and got.dtype == np.int64 and dist.dtype == np.float32
    assert (np.sort(got, axis=1) == np.arange(n)).all(), "not a permutation"
    assert (np.diff(dist, axis=1) >= 0).all(), "distances do not ascend"
    final = t.final.astype(np.float64)
    bound = entry_bound(t.exposed, t.lambda_value)
    err = np.abs(np.take_along_axis(final, got, 1) - dist)
    b_got = np.take_along_axis(bound, got, 1)
    plain = ~np.take_along_axis(t.exposed, got, 1)
    print("max |truth - dist|: %.3g unexposed, %.3g exposed (%d of %d entries exposed)" % (
        err[plain].max() if plain.any() else 0.0, err[~plain].max() if (~plain).any() else 0.0, (~plain).sum(), plain.size))
    assert (err <= b_got).all(), "distance off by %.3g" % (err - b_got).max()
    # position by position: a different image only where the truth's own distances agree within the same bound
    gap = np.abs(np.take_along_axis(final, got, 1) - np.take_along_axis(final, t.order, 1))
    assert (gap <= np.maximum(b_got, np.take_along_axis(bound, t.order, 1))).all(), "order off by %.3g" % gap.max()


# ---- seeded inputs: the construction of test_kr_rerank_shapes_and_constants (tests/test_gpu_secondary_sweep.py)

def make_inputs(seed, n, d, nq, ncl=None, copies=0):
    """-> qvecs [D, Q], vecs [D, N] float32, unit columns.  copies > 0: that many exact copies of gallery image 3 in all (rows
    n // 2 ...), and query 0 equal to that image."""
    rng = np.random.default_rng(seed)
    ncl = ncl or max(4, n // 40)
    v = rng.standard_normal((n, d)) * 0.6 + 1.3 * rng.standard_normal((ncl, d))[np.arange(n) % ncl]
    if copies:
        v[n // 2:n // 2 + copies - 1] = v[3]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    q = v[rng.choice(n, nq, replace=False)] + 0.15 * rng.standard_normal((nq, d))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if copies:
        q[0] = v[3]
    return q.T.astype(np.float32), v.T.astype(np.float32)


# name -> (seed, n, d, nq, ncl, copies, k1, k2, lambda, s_form).  Behind every seed: the share of the case's [Q, N] entries that
# are exposed to a float16 rounding boundary, as test_exposed_share_of_every_gpu_case measures it (it must stay <= 1 %)
CASES = {
    # k2 == 1: V stays float32 (six cases on one input)
    "k2_1-k1_2-lam_0": (11, 200, 24, 6, 10, 0, 2, 1, 0.0, "f32"),        # seed 11: 0 (k2 == 1 rounds nothing)
    "k2_1-k1_2-lam_0.3": (11, 200, 24, 6, 10, 0, 2, 1, 0.3, "f32"),      # seed 11: 0
    "k2_1-k1_5-lam_0": (11, 200, 24, 6, 10, 0, 5, 1, 0.0, "f32"),        # seed 11: 0
    "k2_1-k1_5-lam_0.3": (11, 200, 24, 6, 10, 0, 5, 1, 0.3, "f32"),      # seed 11: 0
    "k2_1-k1_8-lam_0": (11, 200, 24, 6, 10, 0, 8, 1, 0.0, "f32"),        # seed 11: 0
    "k2_1-k1_8-lam_0.3": (11, 200, 24, 6, 10, 0, 8, 1, 0.3, "f32"),      # seed 11: 0
    "smallest": (21, 5, 16, 1, None, 0, 5, 3, 0.3, "f32"),               # seed 21: 0 of 5.  all == k1 + 1
    "below-one-chunk": (22, 40, 24, 1, None, 0, 5, 3, 0.3, "f32"),       # seed 22: 0 of 40
    "all_255": (23, 252, 16, 3, None, 0, 12, 3, 0.3, "f32"),             # seed 23: 0.40 % (3 of 756)
    "all_256": (24, 253, 16, 3, None, 0, 12, 3, 0.3, "f32"),             # seed 24: 0.66 % (5 of 759)
    "all_257": (25, 254, 16, 3, None, 0, 12, 3, 0.3, "f32"),             # seed 25: 0.13 % (1 of 762)
    "k2_is_k1+1": (26, 300, 24, 4, None, 0, 5, 6, 0.3, "f32"),           # seed 26: 0.08 % (1 of 1200)
    "n_700": (30, 700, 16, 5, None, 0, 20, 6, 0.3, "f32"),               # seed 30: 0.37 % (13 of 3500); seeds 27-29: 1.5-2.5 %
    "lam_0": (51, 400, 24, 4, None, 0, 20, 6, 0.0, "f32"),               # seed 51: 0.56 % (9 of 1600); seed 28: 1.0 %, 27: 3 %
    "lam_1": (51, 400, 24, 4, None, 0, 20, 6, 1.0, "f32"),               # seed 51: 0.56 % (the Jaccard term has weight 0)
    # 9 copies of one image + a query equal to it = 10 identical rows, k1 + 1 = 6: four of them miss their own neighbour list
    "duplicates": (29, 300, 16, 4, None, 9, 5, 3, 0.3, "f64"),           # seed 29: 0 of 1200
    "duplicates-k2_1": (29, 300, 16, 4, None, 9, 5, 1, 0.3, "f64"),      # seed 29: 0.  V_qe[i] is V[i], not V[initial_rank[i, 0]]
    "large-lds": (30, 16500, 16, 3, None, 0, 5, 3, 0.3, "f32"),          # seed 30: 0.002 % (1 of 49500).  all = 16503: 66012 bytes of LDS
}
K2_ONE = [name for name, c in CASES.items() if c[7] == 1 and not c[5]]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (qvecs, vecs, k1, k2, lambda, truth), computed once and shared (callers must not write into them)."""
    seed, n, d, nq, ncl, copies, k1, k2, lam, s_form = CASES[name]
    qv, vecs = make_inputs(seed, n, d, nq, ncl, copies)
    block = 6000 if n + nq <= 6000 else 2048                # column blocks only bound the memory of the large case
    return qv, vecs, k1, k2, lam, kr_truth(qv, vecs, k1, k2, lam, s_form, block)
