"""Exact kNN wrapper with the interface of the reference's faiss wrapper (src/utils/knn.py:8-40):

    KNN(database[N,D], 'cosine').search(queries[Q,D], k) -> (sims float32 [Q,k], ids int64 [Q,k])

`cosine` is faiss.IndexFlatIP there: exact top-k raw inner products, descending; rows are used as
given (the callers L2-normalise beforehand).  Here the index is a device-resident gallery
(NORM_NONE) and the search runs through the HIP path; ties go to the lower id.

    KNN(database[N,D], 'euclidean').search(queries[Q,D], k) -> (squared distances float32 [Q,k], ids int64 [Q,k])

`euclidean` is faiss.IndexFlatL2: exact top-k squared L2 distances of the rows as given, ascending -- the return of
IndexFlatL2.search -- through a squared-L2 gallery (Gallery.l2_from_host); ties go to the lower id.

    KNN(codes uint8 [N, nbits/8], 'hamming').search(qcodes uint8 [Q, nbits/8], k) -> (distances int32 [Q,k], ids int64 [Q,k])

`hamming` is faiss.IndexBinaryFlat: exact top-k Hamming distances of packed binary codes (_lib.pack_bits: bit j of a code is
bit j & 7 of byte j >> 3), ascending -- the return of IndexBinaryFlat.search -- through a binary index (_lib.BinaryGallery);
ties go to the lower id.  Removal, radius search, save / load and sharding are not built for binary indexes.

    KNN(database[N,D], 'l1' | 'linf').search(queries[Q,D], k)    KNN(database[N,D], 'lp', p=0.5).search(queries[Q,D], k)
        -> (distances float32 [Q,k] ascending, ids int64 [Q,k])

`l1`, `linf` and `lp` are faiss.IndexFlat(D, METRIC_L1 | METRIC_Linf | METRIC_Lp) (metric_arg = p): sum |q - x|, max |q - x| and
sum |q - x| ** p -- faiss's value, not raised to 1 / p -- of the rows as given, in float64 over a NORM_NONE gallery
(Gallery.search_minkowski); ties go to the lower id.  remove_ids works; range_search is not defined for them, radius_search is:

    KNN(database[N,D], 'euclidean' | 'l1' | 'linf' | 'lp').radius_search(queries[Q,D], radius)
        -> (lims int64 [Q+1], D float32 [lims[-1]] ascending per query, I int64 [lims[-1]])

every row whose value in the index's own metric is <= radius (inclusive; Gallery.range_search_minkowski): squared L2 for
'euclidean', faiss's un-rooted sum for 'lp'.

    ANN(database[N,D], 'euclidean', M=64, nbits=8, nlist=256, nprobe=64).search(queries[Q,D], k)
        -> (squared ADC distances float32 [Q,k] ascending, ids int64 [Q,k])

the counterpart of the reference's approximate wrapper (src/utils/knn.py:43-53, faiss.IndexIVFPQ with its defaults, so
by_residual = true) on a residual _lib.IVFPQIndex.
"""
import numpy as np

from ._lib import (BinaryGallery, Gallery, IVFPQIndex, IVF_MAX_LISTS, MINK_METRICS, NORM_NONE, PQ_MAX_BOOKS, minkowski_args,
                   minkowski_range_args)


class KNN:
    method = "cosine"

    def __init__(self, database, method="cosine", device=0, p=None):
        if method not in ("cosine", "euclidean", "hamming") and method not in MINK_METRICS:
            raise NotImplementedError("method must be 'cosine' (IndexFlatIP), 'euclidean' (IndexFlatL2), 'hamming' "
                                      "(IndexBinaryFlat) or 'l1', 'linf', 'lp' (IndexFlat with a Minkowski metric), got %r"
                                      % (method,))
        self.method, self.p = method, p
        if method in MINK_METRICS:
            minkowski_args(method, p, 1)          # a bad p raises here, before a device is touched
        database = np.asarray(database)
        if method == "hamming":
            if database.dtype != np.uint8 or database.ndim != 2:
                raise ValueError("'hamming' takes packed codes uint8 [N, nbits / 8] (_lib.pack_bits)")
            self.N, self.D = database.shape[0], database.shape[1] * 8
            self.gallery = BinaryGallery.from_host(database, device=device)
            return
        if database.dtype != np.float32:          # src/utils/knn.py:10-11
            database = database.astype(np.float32)
        self.N, self.D = database.shape
        if method == "euclidean":
            self.gallery = Gallery.l2_from_host(database, device=device)
        else:
            self.gallery = Gallery.from_host(database, norm_mode=NORM_NONE, device=device)

    def search(self, queries, k, allow=None):
        """-> (sims float32 [Q,k], ids int64 [Q,k]).  allow (optional, like faiss's ID selector in the search parameters):
        restrict the search to some rows -- a bool mask [N], an array of allowed ids, or packed AllowBits words (_lib.allow_bitmap;
        _lib.allow_ranges for row ranges).  Fewer than k allowed rows: trailing ids -1, sims -inf.
        'euclidean': -> (squared distances float32 [Q,k] ascending, ids int64 [Q,k]); fewer than k rows: ids -1, distances +inf."""
        if self.method == "hamming":              # -> (distances int32 [Q,k] ascending, ids int64 [Q,k]); short: -1 / INT32_MAX
            ids, dist, _ = self.gallery.search(np.asarray(queries), int(k), allow)
            return dist, ids
        queries = np.asarray(queries)
        if queries.dtype != np.float32:           # src/utils/knn.py:28-29
            queries = queries.astype(np.float32)
        if self.method == "euclidean":
            ids, dist, _, _, _ = self.gallery.search_l2(queries, int(k), allow)
            return dist, ids
        if self.method in MINK_METRICS:           # -> (distances float32 [Q,k] ascending, ids int64 [Q,k]); short: -1 / +inf
            ids, dist, _, _ = self.gallery.search_minkowski(queries, int(k), self.method, self.p, allow)
            return dist, ids
        if allow is not None:
            ids, sims, _, _ = self.gallery.search_filtered(queries, int(k), allow)
            return sims, ids
        ids, sims, _ = self.gallery.search(queries, int(k))
        return sims, ids

    def set_groups(self, labels):
        """One integer label per database row ('cosine' only): rows of one label are one item for search_grouped; -1 makes a row
        an item of its own, None clears the labels.  remove_ids drops them."""
        if self.method != "cosine":
            raise NotImplementedError("groups are defined for 'cosine' only")
        self.gallery.set_groups(labels)

    def search_grouped(self, queries, k, exclude=None):
        """-> (sims float32 [Q,k], ids int64 [Q,k]) like search, but at most one row per group -- the group's best --, k groups
        per query (the collapse / group-by search of other engines).  exclude: None, one label or one per query, whose rows are
        skipped.  Fewer than k groups: trailing ids -1, sims -inf.  'cosine' only."""
        if self.method != "cosine":
            raise NotImplementedError("search_grouped is defined for 'cosine' only")
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            queries = queries.astype(np.float32)
        ids, sims, _ = self.gallery.search_grouped(queries, int(k), exclude)
        return sims, ids

    def range_search(self, queries, thresh):
        """-> (lims int64 [Q+1], D float32 [lims[-1]], I int64 [lims[-1]]), the return shape of faiss's `range_search`: the
        results of query i are D/I[lims[i]:lims[i+1]].  Every row whose exact inner product with the query is >= thresh
        (the bound is INCLUSIVE), ordered by (score desc, id asc).  'cosine' only."""
        if self.method != "cosine":
            raise NotImplementedError("range_search is defined for 'cosine' only (a radius search in L2 is not built)")
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            queries = queries.astype(np.float32)
        lims, ids, sims, _ = self.gallery.range_search(queries, float(thresh))
        return lims, sims, ids

    def radius_search(self, queries, radius):
        """-> (lims int64 [Q+1], D float32 [lims[-1]], I int64 [lims[-1]]), the return shape of range_search: every row whose
        distance to the query in the index's own metric is <= radius (the bound is INCLUSIVE), ordered by (distance asc, id asc).
        'euclidean': squared L2 distances, the values search returns (faiss IndexFlatL2.range_search), so a Euclidean radius r is
        passed as r * r; 'l1', 'linf', 'lp': the values search returns ('lp': sum |q - x| ** p, not raised to 1 / p).  'cosine'
        and 'hamming' have range_search."""
        if self.method in ("cosine", "hamming"):
            raise NotImplementedError("radius_search is defined for 'euclidean', 'l1', 'linf' and 'lp'; %r has range_search"
                                      % (self.method,))
        metric, p = ("lp", 2.0) if self.method == "euclidean" else (self.method, self.p)
        minkowski_range_args(metric, p, radius)   # a bad radius raises here, before the queries are touched
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            queries = queries.astype(np.float32)
        lims, ids, dist, _, _ = self.gallery.range_search_minkowski(queries, float(radius), metric, p)
        return lims, dist, ids

    def remove_ids(self, ids):
        """faiss's IndexFlat.remove_ids, every float metric: the rows leave the index, the others keep their order and are renumbered
        0 .. N' - 1.  ids: an array of row ids (duplicates are fine), a bool mask [N] or packed AllowBits words.  -> the number
        of rows removed."""
        if self.method == "hamming":
            raise NotImplementedError("remove_ids is not built for binary indexes")
        before = self.gallery.n
        self.gallery.remove(ids)
        self.N = self.gallery.n
        return before - self.N

    def close(self):
        self.gallery.close()


def _unit_rows(a):
    a = np.asarray(a, dtype=np.float32)
    norm = np.sqrt((a.astype(np.float64) ** 2).sum(1, keepdims=True))
    return (a / np.maximum(norm, np.finfo(np.float64).tiny)).astype(np.float32)


class ANN:
    """The reference's ANN (src/utils/knn.py:43-53: faiss.IndexIVFPQ(quantizer, D, nlist, M, nbits), trained on a fifth of the
    rows, nprobe set after the add) on a residual IVFPQIndex.

    LIMITS: the index takes M <= 64 books, nlist <= 256 lists and nbits == 8 only; anything else raises ValueError.  The
    reference's own defaults, M = 128 and nlist = 316, lie OUTSIDE these limits, which is why the defaults here are M = 64 and
    nlist = 256.  D must be a multiple of M and N // 5 >= max(256, nlist).

    It trains on the N // 5 rows RandomState(seed).permutation(N)[:N // 5] (IVFPQIndex.train(by_residual=True) with `seed`), then
    adds all rows.  The clusters and codebooks are this library's deterministic k-means, NOT faiss's, on purpose: nothing pins them
    to faiss.  What is exact is the search given them: the residual contract of the index, top-k by (distance asc, id asc).
    'cosine' L2-normalises the database and the queries first, so that the squared distance orders like the inner product; the
    values returned are still squared distances, ascending.  Diffusion does not use this class: the exact search is faster
    there."""

    def __init__(self, database, method="euclidean", M=64, nbits=8, nlist=256, nprobe=64, seed=0, device=0, refine_k_factor=0):
        if method not in ("cosine", "euclidean"):
            raise NotImplementedError("method must be 'cosine' or 'euclidean', got %r" % (method,))
        M, nbits, nlist, nprobe = int(M), int(nbits), int(nlist), int(nprobe)
        self.refine_k_factor = int(refine_k_factor)
        if self.refine_k_factor < 0:
            raise ValueError("refine_k_factor = %d: 0 = no refinement, f >= 1 = re-rank k * f ids" % self.refine_k_factor)
        self.rows = None
        if not 1 <= M <= PQ_MAX_BOOKS:
            raise ValueError("M = %d books, the IVF-PQ index takes 1 .. %d (the reference's default of 128 is outside)" % (M, PQ_MAX_BOOKS))
        if nbits != 8:
            raise ValueError("nbits = %d, the IVF-PQ index takes nbits = 8 only (one byte per book)" % nbits)
        if not 2 <= nlist <= IVF_MAX_LISTS:
            raise ValueError("nlist = %d lists, the IVF-PQ index takes 2 .. %d (the reference's default of 316 is outside)"
                             % (nlist, IVF_MAX_LISTS))
        if not 1 <= nprobe <= nlist:
            raise ValueError("nprobe = %d, the index has nlist = %d lists (1 .. nlist)" % (nprobe, nlist))
        database = np.asarray(database)
        if database.ndim != 2:
            raise ValueError("database must be [N, D]")
        if database.dtype != np.float32:          # src/utils/knn.py:10-11
            database = database.astype(np.float32)
        self.method, self.nprobe = method, nprobe
        self.N, self.D = database.shape
        if self.D % M:
            raise ValueError("D = %d is no multiple of M = %d" % (self.D, M))
        if self.N // 5 < max(1 << nbits, nlist):
            raise ValueError("N // 5 = %d training rows, %d codewords and %d lists need at least as many" % (self.N // 5, 1 << nbits, nlist))
        if method == "cosine":
            database = _unit_rows(database)
        samples = database[np.random.RandomState(seed).permutation(self.N)[:self.N // 5]]
        g, cb, _, _ = IVFPQIndex.train(samples, nlist, M, 1 << nbits, seed=seed, device=device, by_residual=True)
        self.index = IVFPQIndex.empty(g, cb, self.N, device=device, by_residual=True)
        self.index.add(database)
        if self.refine_k_factor > 0:
            # faiss IndexRefineFlat over the IVF-PQ index: the rows themselves (unit rows for 'cosine') beside the codes
            self.rows = Gallery.l2_from_host(database, device=device)

    def search(self, queries, k):
        """-> (squared distances float32 [Q,k] ascending, ids int64 [Q,k]); fewer than k rows in the probed lists: ids -1,
        distances +inf.  With refine_k_factor = f > 0 the index returns min(k * f, N, 8192) ids per query and the k best of them
        by their EXACT squared distance to the stored rows come back, with those distances (Gallery.refine)."""
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            queries = queries.astype(np.float32)
        if self.method == "cosine":
            queries = _unit_rows(queries)
        if getattr(self, "rows", None) is not None:
            ids, dist, _ = self.index.search(queries, int(k), nprobe=self.nprobe, refine=self.rows, k_factor=self.refine_k_factor)
            return dist, ids
        ids, dist, _ = self.index.search(queries, int(k), nprobe=self.nprobe)
        return dist, ids

    def remove_ids(self, ids):
        """faiss's IndexIVFPQ.remove_ids: the rows leave the index, the others keep their order, codes and lists and are renumbered
        0 .. N' - 1.  ids: an array of row ids (duplicates are fine), a bool mask [N] or packed AllowBits words.  -> the number of
        rows removed."""
        before = self.index.n
        if getattr(self, "rows", None) is not None:
            from ._lib import allow_bitmap
            ids = allow_bitmap(ids, self.index.n, 0)             # one bitmap for both: the index and the rows stay aligned
            self.rows.remove(ids)
        self.index.remove(ids)
        self.N = self.index.n
        return before - self.N

    def close(self):
        self.index.close()
        if getattr(self, "rows", None) is not None:
            self.rows.close()
            self.rows = None
