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
"""
import numpy as np

from ._lib import BinaryGallery, Gallery, NORM_NONE


class KNN:
    method = "cosine"

    def __init__(self, database, method="cosine", device=0):
        if method not in ("cosine", "euclidean", "hamming"):
            raise NotImplementedError("method must be 'cosine' (IndexFlatIP), 'euclidean' (IndexFlatL2) or 'hamming' "
                                      "(IndexBinaryFlat), got %r" % (method,))
        self.method = method
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
        if allow is not None:
            ids, sims, _, _ = self.gallery.search_filtered(queries, int(k), allow)
            return sims, ids
        ids, sims, _ = self.gallery.search(queries, int(k))
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

    def remove_ids(self, ids):
        """faiss's IndexFlat.remove_ids, both float metrics: the rows leave the index, the others keep their order and are renumbered
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
