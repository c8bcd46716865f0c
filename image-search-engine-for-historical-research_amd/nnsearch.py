"""Host-side mirror of the reference's matcher surface (src/utils/nnsearch.py) for the HIP path.

    matching_HIP(K, embedded_features_train[N,D], embedded_features_test[Q,D], dataset=None,
                 ifgenerate=False) -> (idx int64 [Q,K], time_per_query seconds)

follows the convention of the reference's matchers: stateless ones are called as
`matching_L2(K, train, test)` (src/utils/nnsearch.py:687), stateful ones take `dataset` /
`ifgenerate`, persist under `outputs/<dataset>/` and rebuild iff `ifgenerate`
(src/utils/nnsearch.py:503-525, 1033-1044).  Callers pass `vecs.T` / `qvecs.T` and use
`match_idx.T` as ranks[K,Q] (src/offline.py:107-118, src/online.py:132-147).

Results: the exact top-K by cosine similarity of the L2-normalised rows -- the ordering
matching_L2 computes via ||q - g|| -- with ties to the lower index.  All arithmetic runs in the
HIP library; there is no CPU path.
"""
import os
import threading
import time
import uuid

import numpy as np

from . import _lib
from ._lib import Gallery, NORM_L2, NORM_NONE, NORM_L2_EPS  # noqa: F401

TOPK_PATH_MAX_K = 2048      # beyond this the full-length ranking path is used

_cache = {}
_cache_lock = threading.Lock()
_savers = {}                # cache key -> thread writing that gallery's file behind the call that built it
_state_lock = threading.Lock()   # _savers, _path_locks, last_timing["save"] (written by saver threads)
_path_locks = {}            # gallery file -> lock: one writer per file at a time
last_timing = {}            # what the last get_gallery() did: {"source": built | cached | file, "build_s", "save": ...}


def _gallery_path(dataset, norm_mode=NORM_L2):
    # one file per normalisation: matching_HIP (L2-normalised rows) and the QGE / inner-product callers (rows as given)
    # prepare different galleries of the same dataset
    suffix = {NORM_L2: "l2", NORM_NONE: "raw", NORM_L2_EPS: "l2eps"}[norm_mode]
    return os.path.join("outputs", dataset.replace("/", "_"), "mi355_gallery_%s.bin" % suffix)


def _save_behind(key, g, path):
    """The prepared-gallery file (12 GB at the 1M-row size: ~1.2 s of D2H + page-cache writes) is written by a thread of its
    own AFTER the gallery is usable: the caller's timer (matching_<method> times everything it does, src/utils/nnsearch.py:688-705)
    no longer spans it.  mi_gallery_save reads the handle's immutable buffers (checksums and copies on streams of its own) and
    takes the handle's mutex for the one mutable thing it stores, the XCD shares of the search workspace; searches run beside
    it.  Written to a temporary name of its own and renamed: a reader never sees half a file."""
    def work():
        # one temporary name per writer (two galleries of one dataset on two devices share `path`), one writer per path at a time
        tmp = "%s.tmp.%d.%s" % (path, os.getpid(), uuid.uuid4().hex[:12])
        t0 = time.time()
        with _path_lock(path):
            try:
                g.save(tmp)
                os.replace(tmp, path)
                rec = {"seconds": time.time() - t0, "path": path, "behind_the_call": True}
            except Exception as e:        # the file is a cache: failing to write it must not fail a search that succeeded
                rec = {"error": "%s: %s" % (type(e).__name__, e)}
                try:
                    os.unlink(tmp)
                except OSError:
                    pass
        with _state_lock:
            last_timing["save"] = rec
    th = threading.Thread(target=work, name="mi355-gallery-save", daemon=False)
    with _state_lock:
        _savers[key] = th
    th.start()


def _path_lock(path):
    with _state_lock:
        return _path_locks.setdefault(os.path.abspath(path), threading.Lock())


def wait_for_saves():
    """Blocks until every write-behind gallery file is complete (a process that exits joins them anyway)."""
    with _state_lock:
        ths = list(_savers.values())
        _savers.clear()
    for th in ths:
        th.join()


def _join_saver(key):
    with _state_lock:
        th = _savers.pop(key, None)
    if th is not None:
        th.join()


def get_gallery(train, dataset=None, ifgenerate=False, norm_mode=NORM_L2, device=0):
    """Device-resident prepared gallery for `train` [N,D].

    dataset=None: a fresh (uncached) gallery.  Otherwise the gallery is cached in-process under
    `dataset`, persisted to outputs/<dataset>/mi355_gallery_<norm>.bin (written behind the call, _save_behind), and rebuilt
    iff `ifgenerate` (or when its shape no longer matches `train`, which the reference leaves to the user:
    README "delete the cache when the database changes").  The cache and the file are keyed by `dataset`, not by content: a
    caller who takes rows out of the returned gallery (Gallery.remove) saves it again (Gallery.save over the file) or passes
    `ifgenerate` with the reduced `train` the next time -- otherwise the next process loads the rows that were removed."""
    last_timing.clear()
    if dataset is None:
        t0 = time.time()
        g = _build_gallery(train, norm_mode, device)
        last_timing.update(source="built", build_s=time.time() - t0)
        return g
    key = (dataset, norm_mode, device)
    with _cache_lock:
        g = _cache.get(key)
        shape = _train_shape(train)
        if g is not None and not ifgenerate and (g.n, g.d) == shape:
            last_timing.update(source="cached")
            return g
        _join_saver(key)                  # the handle about to be closed / the file about to be replaced may still be written
        if g is not None:
            g.close()
            _cache.pop(key, None)
        path = _gallery_path(dataset, norm_mode)
        t0 = time.time()
        if not ifgenerate and os.path.exists(path):
            try:
                g = Gallery.load(path, device=device)
            except RuntimeError as e:
                # a file that does not load -- truncated, a checksum that does not match, an older layout -- is a cache miss:
                # the gallery is rebuilt from `train` and the file replaced (MI_ERR_IO = 4; anything else is a real failure)
                if "error 4" not in str(e):
                    raise
                last_timing.update(file_rejected=str(e))
                g = None
            if g is None:
                pass
            elif (g.n, g.d) != shape or g.norm_mode != norm_mode:
                g.close()
                g = None
            else:
                last_timing.update(source="file", load_s=time.time() - t0)
        else:
            g = None
        if g is None:
            t0 = time.time()
            g = _build_gallery(train, norm_mode, device)
            last_timing.update(source="built", build_s=time.time() - t0)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            _save_behind(key, g, path)
        _cache[key] = g
        return g


class ColumnBlocks:
    """`train` given as the blocks the reference concatenates on the host -- ColumnBlocks([vecs, vecs_1m]) stands for
    np.concatenate([vecs, vecs_1m], axis=1).T (src/test_rOP1m.py:136-139, 155-156) -- ingested block by block."""

    def __init__(self, blocks):
        self.blocks = list(blocks)
        self.shape = (sum(b.shape[1] for b in self.blocks), self.blocks[0].shape[0])


def _train_shape(train):
    return tuple(train.shape) if isinstance(train, ColumnBlocks) else tuple(np.shape(train))


def _build_gallery(train, norm_mode, device):
    if isinstance(train, ColumnBlocks):
        return Gallery.from_blocks(train.blocks, norm_mode=norm_mode, device=device)
    return Gallery.from_host(train, norm_mode=norm_mode, device=device)


def drop_cached_galleries():
    """Closes every cached gallery and gives the library's spare-buffer slots back too (mi_set_global_option "release_spares":
    up to 16 GiB + ~200 MB that would otherwise stay with the process for the next gallery of the same sizes).  A gallery an
    online chain is still built on (entry.online.Searcher: close() it first) is refused by the library and stays cached."""
    with _cache_lock:
        wait_for_saves()
        for key in list(_cache):
            try:
                _cache[key].close()
            except RuntimeError as e:
                if "online handle" not in str(e):
                    raise
                continue
            del _cache[key]
        _lib.set_global_option("release_spares", 1)


def matching_HIP(K, embedded_features_train, embedded_features_test, dataset=None, ifgenerate=False,
                 device=0, return_scores=False, devices=None):
    """Drop-in `--matching_method HIP`.  The timer spans everything the call does (for a stateless
    call that includes the gallery ingest, like matching_L2's timer includes its normalisation,
    src/utils/nnsearch.py:688-705), device-synchronised.
    devices: a list of GPU ids -> the gallery rows are split over them inside THIS process
    (sharded.MultiDeviceGallery: the reference's drivers are single processes); K <= 2048, stateless."""
    t1 = time.time()
    num_test = np.shape(embedded_features_test)[0]
    if devices is not None and len(devices) > 1:
        from .sharded import MultiDeviceGallery
        if int(K) > TOPK_PATH_MAX_K or isinstance(embedded_features_train, ColumnBlocks):
            raise ValueError("devices=[...]: top-K path only (K <= %d), one host array" % TOPK_PATH_MAX_K)
        mg = MultiDeviceGallery.from_host(np.asarray(embedded_features_train), devices, NORM_L2, k_max=int(K))
        try:
            idx, scores = mg.search(embedded_features_test, int(K))
        finally:
            mg.close()
        tpq = (time.time() - t1) / num_test
        return (idx, tpq, scores) if return_scores else (idx, tpq)
    g = get_gallery(embedded_features_train, dataset, ifgenerate, NORM_L2, device)
    try:
        if int(K) > TOPK_PATH_MAX_K:
            # deep / full-length ranking (--mode mAP ranks the whole database, src/test_rOP1m.py:144-149): dense exact
            # scores + per-query radix sort on the device; only the first K columns come back to the host
            if int(K) > g.n:
                raise RuntimeError("mi355_retrieval error 1: k > number of gallery rows")
            idx, scores, _ = g.rank_prefix(embedded_features_test, int(K), return_scores=True)
        else:
            idx, scores, _ = g.search(embedded_features_test, int(K))
    finally:
        if dataset is None:
            g.close()
    t2 = time.time()
    time_per_query = (t2 - t1) / num_test
    if return_scores:
        return idx, time_per_query, scores
    return idx, time_per_query


def matching_L2_hip(K, embedded_features_train, embedded_features_test):
    """Same signature as matching_L2 (src/utils/nnsearch.py:687)."""
    return matching_HIP(K, embedded_features_train, embedded_features_test)


def matching_Greedyhash_hip(K, hash_codes_train, hash_codes_test):
    """Same signature and return shape as matching_Greedyhash (src/utils/nnsearch.py:1001-1013): exact Hamming top-K of 0/1 hash
    codes [N, code_len] / [Q, code_len] (any integer or bool dtype) -> (idx int64 [Q, K], time_per_query).  The reference
    sorts `(query ^ train).sum(axis=1)` with an unstable argsort; here rows at equal distance come by ascending index.
    code_len is padded to a multiple of 8 with zero columns on both sides, which changes no distance.  K > N raises, as the
    reference's `idx[row, :] = ...` assignment does.  The timer spans what the reference's spans: everything the call does
    (packing, index build and search), device-synchronised."""
    t1 = time.time()
    train, test = np.asarray(hash_codes_train), np.asarray(hash_codes_test)
    if train.ndim != 2 or test.ndim != 2 or train.shape[1] != test.shape[1]:
        raise ValueError("expected hash codes [N, code_len] and [Q, code_len], got %s and %s" % (train.shape, test.shape))
    for name, a in (("hash_codes_train", train), ("hash_codes_test", test)):
        if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("%s: binary codes must be an integer or bool array of 0 / 1 values (got %s)" % (name, a.dtype))
    K = int(K)
    num_train, num_test = train.shape[0], test.shape[0]
    if K > num_train or K < 1:
        raise ValueError("K = %d, the database holds %d codes" % (K, num_train))
    if K > TOPK_PATH_MAX_K:
        raise ValueError("K <= %d" % TOPK_PATH_MAX_K)
    g = _lib.BinaryGallery.from_host(_lib.pack_bits(train))        # (pack_bits raises ValueError on anything but 0 / 1)
    try:
        idx, _, _ = g.search(_lib.pack_bits(test), K)
    finally:
        g.close()
    return idx, (time.time() - t1) / num_test


def matching_LSH_hip(K, embedded_features_train, embedded_features_test, n_bits, seed=5, refine_rows=None, k_factor=10):
    """Same signature and return shape as matching_LSH_faiss (src/utils/nnsearch.py:734-745), plus the seed faiss fixes at 5:
    faiss.IndexLSH(feature_len, n_bits) over the database rows, searched with the queries -> (idx int64 [Q, K],
    time_per_query).  A row's code is bit j = (x . R[j] >= 0), the sums in float64, R = _lib.lsh_rotation(dim, n_bits, seed) --
    faiss's construction of the random rotation, not faiss's random stream, so the codes differ from faiss's the way two seeds
    differ; the answer given the codes is the exact Hamming top-K, rows at equal distance by ascending index.  The rows are used
    as given (faiss does not normalise here).  n_bits a multiple of 8 in [8, 4096], dim <= 4096, 1 <= K <= min(N, 2048); bad
    input raises ValueError before the device is touched.  No reference entry point dispatches to LSH, so it is not in
    MATCHING_METHODS.  The timer spans what the reference's spans: the search only -- upload and encoding of the queries
    included --, device-synchronised; the index build lies before it.
    refine_rows: the raw features [N, D] (usually embedded_features_train itself) -> faiss IndexRefineFlat on top: the Hamming
    search hands min(K * k_factor, N, 8192) ids to an exact squared-L2 re-ranking against those rows on the device
    (_lib.Gallery.refine), and the K best of them come back."""
    train, test = np.asarray(embedded_features_train), np.asarray(embedded_features_test)
    if train.ndim != 2 or test.ndim != 2 or train.shape[1] != test.shape[1]:
        raise ValueError("expected rows [N, dim] and queries [Q, dim], got %s and %s" % (train.shape, test.shape))
    for name, a in (("embedded_features_train", train), ("embedded_features_test", test)):
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError("%s must be a floating-point array (got %s)" % (name, a.dtype))
    K = int(K)
    dim, n_bits = _lib._lsh_shape(train.shape[1], n_bits)        # (raises ValueError on n_bits or dim outside the limits)
    num_train, num_test = train.shape[0], test.shape[0]
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d rows" % (K, num_train))
    if K > TOPK_PATH_MAX_K:
        raise ValueError("K <= %d" % TOPK_PATH_MAX_K)
    rows = _refine_gallery(refine_rows, num_train, dim)
    try:
        with _lib.LSHIndex.from_host(train, R=_lib.lsh_rotation(dim, n_bits, seed)) as g:
            t1 = time.time()
            if rows is None:
                idx, _, _ = g.search(test, K)              # (synchronous: the results are on the host when it returns)
            else:
                idx, _, _ = g.search(test, K, refine=rows, k_factor=k_factor)
            t2 = time.time()
    finally:
        if rows is not None:
            rows.close()
    return idx, (t2 - t1) / max(num_test, 1)


def _refine_gallery(refine_rows, n, dim):
    """The squared-L2 gallery of the raw features a matcher re-ranks its shortlist on, or None."""
    if refine_rows is None:
        return None
    r = np.asarray(refine_rows)
    if r.ndim != 2 or r.shape != (n, dim) or not np.issubdtype(r.dtype, np.floating):
        raise ValueError("refine_rows must be the raw floating-point features [N = %d, D = %d] (got %s %s)" % (n, dim, r.dtype, r.shape))
    return _lib.Gallery.l2_from_host(r)


def matching_PQ_Net_hip(K, Codewords, Query, N_books, CW_idx):
    """Same signature and return shape as matching_PQ_Net (src/utils/nnsearch.py:905-946): asymmetric-distance top-K of queries
    [Q, dim] against N_books-byte PQ codes CW_idx [N, N_books] under Codewords [N_words, dim] (book j is the column block
    j * L .. (j + 1) * L, L = dim / N_books) -> (idx int64 [Q, K], time_per_query).  The reference sorts float32 sums of a
    float32 table with an unstable argsort; here a table entry is the float64 sum of squares rounded once to float32, a
    distance is the float32 sum of a row's entries in book order, and rows at equal distance come by ascending index
    (include/mi355_retrieval.h, PQ index).  N_words <= 256 (one byte per book), dim % N_books == 0, 1 <= K <= min(N, 2048);
    CW_idx must be an integer array with values in [0, N_words).  Bad input raises ValueError before the device is touched.  It
    is no (K, train, test) matcher and therefore not in MATCHING_METHODS.  The timer spans what the reference's spans:
    everything the call does (index build, tables and search), device-synchronised."""
    t1 = time.time()
    cw, q, codes = np.asarray(Codewords), np.asarray(Query), np.asarray(CW_idx)
    if cw.ndim != 2 or q.ndim != 2 or codes.ndim != 2 or q.shape[1] != cw.shape[1]:
        raise ValueError("expected Codewords [N_words, dim], Query [Q, dim] and CW_idx [N, N_books], got %s, %s and %s"
                         % (cw.shape, q.shape, codes.shape))
    N_books, K = int(N_books), int(K)
    n_words, dim = cw.shape
    if N_books < 1 or dim % N_books:
        raise ValueError("dim = %d is no multiple of N_books = %d" % (dim, N_books))
    if codes.shape[1] != N_books:
        raise ValueError("CW_idx has %d columns, N_books = %d" % (codes.shape[1], N_books))
    if n_words > _lib.PQ_MAX_WORDS:
        raise ValueError("N_words = %d, a code byte holds at most %d codewords per book" % (n_words, _lib.PQ_MAX_WORDS))
    num_train, num_test = codes.shape[0], q.shape[0]
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d codes" % (K, num_train))
    if K > TOPK_PATH_MAX_K:
        raise ValueError("K <= %d" % TOPK_PATH_MAX_K)
    if not (np.issubdtype(q.dtype, np.floating) and np.isfinite(q).all()):
        raise ValueError("Query must be a finite floating-point array")
    # [N_words, N_books * L] -> [N_books, N_words, L]
    books = cw.reshape(n_words, N_books, dim // N_books).transpose(1, 0, 2)
    with _lib.PQIndex.from_codes(books, codes) as g:              # (raises ValueError on non-integer or out-of-range codes)
        idx, _, _ = g.search(q, K)
    return idx, (time.time() - t1) / max(num_test, 1)


def matching_PQ_Net_bucket_hip(K, Codewords, Query, N_books, CW_idx, Gallery_features, n_clusters=10, nprobe=1, refine_rows=None,
                               k_factor=10):
    """Same signature and return shape as matching_PQ_Net_bucket (src/utils/nnsearch.py:949-998), plus n_clusters (the reference
    fixes 10) and nprobe (the reference's 1): k-means buckets over Gallery_features [N, dim]; a query is answered by the ADC top-K
    of matching_PQ_Net_hip over the rows of the nprobe buckets nearest to it -> (idx int64 [Q, K], time_per_query).  Both of the
    reference's TODOs are closed by construction: a query whose buckets hold fewer than K rows gets trailing ids -1, and nprobe
    selects several buckets.
    The CLUSTERS differ from the reference's, on purpose and unpinned: the reference runs sklearn's KMeans(n_clusters,
    random_state=0) -- k-means++ seeding from sklearn's random stream, float32 / Elkan arithmetic, several restarts -- while the
    coarse centroids here are _lib.pq_train(Gallery_features, 1, n_clusters, seed=0): Lloyd's iteration from rows drawn by
    RandomState(0), float64 assignment.  Which local optimum k-means reaches is a matter of initialisation, and no answer below
    depends on it being sklearn's.  What IS exact is the search given the buckets: a row's bucket is the float64 argmin over the
    centroids (ties to the lower bucket: the 1-book encode), a query's buckets are the nprobe smallest by (float64 distance, id),
    and the answer is the top-K by (distance asc, id asc) of matching_PQ_Net_hip's distances over those rows
    (include/mi355_retrieval.h, IVF index over PQ codes).  Limits as for matching_PQ_Net_hip, 2 <= n_clusters <= 256 and
    N >= n_clusters; bad input raises ValueError before the device is touched.  It is no (K, train, test) matcher and therefore
    not in MATCHING_METHODS.  The timer spans what the reference's spans: the bucket of every query, tables and search,
    device-synchronised; clustering and index build lie before it, as the reference's KMeans.fit does.
    refine_rows: the raw features [N, dim] -> faiss IndexRefineFlat on top: the search hands min(K * k_factor, N, 8192) ids to an
    exact squared-L2 re-ranking against those rows on the device (_lib.Gallery.refine), and the K best of them come back."""
    cw, q, codes, gal = np.asarray(Codewords), np.asarray(Query), np.asarray(CW_idx), np.asarray(Gallery_features)
    if cw.ndim != 2 or q.ndim != 2 or codes.ndim != 2 or gal.ndim != 2 or q.shape[1] != cw.shape[1] or gal.shape[1] != cw.shape[1]:
        raise ValueError("expected Codewords [N_words, dim], Query [Q, dim], CW_idx [N, N_books] and Gallery_features [N, dim], got "
                         "%s, %s, %s and %s" % (cw.shape, q.shape, codes.shape, gal.shape))
    N_books, K, n_clusters, nprobe = int(N_books), int(K), int(n_clusters), int(nprobe)
    n_words, dim = cw.shape
    if N_books < 1 or dim % N_books:
        raise ValueError("dim = %d is no multiple of N_books = %d" % (dim, N_books))
    if codes.shape[1] != N_books:
        raise ValueError("CW_idx has %d columns, N_books = %d" % (codes.shape[1], N_books))
    if n_words > _lib.PQ_MAX_WORDS:
        raise ValueError("N_words = %d, a code byte holds at most %d codewords per book" % (n_words, _lib.PQ_MAX_WORDS))
    num_train, num_test = codes.shape[0], q.shape[0]
    if gal.shape[0] != num_train:
        raise ValueError("Gallery_features has %d rows, CW_idx %d" % (gal.shape[0], num_train))
    if not 2 <= n_clusters <= _lib.IVF_MAX_LISTS:
        raise ValueError("n_clusters = %d, a list id is one byte (2 .. %d)" % (n_clusters, _lib.IVF_MAX_LISTS))
    if not 1 <= nprobe <= n_clusters:
        raise ValueError("nprobe = %d of n_clusters = %d" % (nprobe, n_clusters))
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d codes" % (K, num_train))
    if K > TOPK_PATH_MAX_K:
        raise ValueError("K <= %d" % TOPK_PATH_MAX_K)
    if not (np.issubdtype(q.dtype, np.floating) and np.isfinite(q).all()):
        raise ValueError("Query must be a finite floating-point array")
    if not (np.issubdtype(gal.dtype, np.floating) and np.isfinite(gal).all()):
        raise ValueError("Gallery_features must be a finite floating-point array")
    books = cw.reshape(n_words, N_books, dim // N_books).transpose(1, 0, 2)
    code_rows, _ = _lib.pq_code_rows(codes, N_books, n_words)      # (raises ValueError on non-integer or out-of-range codes)
    coarse, _ = _lib.pq_train(gal, 1, n_clusters, seed=0)
    with _lib.PQIndex.empty(coarse, 1) as one_book:
        labels = one_book.encode(gal)[:, 0]
    rows = _refine_gallery(refine_rows, num_train, dim)
    try:
        with _lib.IVFPQIndex.from_codes(coarse[0], books, code_rows, labels) as g:
            t1 = time.time()
            if rows is None:
                idx, _, _ = g.search(q, K, nprobe=nprobe)
            else:
                idx, _, _ = g.search(q, K, nprobe=nprobe, refine=rows, k_factor=k_factor)
            t2 = time.time()
    finally:
        if rows is not None:
            rows.close()
    return idx, (t2 - t1) / max(num_test, 1)


def _l2_rows_f32(a, name):
    """The reference's normalisation (src/utils/nnsearch.py:832-835, 866-873): rows divided by their Euclidean norm in the
    array's own precision, then cast to float32."""
    a = np.asarray(a)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.floating):
        raise ValueError("%s must be a 2-D floating-point array (got %s %s)" % (name, a.dtype, a.shape))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (a / np.expand_dims(np.linalg.norm(a, axis=1), axis=1)).astype(np.float32)
    if not np.isfinite(out).all():
        raise ValueError("%s: rows must be finite and non-zero" % name)
    return out


def _pq_words(n_bits_perbook):
    n_bits = int(n_bits_perbook)
    if n_bits < 1 or (1 << n_bits) > _lib.PQ_MAX_WORDS:
        raise ValueError("n_bits_perbook = %d: a code byte holds Ks <= %d codewords per book (1 .. 8 bits)" % (n_bits, _lib.PQ_MAX_WORDS))
    return 1 << n_bits


def _pqw_words(n_bits_perbook):
    n_bits = int(n_bits_perbook)
    if n_bits < 1 or (1 << n_bits) > _lib.PQW_MAX_WORDS:
        raise ValueError("n_bits_perbook = %d: a wide PQ index holds Ks <= %d codewords per book (1 .. 13 bits)"
                         % (n_bits, _lib.PQW_MAX_WORDS))
    return 1 << n_bits


def _pq_books_path(dataset, n_books, n_words, stem="mi355_pq"):
    return os.path.join(os.path.dirname(_gallery_path(dataset)), "%s_M%d_Ks%d.npz" % (stem, n_books, n_words))


def _nano_pq(index_cls, embedded_features, N_books, N_words):
    """Nano_PQ_hip / Nano_PQ_wide_hip on their index class."""
    x = _l2_rows_f32(embedded_features, "embedded_features")
    N_books, N_words = int(N_books), int(N_words)
    with index_cls.fit(x, N_books, N_words, iters=20, seed=42) as g:
        books, codes = g.codebooks, g.get_codes()
    recon = np.concatenate([books[j][codes[:, j]] for j in range(N_books)], axis=1)
    codewords = np.ascontiguousarray(books.transpose(1, 0, 2)).reshape(N_words, -1)
    return codes, codewords, recon


def Nano_PQ_hip(embedded_features, N_books, N_words):
    """Same signature and return shape as Nano_PQ (src/utils/nnsearch.py:828-845): rows L2-normalised and cast to float32,
    codebooks learned on them (20 iterations, seed 42: _lib.pq_train), rows encoded -> (codes uint8 [N, N_books], Codewords
    [N_words, dim] in the reference's layout -- book j is the column block j * L .. (j + 1) * L -- and the reconstruction
    float32 [N, dim], codebooks[j, code[:, j]] gathered on the host).  The iteration is the one nanopq runs
    (scipy.cluster.vq.kmeans2, minit="matrix") in float64 with float32 centroids; nanopq's random draw of the initial rows
    is not reproduced, so the codebooks differ from nanopq's the way two seeds differ."""
    return _nano_pq(_lib.PQIndex, embedded_features, N_books, N_words)


def Nano_PQ_wide_hip(embedded_features, N_books, N_words):
    """Nano_PQ_hip on the wide index (_lib.WidePQIndex, _lib.pqw_train): N_words <= 8192, codes uint16 [N, N_books]; everything
    else as there."""
    return _nano_pq(_lib.WidePQIndex, embedded_features, N_books, N_words)


def matching_Nano_PQ_hip(K, embedded_features_train, embedded_features_test, dataset=None, N_books=16, n_bits_perbook=8,
                         ifgenerate=True):
    """Same signature and return shape as matching_Nano_PQ (src/utils/nnsearch.py:847-901), `--matching_method PQ`: both sides
    L2-normalised and cast to float32 as the reference does (:866-873), codebooks of N_books books of 2^n_bits_perbook
    codewords learned on the database rows (20 iterations, seed 42), rows encoded, exact ADC top-K
    -> (idx int64 [Q, K], time_per_query).  n_bits_perbook <= 8 (Ks <= 256, one byte per book; the reference's entry points pass
    13: matching_Nano_PQ_wide_hip, `PQ13`, takes it), 1 <= K <= min(N, 2048).  With a `dataset` the codebooks persist as
    outputs/<dataset>/mi355_pq_M<M>_Ks<Ks>.npz (written to a temporary name and renamed): learned and written iff `ifgenerate`,
    otherwise loaded -- a missing file raises FileNotFoundError, as the reference's open() does; dataset=None writes nothing
    (and needs ifgenerate).  The timer spans what the reference's spans (:892-900): the search only, device-synchronised.
    Learning is deterministic (see _lib.pq_train) but does not reproduce nanopq's random draw of initial rows.  Bad input raises
    ValueError before the device is touched."""
    return _matching_nano_pq(_lib.PQIndex, "mi355_pq", K, embedded_features_train, embedded_features_test, dataset, N_books,
                             _pq_words(n_bits_perbook), ifgenerate)


def matching_Nano_PQ_wide_hip(K, embedded_features_train, embedded_features_test, dataset=None, N_books=16, n_bits_perbook=13,
                              ifgenerate=True):
    """matching_Nano_PQ_hip on the wide index, with the reference's signature AND its defaults (src/utils/nnsearch.py:847; its
    entry points pass N_books = 16, n_bits_perbook = 13: src/offline.py:110): 1 <= n_bits_perbook <= 13, Ks = 2^n_bits_perbook <=
    8192 codewords per book, uint16 codes (_lib.WidePQIndex, _lib.pqw_train).  Normalisation, learning, timer, K and every refusal
    are matching_Nano_PQ_hip's; the codebooks persist as outputs/<dataset>/mi355_pqw_M<M>_Ks<Ks>.npz.  Learning needs N >= Ks rows.
    `PQ13` in MATCHING_METHODS."""
    return _matching_nano_pq(_lib.WidePQIndex, "mi355_pqw", K, embedded_features_train, embedded_features_test, dataset, N_books,
                             _pqw_words(n_bits_perbook), ifgenerate)


def _matching_nano_pq(index_cls, stem, K, embedded_features_train, embedded_features_test, dataset, N_books, n_words, ifgenerate):
    """The body of matching_Nano_PQ_hip and matching_Nano_PQ_wide_hip: index_cls is _lib.PQIndex or _lib.WidePQIndex, `stem` names
    the stored codebooks."""
    N_books, K = int(N_books), int(K)
    train = _l2_rows_f32(embedded_features_train, "embedded_features_train")
    test = _l2_rows_f32(embedded_features_test, "embedded_features_test")
    if train.shape[1] != test.shape[1]:
        raise ValueError("expected rows [N, dim] and queries [Q, dim], got %s and %s" % (train.shape, test.shape))
    num_train, num_test = train.shape[0], test.shape[0]
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d rows" % (K, num_train))
    if K > TOPK_PATH_MAX_K:
        raise ValueError("K <= %d" % TOPK_PATH_MAX_K)
    L = _lib._pq_train_shape(num_train, train.shape[1], N_books, n_words, 20, index_cls._MAX_WORDS)
    if dataset is None and not ifgenerate:
        raise ValueError("ifgenerate=False loads the codebooks of a dataset: give one")
    if ifgenerate:
        books, _ = index_cls._TRAIN(train, N_books, n_words, iters=20, seed=42)
        if dataset is not None:
            path = _pq_books_path(dataset, N_books, n_words, stem)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            tmp = "%s.tmp.%d.%s.npz" % (path, os.getpid(), uuid.uuid4().hex[:12])
            with _path_lock(path):
                np.savez(tmp, codebooks=books)
                os.replace(tmp, path)
    else:
        with np.load(_pq_books_path(dataset, N_books, n_words, stem)) as z:        # (FileNotFoundError when it was never generated)
            books = z["codebooks"]
        if books.shape != (N_books, n_words, L):
            raise ValueError("stored codebooks of shape %s, this call takes %s" % (books.shape, (N_books, n_words, L)))
    with index_cls.empty(books, num_train) as g:
        g.add(train)
        t1 = time.time()
        idx, _, _ = g.search(test, K)                  # (synchronous: the results are on the host when it returns)
        t2 = time.time()
    return idx, (t2 - t1) / max(num_test, 1)


def _fill_short_rows(idx, num_train):
    """Rows of idx [Q, K] with trailing -1s get the lowest indices not in the answer behind what was found, as the reference's
    graph matchers do (src/utils/nnsearch.py:532-534, 574-576)."""
    K = idx.shape[1]
    for row in np.flatnonzero((idx < 0).any(axis=1)):
        got = idx[row][idx[row] >= 0]
        miss = np.flatnonzero(~np.isin(np.arange(num_train), got))
        idx[row] = np.concatenate((got, miss))[:K]
    return idx


def _graph_path(dataset, R):
    return os.path.join(os.path.dirname(_gallery_path(dataset)), "mi355_graph_R%d.npz" % R)


def matching_HNSW_hip(K, embedded_features_train, embedded_features_test, dataset=None, m=4, ef=8, ifgenerate=True):
    """Same signature and return shape as matching_HNSW (src/utils/nnsearch.py:487-538), `--matching_method HNSW`: a neighbour
    graph over the database rows under squared Euclidean distance, searched best-first with a candidate list of K rows (the
    reference searches with ef=K, :531; its `ef` argument is efConstruction, which this build has no use for and ignores)
    -> (idx int64 [Q, K], time_per_query).  THE GRAPH IS THIS LIBRARY'S, not the reference's: _lib.GraphIndex.build with
    R = 2 * m neighbours per row (faiss's and the reference's bottom-layer degree m0) -- each row's m nearest rows, up to m
    reverse edges and further nearest rows, from the exact search, with 16 evenly spaced entry rows -- not an insertion-order HNSW
    with layers, and nothing pins it to that graph.  What is exact is the search GIVEN the graph: float64
    direct-form distances, ties to the lower index.  Where fewer than K rows are reached the tail is filled with the lowest
    indices not in the answer, as :532-534 does.  With a `dataset` the table and the entry rows persist as
    outputs/<dataset>/mi355_graph_R<R>.npz (written to a temporary name and renamed): built and written iff `ifgenerate`,
    otherwise loaded -- a missing file raises FileNotFoundError, as the reference's open() does; dataset=None writes nothing (and
    needs ifgenerate).  1 <= m <= 32, 1 <= K <= min(N, 2048), N >= 2.  The timer spans what the reference's spans (:528-536):
    the search only, device-synchronised.  Bad input raises ValueError before the device is touched."""
    train, test = np.asarray(embedded_features_train), np.asarray(embedded_features_test)
    if train.ndim != 2 or test.ndim != 2 or train.shape[1] != test.shape[1]:
        raise ValueError("expected rows [N, dim] and queries [Q, dim], got %s and %s" % (train.shape, test.shape))
    for name, a in (("embedded_features_train", train), ("embedded_features_test", test)):
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError("%s must be a floating-point array (got %s)" % (name, a.dtype))
    K, m = int(K), int(m)
    if m < 1 or 2 * m > _lib.GRAPH_MAX_R:
        raise ValueError("m = %d: the graph holds R = 2 * m <= %d neighbours per row" % (m, _lib.GRAPH_MAX_R))
    R = 2 * m
    num_train, num_test = train.shape[0], test.shape[0]
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d rows" % (K, num_train))
    if K > TOPK_PATH_MAX_K:
        raise ValueError("K <= %d" % TOPK_PATH_MAX_K)
    _lib._graph_build_shape(num_train, R, 16)
    if dataset is None and not ifgenerate:
        raise ValueError("ifgenerate=False loads the graph of a dataset: give one")
    if not ifgenerate:
        with np.load(_graph_path(dataset, R)) as z:                 # (FileNotFoundError when it was never generated)
            table, entries = _lib._graph_table(num_train, z["neighbors"], z["entries"])
        if table.shape[1] != R:
            raise ValueError("stored table of shape %s, this call takes [%d, %d]" % (table.shape, num_train, R))
    rows = Gallery.l2_from_host(train)
    try:
        if ifgenerate:
            g = _lib.GraphIndex.build(rows, R=R, n_entry=16)
        else:
            g = _lib.GraphIndex.from_neighbors(rows, table, entries)
        with g:
            if ifgenerate and dataset is not None:
                path = _graph_path(dataset, R)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                tmp = "%s.tmp.%d.%s.npz" % (path, os.getpid(), uuid.uuid4().hex[:12])
                with _path_lock(path):
                    np.savez(tmp, neighbors=g.neighbors, entries=g.entries)
                    os.replace(tmp, path)
            t1 = time.time()
            idx, _, _ = g.search(test, K, ef=K)            # (synchronous: the results are on the host when it returns)
            t2 = time.time()
    finally:
        rows.close()
    return _fill_short_rows(idx, num_train), (t2 - t1) / max(num_test, 1)


def _pq_graph_shape(K, num_train, m):
    """(K, R) of the PQ + HNSW matchers; raises ValueError outside 1 <= m <= 32, 1 <= K <= min(N, 2048), N >= 2."""
    K, m = int(K), int(m)
    if m < 1 or 2 * m > _lib.GRAPH_MAX_R:
        raise ValueError("m = %d: the graph holds R = 2 * m <= %d neighbours per row" % (m, _lib.GRAPH_MAX_R))
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d rows" % (K, num_train))
    if K > TOPK_PATH_MAX_K:
        raise ValueError("K <= %d" % TOPK_PATH_MAX_K)
    _lib._graph_build_shape(num_train, 2 * m, 16)
    return K, 2 * m


def matching_HNSW_PQ_hip(K, Codewords, embedded_features_test, CW_idx, m=4):
    """Same signature and return shape as matching_HNSW_PQ (src/utils/nnsearch.py:541-582), plus m (the reference fixes 4): a
    neighbour graph over the PQ codes CW_idx [N, N_books] under Codewords [N_words, dim] (book j is the column block j * L ..
    (j + 1) * L), searched best-first on asymmetric distances with a candidate list of K rows (the reference searches with
    ef=K, :573) -> (idx int64 [Q, K], time_per_query).  Queries are L2-normalised in their own precision as :546-548 does.
    THE GRAPH IS THIS LIBRARY'S, not the reference's: _lib.PQGraphIndex.build with R = 2 * m neighbours per row and 16 evenly
    spaced entry rows, built over the codes as given.  The codes are NOT de-duplicated: the reference's
    np.unique / reverse-index expansion returns the rows of a code together, which is what the order (distance asc, id asc) gives
    when the duplicates are reached.  What is exact is the search GIVEN the graph: the distances of matching_PQ_Net_hip, ties to
    the lower index.  Where fewer than K rows are reached the tail is filled with the lowest indices not in the answer, as
    :574-576 does.  N_words <= 256, dim % N_books == 0, 1 <= m <= 32, 1 <= K <= min(N, 2048), N >= 2; CW_idx must be an integer
    array with values in [0, N_words).  Bad input raises ValueError before the device is touched.  It is no (K, train, test)
    matcher and therefore not in MATCHING_METHODS.  The timer spans what the reference's spans: the search only,
    device-synchronised."""
    cw, q, codes = np.asarray(Codewords), np.asarray(embedded_features_test), np.asarray(CW_idx)
    if cw.ndim != 2 or q.ndim != 2 or codes.ndim != 2 or q.shape[1] != cw.shape[1]:
        raise ValueError("expected Codewords [N_words, dim], embedded_features_test [Q, dim] and CW_idx [N, N_books], got %s, %s and %s"
                         % (cw.shape, q.shape, codes.shape))
    n_words, dim = cw.shape
    n_books = codes.shape[1]
    if n_books < 1 or dim % n_books:
        raise ValueError("dim = %d is no multiple of N_books = %d" % (dim, n_books))
    if n_words > _lib.PQ_MAX_WORDS:
        raise ValueError("N_words = %d, a code byte holds at most %d codewords per book" % (n_words, _lib.PQ_MAX_WORDS))
    num_train, num_test = codes.shape[0], q.shape[0]
    K, R = _pq_graph_shape(K, num_train, m)
    if not np.issubdtype(q.dtype, np.floating):
        raise ValueError("embedded_features_test must be a floating-point array (got %s)" % q.dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = q / np.expand_dims(np.linalg.norm(q, axis=1), axis=1)
    if not np.isfinite(q).all():
        raise ValueError("embedded_features_test: rows must be finite and non-zero")
    books = _lib.pq_codebooks(cw.reshape(n_words, n_books, dim // n_books).transpose(1, 0, 2))
    code_rows, _ = _lib.pq_code_rows(codes, n_books, n_words)      # (raises ValueError on non-integer or out-of-range codes)
    with _lib.PQIndex.from_codes(books, code_rows) as pq, _lib.PQGraphIndex.build(pq, R=R, n_entry=16) as g:
        t1 = time.time()
        idx, _, _ = g.search(q, K, ef=K)                   # (synchronous: the results are on the host when it returns)
        t2 = time.time()
    return _fill_short_rows(idx, num_train), (t2 - t1) / max(num_test, 1)


def _pq_graph_path(dataset, n_books, n_words, R):
    return os.path.join(os.path.dirname(_gallery_path(dataset)), "mi355_pqgraph_M%d_Ks%d_R%d.npz" % (n_books, n_words, R))


def matching_HNSW_NanoPQ_hip(K, embedded_features, embedded_features_test, dataset=None, N_books=16, N_words=256, m=4, ef=8,
                             ifgenerate=True):
    """Same signature and return shape as matching_HNSW_NanoPQ (src/utils/nnsearch.py:585-683), `--matching_method PQ_HNSW`: both
    sides L2-normalised and cast to float32, codebooks of N_books books of N_words codewords learned on the database rows
    (_lib.pq_train: 20 iterations, seed 42), rows encoded, a neighbour graph built over the codes and searched best-first on
    asymmetric distances with a candidate list of K rows (the reference searches with ef=K, :675; its `ef` argument is
    efConstruction, which this build has no use for and ignores) -> (idx int64 [Q, K], time_per_query).  No raw row stays on the
    device: the index is N_books + 8 * m bytes per row.  THE GRAPH IS THIS LIBRARY'S, not the reference's:
    _lib.PQGraphIndex.build with R = 2 * m neighbours per row and 16 evenly spaced entry rows.  The codes are
    NOT de-duplicated: the reference's np.unique / dict_recover expansion returns the rows of a code together, which is what
    the order (distance asc, id asc) gives when the duplicates are reached.  What is exact is the search GIVEN codebooks, codes
    and graph: the distances of matching_Nano_PQ_hip, ties to the lower index.  Where fewer than K rows are reached the tail is
    filled with the lowest indices not in the answer, as :676-678 does.  N_words <= 256 (one byte per book; the reference's
    entry points pass 2**13, which this build does not take), 1 <= m <= 32, 1 <= K <= min(N, 2048), N >= max(2, N_words).  With
    a `dataset` codebooks, table and entry rows persist in one file outputs/<dataset>/mi355_pqgraph_M<M>_Ks<Ks>_R<R>.npz (written
    to a temporary name and renamed): learned, built and written iff `ifgenerate`, otherwise loaded -- a missing file raises
    FileNotFoundError, as the reference's open() does; dataset=None writes nothing (and needs ifgenerate).  The timer spans what
    the reference's spans (:670-682): the search only, device-synchronised.  Learning is deterministic (see _lib.pq_train) but
    does not reproduce nanopq's random draw of initial rows.  Bad input raises ValueError before the device is touched."""
    N_books, N_words = int(N_books), int(N_words)
    if N_words < 2 or N_words > _lib.PQ_MAX_WORDS:
        raise ValueError("N_words = %d: a code byte holds 2 .. %d codewords per book" % (N_words, _lib.PQ_MAX_WORDS))
    train = _l2_rows_f32(embedded_features, "embedded_features")
    test = _l2_rows_f32(embedded_features_test, "embedded_features_test")
    if train.shape[1] != test.shape[1]:
        raise ValueError("expected rows [N, dim] and queries [Q, dim], got %s and %s" % (train.shape, test.shape))
    num_train, num_test = train.shape[0], test.shape[0]
    K, R = _pq_graph_shape(K, num_train, m)
    L = _lib._pq_train_shape(num_train, train.shape[1], N_books, N_words, 20)
    if dataset is None and not ifgenerate:
        raise ValueError("ifgenerate=False loads codebooks and graph of a dataset: give one")
    if ifgenerate:
        books, _ = _lib.pq_train(train, N_books, N_words, iters=20, seed=42)
    else:
        with np.load(_pq_graph_path(dataset, N_books, N_words, R)) as z:     # (FileNotFoundError when it was never generated)
            books = z["codebooks"]
            table, entries = _lib._graph_table(num_train, z["neighbors"], z["entries"])
        if books.shape != (N_books, N_words, L) or table.shape[1] != R:
            raise ValueError("stored codebooks of shape %s and table of shape %s, this call takes %s and [%d, %d]"
                             % (books.shape, table.shape, (N_books, N_words, L), num_train, R))
    with _lib.PQIndex.empty(books, num_train) as pq:
        pq.add(train)
        g = _lib.PQGraphIndex.build(pq, R=R, n_entry=16) if ifgenerate else _lib.PQGraphIndex.from_neighbors(pq, table, entries)
        with g:
            if ifgenerate and dataset is not None:
                path = _pq_graph_path(dataset, N_books, N_words, R)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                tmp = "%s.tmp.%d.%s.npz" % (path, os.getpid(), uuid.uuid4().hex[:12])
                with _path_lock(path):
                    np.savez(tmp, codebooks=books, neighbors=g.neighbors, entries=g.entries)
                    os.replace(tmp, path)
            t1 = time.time()
            idx, _, _ = g.search(test, K, ef=K)            # (synchronous: the results are on the host when it returns)
            t2 = time.time()
    return _fill_short_rows(idx, num_train), (t2 - t1) / max(num_test, 1)


# the matchers of this build by the name the reference's entry points dispatch on (--matching_method, src/offline.py:107-118)
def _forest_path(dataset, T, L):
    return os.path.join(os.path.dirname(_gallery_path(dataset)), "mi355_forest_T%d_L%d.npz" % (T, L))


def matching_ANNOY_hip(K, embedded_features_train, embedded_features_test, metric="euclidean", dataset=None, n_trees=100,
                       ifgenerate=True):
    """Same signature and return shape as matching_ANNOY (src/utils/nnsearch.py; src/test_rOP1m.py:156 calls it with 'euclidean' and
    n_trees=100), `--matching_method ANNOY`: a forest of n_trees random-projection trees over the database rows, a query descends
    every tree and the rows of the leaves it reaches are ranked by their exact distances -> (idx int64 [Q, K], time_per_query).
    THE FOREST IS THIS LIBRARY'S, not the reference's: _lib.ForestIndex.build -- one standard normal direction (seed 5) per level of
    a tree, every node split at the median of its rows' projections, the depth chosen by _lib._forest_shape (leaves of at most 64
    rows) -- not annoy's two-means hyperplanes, its random numbers, its search_k queue or its file format, and nothing pins it to
    annoy's trees.  What is exact is the search GIVEN the forest: float64 direct-form distances over the union of
    the leaves, ties to the lower index.  metric 'euclidean': the raw rows in a squared-L2 gallery; 'angular': rows and queries
    L2-normalised first (annoy's angular distance sqrt(2 - 2 cos) orders as the squared distance of the normalised rows does);
    anything else raises ValueError.  Where the leaves hold fewer than K distinct rows the tail is filled with the lowest indices
    not in the answer.  With a `dataset` the directions, split values and permutations persist as
    outputs/<dataset>/mi355_forest_T<T>_L<L>.npz (written to a temporary name and renamed): built and written iff `ifgenerate`,
    otherwise loaded -- a missing file raises FileNotFoundError; dataset=None writes nothing (and needs ifgenerate).
    1 <= n_trees <= 256, 1 <= K <= min(N, n_trees * leaf_max), N >= 2.  The timer spans what the reference's spans: the search
    only, device-synchronised.  Bad input raises ValueError before the device is touched."""
    if metric not in ("euclidean", "angular"):
        raise ValueError("metric = %r: 'euclidean' or 'angular'" % (metric,))
    train, test = np.asarray(embedded_features_train), np.asarray(embedded_features_test)
    if train.ndim != 2 or test.ndim != 2 or train.shape[1] != test.shape[1]:
        raise ValueError("expected rows [N, dim] and queries [Q, dim], got %s and %s" % (train.shape, test.shape))
    for name, a in (("embedded_features_train", train), ("embedded_features_test", test)):
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError("%s must be a floating-point array (got %s)" % (name, a.dtype))
    K, T = int(K), int(n_trees)
    num_train, num_test = train.shape[0], test.shape[0]
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d rows" % (K, num_train))
    L, _ = _lib._forest_shape(K, num_train, T)
    _lib._forest_check(num_train, train.shape[1], T, L)
    if dataset is None and not ifgenerate:
        raise ValueError("ifgenerate=False loads the forest of a dataset: give one")
    if metric == "angular":
        train = _l2_rows_f32(train, "embedded_features_train")
        test = _l2_rows_f32(test, "embedded_features_test")
    if not ifgenerate:
        with np.load(_forest_path(dataset, T, L)) as z:              # (FileNotFoundError when it was never generated)
            trees = _lib._forest_trees(num_train, train.shape[1], z["dirs"], z["splits"], z["leaves"])[:3]
    rows = Gallery.l2_from_host(train)
    try:
        f = _lib.ForestIndex.build(rows, n_trees=T, depth=L, seed=5) if ifgenerate else _lib.ForestIndex.from_trees(rows, *trees)
        with f:
            if ifgenerate and dataset is not None:
                path = _forest_path(dataset, T, L)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                tmp = "%s.tmp.%d.%s.npz" % (path, os.getpid(), uuid.uuid4().hex[:12])
                with _path_lock(path):
                    np.savez(tmp, dirs=f.dirs(), splits=f.splits(), leaves=f.leaves())
                    os.replace(tmp, path)
            t1 = time.time()
            idx, _, _ = f.search(test, K)                  # (synchronous: the results are on the host when it returns)
            t2 = time.time()
    finally:
        rows.close()
    return _fill_short_rows(idx, num_train), (t2 - t1) / max(num_test, 1)


def _ivfflat_path(dataset, nlist):
    return os.path.join(os.path.dirname(_gallery_path(dataset)), "mi355_ivfflat_L%d.npz" % nlist)


def ivfflat_default_nlist(num_train):
    """faiss's rule of thumb for the lists of an inverted file, 4 sqrt(N), kept within what the index takes: 2 .. 8192."""
    return int(min(_lib.IVFFLAT_MAX_LISTS, max(2, round(4 * np.sqrt(int(num_train))))))


def matching_IVF_hip(K, embedded_features_train, embedded_features_test, dataset=None, nlist=None, nprobe=8, metric="euclidean",
                     ifgenerate=True):
    """An inverted file over the raw database rows, faiss IndexIVFFlat -- the reference's matching_PQ_Net_bucket
    (src/utils/nnsearch.py:949-998) without the PQ loss --, `--matching_method IVF`, with the reference's return convention
    -> (idx int64 [Q, K], time_per_query).  nlist centroids are learned on the database rows (_lib.IVFFlatIndex.train: the
    library's deterministic k-means, seed 0; nlist=None: ivfflat_default_nlist(N) = min(8192, max(2, round(4 sqrt(N))))), every
    row goes to the list of its nearest centroid, and a query's answer is the exact top K, by float64 direct-form distance with
    ties to the lower index, among the rows of its nprobe nearest lists; nprobe == nlist is the exhaustive
    answer of matching_L2_hip.  metric 'euclidean': the raw rows in a squared-L2 gallery; 'angular': rows and queries L2-normalised
    first; anything else raises ValueError.  Where the probed lists hold fewer than K rows the tail is filled with the lowest indices
    not in the answer, as the reference's graph matchers do.  With a `dataset` the centroids and the list of every row persist as
    outputs/<dataset>/mi355_ivfflat_L<nlist>.npz (written to a temporary name and renamed): trained, assigned and written iff
    `ifgenerate`, otherwise loaded -- a missing file raises FileNotFoundError; dataset=None writes nothing (and needs ifgenerate).
    2 <= nlist <= min(N, 8192), 1 <= nprobe <= nlist, 1 <= K <= min(N, 2048).  The timer spans the search only,
    device-synchronised.  Bad input raises ValueError before the device is touched.  The speed of this index has not been measured."""
    if metric not in ("euclidean", "angular"):
        raise ValueError("metric = %r: 'euclidean' or 'angular'" % (metric,))
    train, test = np.asarray(embedded_features_train), np.asarray(embedded_features_test)
    if train.ndim != 2 or test.ndim != 2 or train.shape[1] != test.shape[1]:
        raise ValueError("expected rows [N, dim] and queries [Q, dim], got %s and %s" % (train.shape, test.shape))
    for name, a in (("embedded_features_train", train), ("embedded_features_test", test)):
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError("%s must be a floating-point array (got %s)" % (name, a.dtype))
    K, nprobe = int(K), int(nprobe)
    num_train, num_test = train.shape[0], test.shape[0]
    if K < 1 or K > num_train:
        raise ValueError("K = %d, the database holds %d rows" % (K, num_train))
    if K > _lib.IVFFLAT_MAX_K:
        raise ValueError("K <= %d" % _lib.IVFFLAT_MAX_K)
    nlist = ivfflat_default_nlist(num_train) if nlist is None else int(nlist)
    if not 2 <= nlist <= min(num_train, _lib.IVFFLAT_MAX_LISTS):
        raise ValueError("nlist = %d: 2 .. min(N = %d, %d) lists" % (nlist, num_train, _lib.IVFFLAT_MAX_LISTS))
    if not 1 <= nprobe <= nlist:
        raise ValueError("nprobe = %d, the index has nlist = %d lists (1 .. nlist)" % (nprobe, nlist))
    if dataset is None and not ifgenerate:
        raise ValueError("ifgenerate=False loads the lists of a dataset: give one")
    if metric == "angular":
        train = _l2_rows_f32(train, "embedded_features_train")
        test = _l2_rows_f32(test, "embedded_features_test")
    if not ifgenerate:
        with np.load(_ivfflat_path(dataset, nlist)) as z:            # (FileNotFoundError when it was never generated)
            cent = _lib.ivfflat_centroids(z["centroids"], train.shape[1])
            lids = _lib.ivfflat_list_ids(z["list_ids"], num_train, cent.shape[0])
        if cent.shape[0] != nlist:
            raise ValueError("stored centroids of shape %s, this call takes [%d, %d]" % (cent.shape, nlist, train.shape[1]))
    else:
        cent = _lib.IVFFlatIndex.train(train, nlist, seed=0)
    rows = Gallery.l2_from_host(train)
    try:
        f = _lib.IVFFlatIndex.build(rows, cent) if ifgenerate else _lib.IVFFlatIndex.from_lists(rows, cent, lids)
        with f:
            if ifgenerate and dataset is not None:
                path = _ivfflat_path(dataset, nlist)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                tmp = "%s.tmp.%d.%s.npz" % (path, os.getpid(), uuid.uuid4().hex[:12])
                with _path_lock(path):
                    np.savez(tmp, centroids=f.centroids(), list_ids=f.list_ids())
                    os.replace(tmp, path)
            t1 = time.time()
            idx, _, _ = f.search(test, K, nprobe=nprobe)   # (synchronous: the results are on the host when it returns)
            t2 = time.time()
    finally:
        rows.close()
    return _fill_short_rows(idx, num_train), (t2 - t1) / max(num_test, 1)


MATCHING_METHODS = {"HIP": matching_HIP, "L2": matching_L2_hip, "Greedyhash": matching_Greedyhash_hip, "PQ": matching_Nano_PQ_hip,
                    "PQ13": matching_Nano_PQ_wide_hip, "HNSW": matching_HNSW_hip, "PQ_HNSW": matching_HNSW_NanoPQ_hip,
                    "ANNOY": matching_ANNOY_hip, "IVF": matching_IVF_hip}


def _reference_unit_rows(a):
    """x / ||x|| per row as the reference's matchers normalise (src/utils/nnsearch.py:715-720: np.linalg.norm in the array's own
    dtype), as the float32 rows a gallery stores."""
    a = np.asarray(a)
    return np.ascontiguousarray(a / np.expand_dims(np.linalg.norm(a, axis=1), axis=1), dtype=np.float32)


def _fractional_search(K, embedded_features_train, embedded_features_test, p):
    """int64 [Q, K]: the K rows of smallest sum |q - x| ** p per query over unit rows and unit queries, ascending, ties to the lower
    id (Gallery.search_minkowski, metric "lp").  The reference's fractional_distance is that sum ** (1 / p): the same order."""
    train, test = _reference_unit_rows(embedded_features_train), _reference_unit_rows(embedded_features_test)
    K = int(K)
    if K > train.shape[0]:
        raise RuntimeError("mi355_retrieval error 1: k > number of gallery rows")
    g = _lib.Gallery.from_host(train, norm_mode=NORM_NONE)
    try:
        idx, _, _, _ = g.search_minkowski(test, K, "lp", p)
    finally:
        g.close()
    return idx


def matching_fractional_dis_hip(K, embedded_features_train, embedded_features_test, p=2):
    """Same signature and return shape as matching_fractional_dis (src/utils/nnsearch.py:709-731).  The reference calls
    its fractional distance with p = 2 (:721), which orders the gallery exactly like matching_L2, and slices the QUERY
    axis of the argsort by K before the gallery axis (:723-724): it returns the rankings of the first min(Q, K) queries,
    int64 [min(Q, K), K].  Reproduced as is; the timer divides by all queries like the reference's (:730).
    p != 2: what the reference's function would return had it passed that p on to fractional_distance (whose own default is
    0.5): rows and queries normalised as there, the exact Lp top-K of the HIP scan, the same slice."""
    t1 = time.time()
    test = np.asarray(embedded_features_test)
    num_test = test.shape[0]
    if p == 2:
        idx, _ = matching_HIP(K, embedded_features_train, test[:int(K)])
    else:
        idx = _fractional_search(K, embedded_features_train, test[:int(K)], p)
    return idx, (time.time() - t1) / num_test


def matching_Lp_hip(K, embedded_features_train, embedded_features_test, p=0.5):
    """(K, train, test) matcher by the reference's fractional_distance (src/utils/nnsearch.py:46-56, p = 0.5 by default) over unit
    rows and unit queries: -> (idx int64 [Q, K], time_per_query), every query answered (no slice of the query axis)."""
    t1 = time.time()
    test = np.asarray(embedded_features_test)
    idx = _fractional_search(K, embedded_features_train, test, p)
    return idx, (time.time() - t1) / max(test.shape[0], 1)


MATCHING_METHODS["Lp"] = matching_Lp_hip


def ip_rank_hip(vecs, qvecs, dataset=None, ifgenerate=False, device=0, return_scores=False):
    """`ranks = np.argsort(-(vecs.T @ qvecs), axis=0)` in full (src/main_retrieve.py:175-176): int64 [N,Q]."""
    g = get_gallery(np.asarray(vecs).T, dataset, ifgenerate, NORM_NONE, device)
    try:
        out = g.rank_all(np.asarray(qvecs).T, return_scores=return_scores)
    finally:
        if dataset is None:
            g.close()
    return (out[0].T, out[1].T) if return_scores else out[0].T


def ip_topk_hip(vecs, qvecs, K, dataset=None, ifgenerate=False, device=0):
    """Top-K rows of `argsort(-(vecs.T @ qvecs), axis=0)` (src/main_retrieve.py:175-176): raw inner
    product, no normalisation.  vecs [D,N], qvecs [D,Q] -> (ranks int64 [K,Q], scores f32 [K,Q])."""
    g = get_gallery(np.asarray(vecs).T, dataset, ifgenerate, NORM_NONE, device)
    try:
        idx, sc, _ = g.search(np.asarray(qvecs).T, int(K))
    finally:
        if dataset is None:
            g.close()
    return idx.T, sc.T
