"""GPU: row removal in place on the PQ and the IVF-PQ index (mi_pq_remove_rows, mi_ivfpq_remove_rows).  The
truth of every case is a FRESH index built from codes[keep] (and lists[keep]) with the same capacity, and the numpy truth
functions on those same arrays: n, the stored codes and lists, the list sizes, ids and distance BITS of the searches.  Every
comparison is for equality.  d = 32 everywhere except at M = 5, which does not divide 32: there d = 30 (L = 6)."""
import ctypes as C

import numpy as np
import pytest

from _ivfpq_residual_truth import residual_encode_truth, residual_ivfpq_truth
from _ivfpq_truth import ivfpq_truth, probe_truth
from _pq_truth import encode_truth, pq_truth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want):
    """(ids, dist) pairs equal: ids by value, distances by bits"""
    return np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))


def _books(rng, M, Ks):
    return rng.standard_normal((M, Ks, 32 // M if 32 % M == 0 else 6)).astype(np.float32)


def _pq_problem(seed, n, M, Ks, nq=4):
    rng = np.random.default_rng(seed)
    Cb = _books(rng, M, Ks)
    codes = rng.integers(0, Ks, size=(n, M), dtype=np.uint8)
    if n > 4:
        codes[n - 1] = codes[0]                                           # an exact tie between the first and the last row
    q = rng.standard_normal((nq, Cb.shape[0] * Cb.shape[2])).astype(np.float32)
    return Cb, codes, q


def _flat_patterns(n, seed):
    """name -> bool [n] of the rows that leave; masks that coincide at a small n are given once"""
    rng = np.random.default_rng(seed)
    out = {}

    def put(name, mask):
        if mask.any() and not any(np.array_equal(mask, m) for m in out.values()):
            out[name] = mask

    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0], last[n - 1] = True, True
    put("first row", first)
    put("last row", last)
    if n >= 64:
        blk = np.zeros(n, bool)
        b0 = 64 if n >= 128 else 0
        blk[b0:b0 + 64] = True
        put("one whole block", blk)
    put("every other row", np.arange(n) % 2 == 0)
    put("random half", rng.random(n) < 0.5)
    but_one = np.ones(n, bool)
    but_one[n // 2] = False
    put("all but one", but_one)
    put("all rows", np.ones(n, bool))
    return out


def _pq_n(lib, idx):
    n = C.c_int64(-1)
    lib.check(lib.load().mi_pq_info(idx._h, C.byref(n), None, None, None, None, None, None, None))
    return n.value


def _fresh_pq(lib, Cb, codes, row_offset, capacity):
    if codes.shape[0] == 0:
        return lib.PQIndex.empty(Cb, capacity, row_offset=row_offset)
    return lib.PQIndex.from_codes(Cb, codes, row_offset=row_offset, capacity=capacity)


def _check_pq(lib, idx, Cb, codes, q, row_offset, capacity, label=""):
    """idx holds exactly `codes`: n, get_codes, and the searches against a fresh index over `codes` and against pq_truth"""
    n = codes.shape[0]
    assert idx.n == n == _pq_n(lib, idx), label
    assert np.array_equal(idx.get_codes(), codes), label
    with _fresh_pq(lib, Cb, codes, row_offset, capacity) as fresh:
        for k in (1, 10, min(n + 3, 2048)):
            got = idx.search(q, k)[:2]
            assert _same(got, fresh.search(q, k)[:2]), (label, k)
            assert _same(got, pq_truth(q, Cb, codes, k, row_offset=row_offset)), (label, k)
        if n:
            allowed = np.random.default_rng(n).random(n) < 0.5           # a bitmap in the NEW numbering
            got = idx.search(q, 10, allow=allowed)[:2]
            assert _same(got, pq_truth(q, Cb, codes, 10, row_offset=row_offset, allowed=allowed)), label


# ---- 1. flat PQ sweep

@pytest.mark.parametrize("M,Ks", [(4, 16), (5, 16), (16, 256)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 1000])
def test_flat_sweep(lib, n, M, Ks):
    Cb, codes, q = _pq_problem(100 * n + M, n, M, Ks)
    for name, gone in _flat_patterns(n, n + M).items():
        with lib.PQIndex.from_codes(Cb, codes) as idx:
            kept = idx.remove(gone)
            assert kept.dtype == np.int64 and np.array_equal(kept, np.flatnonzero(~gone)), name
            _check_pq(lib, idx, Cb, codes[~gone], q, 0, n, label=name)
            if not (~gone).any():                                         # removing every row leaves a valid empty index
                ids, dist, _ = idx.search(q, 3)
                assert (ids == -1).all() and np.isposinf(dist).all()
                idx.append_codes(codes[:1])
                _check_pq(lib, idx, Cb, codes[:1], q, 0, n, label=name + ", then one row")


# ---- 2. chunking

def test_many_chunks_give_the_result_of_one(lib):
    n = 64 * 7 + 17
    Cb, codes, q = _pq_problem(2, n, 5, 16)
    gone = np.random.default_rng(3).random(n) < 1 / 3
    gone[[0, 70]] = False, True
    assert lib.get_global_option("pq_remove_block_rows") > n
    with lib.PQIndex.from_codes(Cb, codes) as one:
        one.remove(gone)
        want_codes, want = one.get_codes(), one.search(q, n)[:2]
    try:
        lib.set_global_option("pq_remove_block_rows", 64)
        with lib.PQIndex.from_codes(Cb, codes) as idx:
            idx.remove(gone)
            assert np.array_equal(idx.get_codes(), want_codes) and _same(idx.search(q, n)[:2], want)
            _check_pq(lib, idx, Cb, codes[~gone], q, 0, n)
        lib.set_global_option("pq_remove_block_rows", 128)               # two blocks per chunk, the last chunk short
        with lib.PQIndex.from_codes(Cb, codes) as idx:
            idx.remove(gone)
            assert np.array_equal(idx.get_codes(), want_codes) and _same(idx.search(q, n)[:2], want)
    finally:
        lib.set_global_option("pq_remove_block_rows", 0)


# ---- 3. IVF-PQ sweep

def _draw_lists(rng, n, nlist):
    """list 0 is the large one (more than 128 rows where n allows; exactly one full block at n = 65, nlist = 2), list 1 the small
    one (fewer than 64 rows), the others share the rest; in random row order"""
    small = 1 if n < 128 else 40
    big = n - small if nlist == 2 else n // 2
    rest = n - small - big
    li = np.concatenate([np.zeros(big, np.int64), np.ones(small, np.int64), rng.integers(2, max(nlist, 3), size=rest)])
    return rng.permutation(li).astype(np.uint8)


def _ivf_problem(seed, n, nlist, M, Ks, nq=4):
    rng = np.random.default_rng(seed)
    Cb = _books(rng, M, Ks)
    d = Cb.shape[0] * Cb.shape[2]
    G = (3 * rng.standard_normal((nlist, d))).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M), dtype=np.uint8)
    lists = _draw_lists(rng, n, nlist)
    if n > 4:
        codes[n - 1] = codes[0]                                           # the same code twice: a tie where the lists agree
    q = (G[rng.integers(0, nlist, size=nq)] + rng.standard_normal((nq, d))).astype(np.float32)
    return G, Cb, codes, lists, q


def _ivf_patterns(n, lists, seed):
    out = _flat_patterns(n, seed)

    def put(name, mask):
        if mask.any() and not any(np.array_equal(mask, m) for m in out.values()):
            out[name] = mask

    chain = np.flatnonzero(lists == 0)                                    # the rows of list 0 in the order of its chain
    put("a whole list", lists == 0)
    put("the small list", lists == 1)
    if chain.size >= 64:
        m = np.zeros(n, bool)
        m[chain[:64]] = True
        put("the first block of a chain", m)
    if chain.size % 64:
        m = np.zeros(n, bool)
        m[chain[chain.size // 64 * 64:]] = True
        put("the last, partly filled block of a chain", m)
    return out


def _fresh_ivf(lib, kind, G, Cb, codes, lists, row_offset, capacity):
    if codes.shape[0] == 0:
        return lib.IVFPQIndex.empty(G, Cb, capacity, row_offset=row_offset, by_residual=kind)
    return lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=row_offset, capacity=capacity, by_residual=kind)


def _ivf_truth(kind, q, G, Cb, codes, lists, probes, k, row_offset, allowed=None):
    if kind:
        return residual_ivfpq_truth(q, G, Cb, codes, lists, probes, k, row_offset=row_offset, allowed=allowed)
    return ivfpq_truth(q, Cb, codes, lists, probes, k, row_offset=row_offset, allowed=allowed)


def _check_ivf(lib, kind, idx, G, Cb, codes, lists, q, row_offset, capacity, label=""):
    """idx holds exactly (codes, lists): n, list sizes, get_rows and the searches -- library and explicit probes, with and without
    a bitmap in the new numbering -- against a fresh index and against the numpy truth"""
    n, nlist = codes.shape[0], G.shape[0]
    hb = idx._info()
    assert idx.n == n and hb > 0, label
    assert np.array_equal(idx.list_sizes(), np.bincount(lists, minlength=nlist)), label
    stored = idx.get_rows()
    assert np.array_equal(stored[0], codes) and np.array_equal(stored[1], lists), label
    rng = np.random.default_rng(n + 7)
    allowed = rng.random(n) < 0.5
    k = min(n + 3, 200)
    with _fresh_ivf(lib, kind, G, Cb, codes, lists, row_offset, capacity) as fresh:
        assert np.array_equal(fresh.list_sizes(), idx.list_sizes()), label
        for nprobe in (1, nlist):
            explicit = rng.integers(-1, nlist, size=(q.shape[0], nprobe)).astype(np.int32)
            chosen = probe_truth(q, G, nprobe)
            assert np.array_equal(idx.probe(q, nprobe), chosen), label
            for allow in ((None, allowed) if n else (None,)):
                got = idx.search(q, k, nprobe=nprobe, allow=allow)[:2]
                assert _same(got, fresh.search(q, k, nprobe=nprobe, allow=allow)[:2]), (label, nprobe, "library probes")
                assert _same(got, _ivf_truth(kind, q, G, Cb, codes, lists, chosen, k, row_offset, allow)), (label, nprobe)
                got = idx.search(q, k, probes=explicit, allow=allow)[:2]
                assert _same(got, fresh.search(q, k, probes=explicit, allow=allow)[:2]), (label, nprobe, "explicit probes")
                assert _same(got, _ivf_truth(kind, q, G, Cb, codes, lists, explicit, k, row_offset, allow)), (label, nprobe)
        if not kind:                                                      # every list probed: the flat index over the survivors
            with _fresh_pq(lib, Cb, codes, row_offset, capacity) as flat:
                assert _same(idx.search(q, k, nprobe=nlist)[:2], flat.search(q, k)[:2]), label


@pytest.mark.parametrize("kind", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("nlist", [2, 7])
@pytest.mark.parametrize("n", [65, 300, 1500])
def test_ivf_sweep(lib, n, nlist, kind):
    M, Ks = (4, 16) if n != 300 else (5, 16)
    G, Cb, codes, lists, q = _ivf_problem(10 * n + nlist, n, nlist, M, Ks)
    sizes = np.bincount(lists, minlength=nlist)
    assert sizes[1] < 64 and (sizes[0] > 128 or n == 65)
    for name, gone in _ivf_patterns(n, lists, n + nlist).items():
        with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=kind) as idx:
            kept = idx.remove(gone)
            assert kept.dtype == np.int64 and np.array_equal(kept, np.flatnonzero(~gone)), name
            _check_ivf(lib, kind, idx, G, Cb, codes[~gone], lists[~gone], q, 0, n, label=name)
            if not (~gone).any():
                ids, dist, _ = idx.search(q, 3, nprobe=nlist)
                assert (ids == -1).all() and np.isposinf(dist).all()


# ---- 4. life after removal

def test_flat_fill_remove_refill_remove_remove(lib):
    c, M, Ks = 64 * 5 + 17, 4, 16
    Cb, codes, q = _pq_problem(40, c, M, Ks)
    rng = np.random.default_rng(41)
    with lib.PQIndex.from_codes(Cb, codes) as idx:
        assert idx.capacity == c
        gone = rng.random(c) < 0.5
        idx.remove(gone)
        have = codes[~gone]
        _check_pq(lib, idx, Cb, have, q, 0, c, label="first removal")
        x = rng.standard_normal((c - have.shape[0], 32)).astype(np.float32)
        idx.add(x)                                                        # to the brim again
        have = np.concatenate([have, encode_truth(x, Cb)])
        assert idx.n == c
        _check_pq(lib, idx, Cb, have, q, 0, c, label="refilled")
        with pytest.raises(RuntimeError, match="capacity"):
            idx.append_codes(codes[:1])
        for step in range(2):                                             # twice in a row
            gone = rng.random(have.shape[0]) < 0.4
            kept = idx.remove(gone)
            assert np.array_equal(kept, np.flatnonzero(~gone))
            have = have[~gone]
            _check_pq(lib, idx, Cb, have, q, 0, c, label="removal %d after the refill" % step)


@pytest.mark.parametrize("kind", [False, True], ids=["plain", "residual"])
def test_ivf_fill_remove_refill_remove_remove(lib, kind):
    """Every list ends in a partly filled block, so the pool (ceil(c / 64) + nlist blocks) is as full as it gets; the refill sends
    half of its rows to ONE small list, which needs new blocks: they have to come from the ones the removal emptied."""
    sizes = [130, 40, 70, 65, 1, 100, 63]
    nlist, c, M, Ks = len(sizes), sum(sizes), 4, 16
    rng = np.random.default_rng(50 + kind)
    G, Cb, codes, _, q = _ivf_problem(51, c, nlist, M, Ks)
    lists = rng.permutation(np.repeat(np.arange(nlist), sizes)).astype(np.uint8)
    with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=kind) as idx:
        assert idx.capacity == c
        gone = rng.random(c) < 0.5
        idx.remove(gone)
        have_c, have_l = codes[~gone], lists[~gone]
        _check_ivf(lib, kind, idx, G, Cb, have_c, have_l, q, 0, c, label="first removal")
        room = c - have_c.shape[0]
        x = (G[rng.integers(0, nlist, size=room // 2)] + rng.standard_normal((room // 2, 32))).astype(np.float32)
        idx.add(x)
        if kind:
            new_c, new_l = residual_encode_truth(x, G, Cb)
        else:
            new_c, new_l = encode_truth(x, Cb), probe_truth(x, G, 1)[:, 0].astype(np.uint8)
        more = rng.integers(0, Ks, size=(room - room // 2, M), dtype=np.uint8)
        idx.append_codes(more, np.full(more.shape[0], 4, np.uint8))       # all into the list that had one row
        have_c = np.concatenate([have_c, new_c, more])
        have_l = np.concatenate([have_l, new_l, np.full(more.shape[0], 4, np.uint8)])
        assert idx.n == c
        _check_ivf(lib, kind, idx, G, Cb, have_c, have_l, q, 0, c, label="refilled")
        with pytest.raises(RuntimeError, match="capacity"):
            idx.append_codes(codes[:1], lists[:1])
        for step in range(2):
            gone = rng.random(have_c.shape[0]) < 0.4
            kept = idx.remove(gone)
            assert np.array_equal(kept, np.flatnonzero(~gone))
            have_c, have_l = have_c[~gone], have_l[~gone]
            _check_ivf(lib, kind, idx, G, Cb, have_c, have_l, q, 0, c, label="removal %d after the refill" % step)
        # and to the brim once more, every row into one list
        room = c - have_c.shape[0]
        more = rng.integers(0, Ks, size=(room, M), dtype=np.uint8)
        idx.append_codes(more, np.full(room, 1, np.uint8))
        have_c, have_l = np.concatenate([have_c, more]), np.concatenate([have_l, np.full(room, 1, np.uint8)])
        _check_ivf(lib, kind, idx, G, Cb, have_c, have_l, q, 0, c, label="refilled into one list")


# ---- 5. other entry forms

def _device_words(torch, words):
    t = torch.from_numpy(np.asarray(words).view(np.int64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


def test_flat_entry_forms(lib):
    import torch
    n, off = 200, 1000
    Cb, codes, q = _pq_problem(60, n, 5, 16)
    gone = np.random.default_rng(61).random(n) < 0.4
    gone[[0, n - 1]] = True
    ids = np.flatnonzero(gone) + off
    want_kept = np.flatnonzero(~gone) + off
    with lib.PQIndex.from_codes(Cb, codes, row_offset=off) as idx:       # global ids, with duplicates, unordered
        kept = idx.remove(np.concatenate([ids[::-1], ids[:5]]))
        assert np.array_equal(kept, want_kept)
        _check_pq(lib, idx, Cb, codes[~gone], q, off, n, label="global ids")
        with pytest.raises(ValueError):
            idx.remove([off - 1])
    words = np.asarray(lib.allow_bitmap(gone, n)).copy()
    with lib.PQIndex.from_codes(Cb, codes, row_offset=off) as idx:       # the bitmap as a device buffer
        dev = _device_words(torch, words)
        removed = C.c_int64(-1)
        lib.check(lib.load().mi_pq_remove_rows(idx._h, C.c_void_p(dev.data_ptr()), lib.MI_DEVICE, C.byref(removed)))
        assert removed.value == int(gone.sum())
        idx.n = n - removed.value
        _check_pq(lib, idx, Cb, codes[~gone], q, off, n, label="device bitmap")
    with lib.PQIndex.from_codes(Cb, codes, row_offset=off) as idx:       # bits beyond n are ignored
        beyond = words.copy()
        beyond[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
        assert beyond[-1] != words[-1]
        kept = idx.remove(beyond.view(lib.AllowBits))
        assert np.array_equal(kept, want_kept)
        _check_pq(lib, idx, Cb, codes[~gone], q, off, n, label="bits beyond n")
    with lib.PQIndex.from_codes(Cb, codes, row_offset=off) as idx:       # a bitmap that names no row
        before = idx.search(q, n)[:2]
        for nothing in (np.zeros(n, bool), [], lib.allow_bitmap([], n)):
            kept = idx.remove(nothing)
            assert np.array_equal(kept, np.arange(n) + off) and idx.n == n == _pq_n(lib, idx)
        removed, zeros = C.c_int64(-1), np.zeros(4, np.uint64)
        lib.check(lib.load().mi_pq_remove_rows(idx._h, C.c_void_p(zeros.ctypes.data), lib.MI_HOST, C.byref(removed)))
        assert removed.value == 0
        assert np.array_equal(idx.get_codes(), codes) and _same(idx.search(q, n)[:2], before)


@pytest.mark.parametrize("kind", [False, True], ids=["plain", "residual"])
def test_ivf_entry_forms(lib, kind):
    import torch
    n, nlist, off = 300, 7, 1000
    G, Cb, codes, lists, q = _ivf_problem(70, n, nlist, 5, 16)
    gone = np.random.default_rng(71).random(n) < 0.4
    gone[[0, n - 1]] = True
    ids = np.flatnonzero(gone) + off
    want_kept = np.flatnonzero(~gone) + off
    make = lambda: lib.IVFPQIndex.from_codes(G, Cb, codes, lists, row_offset=off, by_residual=kind)  # noqa: E731
    with make() as idx:
        kept = idx.remove(np.concatenate([ids[::-1], ids[:5]]))
        assert np.array_equal(kept, want_kept)
        _check_ivf(lib, kind, idx, G, Cb, codes[~gone], lists[~gone], q, off, n, label="global ids")
        with pytest.raises(ValueError):
            idx.remove([off + n])
    words = np.asarray(lib.allow_bitmap(gone, n)).copy()
    with make() as idx:
        dev = _device_words(torch, words)
        removed = C.c_int64(-1)
        lib.check(lib.load().mi_ivfpq_remove_rows(idx._h, C.c_void_p(dev.data_ptr()), lib.MI_DEVICE, C.byref(removed)))
        assert removed.value == int(gone.sum())
        _check_ivf(lib, kind, idx, G, Cb, codes[~gone], lists[~gone], q, off, n, label="device bitmap")
    with make() as idx:
        beyond = words.copy()
        beyond[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n % 64)
        assert beyond[-1] != words[-1]
        kept = idx.remove(beyond.view(lib.AllowBits))
        assert np.array_equal(kept, want_kept)
        _check_ivf(lib, kind, idx, G, Cb, codes[~gone], lists[~gone], q, off, n, label="bits beyond n")
    with make() as idx:
        before = idx.search(q, n, nprobe=nlist)[:2]
        for nothing in (np.zeros(n, bool), [], lib.allow_bitmap([], n)):
            kept = idx.remove(nothing)
            assert np.array_equal(kept, np.arange(n) + off)
        idx._info()
        assert idx.n == n
        stored = idx.get_rows()
        assert np.array_equal(stored[0], codes) and np.array_equal(stored[1], lists)
        assert _same(idx.search(q, n, nprobe=nlist)[:2], before)


# ---- 6. the device search path after a removal

def _pq_device_search(torch, idx, q, k, stream):
    dev = torch.device("cuda", 0)
    nq = q.shape[0]
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    qd = torch.from_numpy(np.array(q, np.float32)).to(dev)
    torch.cuda.synchronize()
    idx.search_device(qd.data_ptr(), nq, k, out_i.data_ptr(), out_d.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_d.cpu().numpy()


def _ivf_device_search(torch, idx, q, k, nprobe, stream):
    dev = torch.device("cuda", 0)
    nq = q.shape[0]
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    qd = torch.from_numpy(np.array(q, np.float32)).to(dev)
    torch.cuda.synchronize()
    idx.search_device(qd.data_ptr(), nq, k, out_i.data_ptr(), out_d.data_ptr(), nprobe=nprobe, stream=stream.cuda_stream)
    stream.synchronize()
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_d.cpu().numpy()


def test_device_search_on_a_side_stream_after_a_removal(lib):
    import torch
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    n = 1000
    gone = np.random.default_rng(80).random(n) < 0.5
    Cb, codes, q = _pq_problem(81, n, 4, 16)
    with lib.PQIndex.from_codes(Cb, codes) as idx:
        idx.remove(gone)
        host = idx.search(q, 50)[:2]
        assert _same(_pq_device_search(torch, idx, q, 50, side), host)
        assert _same(host, pq_truth(q, Cb, codes[~gone], 50))
    for kind in (False, True):
        G, Cb, codes, lists, q = _ivf_problem(82, n, 7, 4, 16)
        with lib.IVFPQIndex.from_codes(G, Cb, codes, lists, by_residual=kind) as idx:
            idx.remove(gone)
            for nprobe in (1, 7):
                host = idx.search(q, 50, nprobe=nprobe)[:2]
                assert _same(_ivf_device_search(torch, idx, q, 50, nprobe, side), host), (kind, nprobe)
                assert _same(host, _ivf_truth(kind, q, G, Cb, codes[~gone], lists[~gone], probe_truth(q, G, nprobe), 50, 0))


# ---- 7. ANN

def test_ann_remove_ids(lib):
    from isehr_amd.knn import ANN
    rng = np.random.default_rng(90)
    N, nlist = 1300, 4
    centres = 3 * rng.standard_normal((nlist, 32))
    db = (centres[rng.integers(0, nlist, size=N)] + rng.standard_normal((N, 32))).astype(np.float32)
    q = db[rng.integers(0, N, size=5)] + 0.1 * rng.standard_normal((5, 32)).astype(np.float32)
    ann = ANN(db, "euclidean", M=4, nbits=8, nlist=nlist, nprobe=2)
    try:
        codes, lists = ann.index.get_rows()
        ids = rng.integers(0, N, size=400)
        ids[:3] = 0, N - 1, 0
        keep = np.ones(N, bool)
        keep[ids] = False
        assert ann.remove_ids(ids) == len(set(ids.tolist())) == N - keep.sum()
        assert ann.N == keep.sum() == ann.index.n
        after = ann.index.get_rows()
        assert np.array_equal(after[0], codes[keep]) and np.array_equal(after[1], lists[keep])
        dist, got = ann.search(q, 20)
        with lib.IVFPQIndex.from_codes(ann.index.coarse, ann.index.codebooks, after[0], after[1], by_residual=True) as rebuilt:
            want_ids, want_dist, _ = rebuilt.search(q.astype(np.float32), 20, nprobe=2)
        assert np.array_equal(got, want_ids) and np.array_equal(_bits(dist), _bits(want_dist))
        assert ann.remove_ids([]) == 0 and ann.N == keep.sum()
    finally:
        ann.close()
