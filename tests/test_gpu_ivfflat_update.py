"""GPU: the in-place update of the IVF-Flat index (mi_ivfflat_sync, mi_ivfflat_remove_rows, IVFFlatIndex.sync / .remove; DESIGN.md
5.18).  The oracle is always a FRESH IVFFlatIndex.build(gallery, the same centroids) on the gallery as it stands after the update:
n, the list sizes, both list tables byte for byte, the probes and the answers of nprobe = 1 and nprobe = nlist; on top of it the
truth of tests/_ivfflat_truth.py over the updated lists and, on an L2 gallery with every list probed, Gallery.search_l2.  Lattice
data (integer-valued float32 in [-3, 3]): every float64 value is exact and the tie classes are large."""
import ctypes as C

import numpy as np
import pytest

import _ivfflat_truth as T
from _graph_truth import gallery_rows

pytestmark = pytest.mark.gpu

N0 = 2 * 2048 + 5                 # two full blocks of the list build and a ragged one
OFF = 70                          # row_offset of every gallery here: the ids of a removal are global
OUTSIDE = "removal was made outside the index"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


def _gallery(lib, rows, kind, capacity):
    """An appendable gallery of `rows`: squared-L2, or inner product on the rows as given."""
    if kind == "l2":
        return lib.Gallery.l2_from_host(rows, row_offset=OFF, capacity=capacity)
    g = lib.Gallery.empty(capacity, rows.shape[1], norm_mode=lib.NORM_NONE, row_offset=OFF)
    g.append(rows)
    return g


def _data(d, nlist, seed, n=N0, extra=2049):
    rng = np.random.default_rng(seed)
    return T.lattice(rng, (n + extra, d)), T.lattice(rng, (nlist, d)), T.lattice(rng, (5, d))


def _tables(f):
    off, lr = f.lists()
    return off.tobytes(), lr.tobytes(), f.list_sizes().tobytes(), f.n


def _assert_fresh(lib, g, f, cent, q, l2, want_rows=None, k=50):
    """f is, bit for bit, the index a fresh build makes on g as it stands; its answers are the truth's over its own lists."""
    nlist = len(cent)
    stored = gallery_rows(g)
    if want_rows is not None:
        assert g.n == len(want_rows) and stored.tobytes() == np.ascontiguousarray(want_rows).tobytes()
    with lib.IVFFlatIndex.build(g, cent) as w:
        assert f.n == w.n == g.n
        off, lr = f.lists()
        w_off, w_lr = w.lists()
        assert lr.shape == (g.n,) and off[-1] == g.n
        assert off.tobytes() == w_off.tobytes() and lr.tobytes() == w_lr.tobytes()
        assert np.array_equal(f.list_sizes(), w.list_sizes()) and np.array_equal(f.list_sizes(), np.diff(off))
        assert f.centroids().tobytes() == cent.tobytes()
        for nprobe in (1, nlist):
            probes = f.probe(q, nprobe)
            assert np.array_equal(probes, w.probe(q, nprobe)) and np.array_equal(probes, T.probe(q, cent, nprobe, l2))
            ids, v64, _, scanned = f.search(q, k, nprobe=nprobe, return_values64=True, return_scanned=True)
            w_ids, w_v64, _, w_scanned = w.search(q, k, nprobe=nprobe, return_values64=True, return_scanned=True)
            assert np.array_equal(ids, w_ids) and v64.tobytes() == w_v64.tobytes() and np.array_equal(scanned, w_scanned)
            t_ids, t_val, t_scanned = T.search(q, stored, probes, off, lr, nlist, k, l2, g.row_offset)
            assert np.array_equal(ids, t_ids) and v64.tobytes() == t_val.tobytes() and np.array_equal(scanned, t_scanned)
        if l2:                                                   # every list probed: the exhaustive search, bit for bit
            e_ids, _, e64, _, _ = g.search_l2(q, k)
            assert np.array_equal(ids, e_ids) and v64.tobytes() == e64.tobytes()
    return off, lr


@pytest.mark.parametrize("kind", ["l2", "ip"])
@pytest.mark.parametrize("nlist", [7, 300])
@pytest.mark.parametrize("d", [20, 64])
@pytest.mark.parametrize("m", [1, 255, 257, 2049])
def test_sync_after_an_append(lib, m, d, nlist, kind):
    rows, cent, q = _data(d, nlist, 1000 * d + nlist)
    l2 = kind == "l2"
    g = _gallery(lib, rows[:N0], kind, N0 + m)
    try:
        with lib.IVFFlatIndex.build(g, cent) as f:
            old_off, old_lr = f.lists()
            g.append(rows[N0:N0 + m])
            with pytest.raises(RuntimeError, match="gallery has been appended to"):
                f.search(q, 3)
            assert f.sync() == m and f.n == N0 + m
            off, lr = _assert_fresh(lib, g, f, cent, q, l2, rows[:N0 + m])
            for l in range(nlist):                               # the old run of every list, then its new rows, ascending
                run = lr[off[l]:off[l + 1]]
                olen = old_off[l + 1] - old_off[l]
                assert np.array_equal(run[:olen], old_lr[old_off[l]:old_off[l + 1]]) and (run[olen:] >= N0).all()
                assert (np.diff(run) > 0).all()
    finally:
        g.close()


def test_sync_costs_what_a_build_costs(lib):
    """Straight after a sync and after a removal the handle holds exactly what a fresh build holds (no search has grown a workspace)."""
    rows, cent, _ = _data(20, 7, 5)
    with lib.Gallery.l2_from_host(rows[:N0], capacity=N0 + 300) as g, lib.IVFFlatIndex.build(g, cent) as f:
        g.append(rows[N0:N0 + 300])
        assert f.sync() == 300
        with lib.IVFFlatIndex.build(g, cent) as w:
            assert f.hbm_bytes == w.hbm_bytes and f.hbm_bytes >= 4 * g.n
        assert f.remove(np.arange(OFF + 10, OFF + 1010)) == 1000
        with lib.IVFFlatIndex.build(g, cent) as w:
            assert f.hbm_bytes == w.hbm_bytes and f.hbm_bytes >= 4 * g.n


@pytest.mark.parametrize("kind", ["l2", "ip"])
def test_two_appends_one_sync_equal_a_sync_after_each(lib, kind):
    rows, cent, q = _data(20, 300, 11)
    g = _gallery(lib, rows[:N0], kind, N0 + 900)
    try:
        with lib.IVFFlatIndex.build(g, cent) as f1, lib.IVFFlatIndex.build(g, cent) as f2:
            g.append(rows[N0:N0 + 257])
            assert f1.sync() == 257
            g.append(rows[N0 + 257:N0 + 900])
            assert f1.sync() == 643 and f2.sync() == 900
            assert _tables(f1) == _tables(f2)
            _assert_fresh(lib, g, f1, cent, q, kind == "l2", rows[:N0 + 900])
    finally:
        g.close()


def test_sync_with_nothing_appended_changes_nothing(lib):
    rows, cent, q = _data(20, 7, 12)
    with lib.Gallery.l2_from_host(rows[:N0], capacity=N0 + 10) as g, lib.IVFFlatIndex.build(g, cent) as f:
        before, bytes_before = _tables(f), f.hbm_bytes
        added = C.c_int64(-7)
        lib.check(lib.load().mi_ivfflat_sync(f._h, C.byref(added)))
        assert added.value == 0
        assert f.sync() == 0 and _tables(f) == before and f.hbm_bytes == bytes_before
        lib.check(lib.load().mi_ivfflat_sync(f._h, None))                    # out_added may be NULL
        g.append(rows[N0:N0 + 3])
        lib.check(lib.load().mi_ivfflat_sync(f._h, None))
        f.n = g.n                                                            # (the binding's mirror: the C call went beside it)
        _assert_fresh(lib, g, f, cent, q, True, rows[:N0 + 3])


@pytest.mark.parametrize("kind", ["l2", "ip"])
def test_lists_that_change_kind(lib, kind):
    """Four centroids at corners of the lattice, rows next to their corner.  List 2 is empty before a sync and filled by it, list 1
    receives nothing, list 3 is emptied by a removal; empty lists survive both operations."""
    rng = np.random.default_rng(21)
    l2, d = kind == "l2", 4
    cent = np.array([[-3, -3, -3, -3], [3, 3, 3, 3], [3, -3, 3, -3], [-3, 3, -3, 3]], np.float32)

    def near(l, count):                                          # one step towards the centre in some columns: the corner stays the best
        return (cent[l] - np.sign(cent[l]) * rng.integers(0, 2, (count, d))).astype(np.float32)

    first = [(0, 300), (1, 200), (3, 150)]
    lid0 = rng.permutation(np.repeat([l for l, _ in first], [c for _, c in first]))
    base = np.stack([near(l, 1)[0] for l in lid0])
    lid1 = rng.permutation(np.repeat([2, 0], [100, 50]))
    more = np.stack([near(l, 1)[0] for l in lid1])
    q = T.lattice(rng, (5, d))
    g = _gallery(lib, base, kind, len(base) + len(more))
    try:
        with lib.IVFFlatIndex.build(g, cent) as f:
            assert f.list_sizes().tolist() == [300, 200, 0, 150] and np.array_equal(f.list_ids(), lid0)
            g.append(more)
            assert f.sync() == 150
            assert f.list_sizes().tolist() == [350, 200, 100, 150]
            assert np.array_equal(f.list_ids(), np.r_[lid0, lid1])
            _assert_fresh(lib, g, f, cent, q, l2, np.r_[base, more], k=20)
            gone = np.r_[lid0, lid1] == 3
            assert f.remove(gone) == 150 and g.n == 650 and f.n == 650
            assert f.list_sizes().tolist() == [350, 200, 100, 0]
            assert np.array_equal(f.list_ids(), np.r_[lid0, lid1][~gone])
            _assert_fresh(lib, g, f, cent, q, l2, np.r_[base, more][~gone], k=20)
            ids, _, _ = f.search(q, 3, probes=np.full((5, 1), 3, np.int32))       # the emptied list: no candidate
            assert (ids == -1).all()
    finally:
        g.close()


def _named(name, n, lid, rng):
    mask = np.zeros(n, bool)
    if name == "row0":
        mask[0] = True
    elif name == "last":
        mask[n - 1] = True
    elif name == "word_edge":
        mask[[63, 64, 65]] = True
    elif name == "whole_word":
        mask[128:192] = True
    elif name == "one_list":
        mask[lid == np.bincount(lid).argmax()] = True
    else:
        mask[rng.permutation(n)[:n // 2]] = True
    return mask


@pytest.mark.parametrize("kind", ["l2", "ip"])
@pytest.mark.parametrize("nlist", [7, 300])
@pytest.mark.parametrize("d", [20, 64])
@pytest.mark.parametrize("name", ["row0", "last", "word_edge", "whole_word", "one_list", "half"])
def test_remove(lib, name, d, nlist, kind):
    rows, cent, q = _data(d, nlist, 2000 * d + nlist, extra=0)
    l2 = kind == "l2"
    g = _gallery(lib, rows, kind, N0)
    try:
        with lib.IVFFlatIndex.build(g, cent) as f:
            lid = f.list_ids()
            mask = _named(name, N0, lid, np.random.default_rng(3))
            arg = np.flatnonzero(mask) + OFF if name == "word_edge" else mask            # global ids once, masks otherwise
            assert f.remove(arg) == mask.sum()
            assert g.n == N0 - mask.sum() == f.n
            _assert_fresh(lib, g, f, cent, q, l2, rows[~mask])
            assert np.array_equal(f.list_ids(), lid[~mask])
            if name == "one_list":
                assert f.list_sizes()[np.bincount(lid).argmax()] == 0
    finally:
        g.close()


def test_remove_nothing_everything_and_a_device_bitmap(lib):
    import torch
    rows, cent, q = _data(20, 7, 31, extra=0)
    with lib.Gallery.l2_from_host(rows, row_offset=OFF) as g, lib.IVFFlatIndex.build(g, cent) as f:
        before = _tables(f)
        want = f.search(q, 10, nprobe=3, return_values64=True)
        assert f.remove(np.zeros(N0, bool)) == 0 and f.remove(np.zeros(0, np.int64)) == 0
        assert _tables(f) == before and g.n == N0
        for everything in (np.ones(N0, bool), np.arange(OFF, OFF + N0)):
            with pytest.raises(RuntimeError, match="names every row"):
                f.remove(everything)
        assert _tables(f) == before and g.n == N0 and gallery_rows(g).tobytes() == rows.tobytes()
        got = f.search(q, 10, nprobe=3, return_values64=True)
        assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
        # bits at or beyond n are ignored: a last word that is all ones names the rows below n only
        words = np.zeros((N0 + 63) // 64, np.uint64)
        words[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
        some = np.random.default_rng(8).permutation(N0)[:700]
        mask = np.zeros(N0, bool)
        mask[N0 // 64 * 64:] = True
        mask[some] = True
        words |= np.asarray(lib.allow_bitmap(some + OFF, N0, OFF)).view(np.uint64)
        dev = torch.from_numpy(words.view(np.int64)).cuda()
        removed = C.c_int64(-7)
        lib.check(lib.load().mi_ivfflat_remove_rows(f._h, dev.data_ptr(), lib.MI_DEVICE, C.byref(removed)))
        assert removed.value == mask.sum()
        g.n = f.n = N0 - int(mask.sum())                                      # (the binding's mirrors: the C call went beside them)
        _assert_fresh(lib, g, f, cent, q, True, rows[~mask])
        one = torch.zeros((g.n + 63) // 64, dtype=torch.int64, device="cuda")
        one[0] = 1                                                            # row 0; out_removed may be NULL
        lib.check(lib.load().mi_ivfflat_remove_rows(f._h, one.data_ptr(), lib.MI_DEVICE, None))
        g.n = f.n = g.n - 1
        _assert_fresh(lib, g, f, cent, q, True, rows[~mask][1:])


@pytest.mark.parametrize("kind", ["l2", "ip"])
def test_append_sync_remove_append_sync(lib, kind):
    rows, cent, q = _data(64, 300, 41)
    l2 = kind == "l2"
    g = _gallery(lib, rows[:N0], kind, N0 + 2049)
    try:
        with lib.IVFFlatIndex.build(g, cent) as f:
            g.append(rows[N0:N0 + 1000])
            assert f.sync() == 1000
            mask = np.random.default_rng(42).random(N0 + 1000) < 0.3
            assert f.remove(mask) == mask.sum()
            f.search(q, 10, nprobe=300)                                       # (a search between two updates: its workspace stays)
            g.append(rows[N0 + 1000:])
            assert f.sync() == 1049
            now = np.r_[rows[:N0 + 1000][~mask], rows[N0 + 1000:]]
            _assert_fresh(lib, g, f, cent, q, l2, now)
    finally:
        g.close()


def test_a_removal_beside_the_index_is_seen_when_n_is_back(lib):
    """gallery.remove(r rows) then gallery.append(r rows): n is where it was, the row numbers under the lists are not."""
    rows, cent, q = _data(20, 7, 51, n=500, extra=10)
    with lib.Gallery.l2_from_host(rows[:500], row_offset=OFF, capacity=510) as g, lib.IVFFlatIndex.build(g, cent) as f:
        f.search(q, 3)
        g.remove(np.array([7, 9, 300]) + OFF)
        g.append(rows[500:503])
        assert g.n == 500 == f.n
        for call in (lambda: f.search(q, 3), lambda: f.probe(q, 2), f.sync, lambda: f.remove(np.array([OFF]))):
            with pytest.raises(RuntimeError, match=OUTSIDE):
                call()
        assert g.n == 500
        g.append(rows[503:505])                                               # ... and stays refused whatever n becomes
        for call in (lambda: f.search(q, 3), f.sync):
            with pytest.raises(RuntimeError, match=OUTSIDE):
                call()
        with lib.IVFFlatIndex.build(g, cent) as f2:                           # a new index is in step again, and can be kept so
            g.append(rows[505:510])
            assert f2.sync() == 5
            assert f2.remove(np.array([0, 1]) + OFF) == 2
            _assert_fresh(lib, g, f2, cent, q, True)
            with pytest.raises(RuntimeError, match=OUTSIDE):                  # the index that was left behind saw nothing of it
                f.sync()


def test_8192_lists_on_a_small_gallery(lib):
    """Most lists are empty; the LDS-sized edge of the histogram path of the list build, which the sync runs on the appended rows."""
    rows, cent, q = _data(20, 8192, 61, n=5000, extra=300)
    with lib.Gallery.l2_from_host(rows[:5000], row_offset=OFF, capacity=5300) as g, lib.IVFFlatIndex.build(g, cent) as f:
        assert (f.list_sizes() == 0).sum() > 4000
        g.append(rows[5000:])
        assert f.sync() == 300
        _assert_fresh(lib, g, f, cent, q[:2], True, rows)
        mask = np.random.default_rng(62).random(5300) < 0.2
        assert f.remove(mask) == mask.sum()
        _assert_fresh(lib, g, f, cent, q[:2], True, rows[~mask])
