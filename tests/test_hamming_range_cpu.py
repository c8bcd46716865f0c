"""CPU: the radius search and self-join of the binary index (mi_hamming_range_search*, mi_hamming_self_range) are exported and
bound and answer bad arguments before touching a device; the numpy truth agrees with a triple loop; and
dedup.near_duplicate_pairs_hamming batches, concatenates and checks as documented, against a fake index."""
import ctypes as C

import numpy as np
import pytest

from _hamming_range_truth import pairs_truth, range_truth

NEW = {"mi_hamming_range_search": 12, "mi_hamming_range_search_device": 10, "mi_hamming_self_range": 9}


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def test_symbols_are_exported_and_bound(built_lib):
    lib, _lib = built_lib
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        assert getattr(lib, name).restype == C.c_int
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    for meth in ("range_search", "range_search_device", "self_range"):
        assert hasattr(_lib.BinaryGallery, meth), meth
    assert hasattr(_lib.LSHIndex, "range_search")
    from isehr_amd import dedup
    assert callable(dedup.near_duplicate_pairs_hamming)
    assert _lib.get_global_option("hamming_range_bytes") == 1 << 30
    _lib.set_global_option("hamming_range_bytes", 4096)
    assert _lib.get_global_option("hamming_range_bytes") == 4096
    _lib.set_global_option("hamming_range_bytes", 0)
    assert _lib.get_global_option("hamming_range_bytes") == 1 << 30
    assert lib.mi_set_global_option(b"hamming_range_bytes", -1.0) == 1 and b"hamming_range_bytes" in lib.mi_last_error()
    default = _lib.get_global_option("hamming_range_early_exit")
    assert default in (0, 1)
    _lib.set_global_option("hamming_range_early_exit", 1 - default)
    assert _lib.get_global_option("hamming_range_early_exit") == 1 - default
    _lib.set_global_option("hamming_range_early_exit", default)
    assert lib.mi_set_global_option(b"hamming_range_early_exit", 2.0) == 1


def test_invalid_arguments_answer_without_a_device(built_lib):
    lib, _lib = built_lib
    q = np.zeros((2, 8), np.uint8)
    lims = np.full(3, -7, np.int64)
    idx = np.zeros(8, np.int64)
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    fake = C.c_void_p(16)                         # non-null, never dereferenced: these checks answer before the handle is read

    def host(h=fake, radius=1, nq=2, cap=8, lims_p=P(lims), idx_p=P(idx), memspace=0, bits=None):
        return lib.mi_hamming_range_search(h, P(q), nq, 8, radius, bits, memspace, cap, lims_p, idx_p, None, None)

    def dev(h=fake, radius=1, nq=2, cap=8, lims_p=P(lims), idx_p=P(idx)):
        return lib.mi_hamming_range_search_device(h, P(q), nq, radius, None, cap, lims_p, idx_p, None, None)

    def self_(h=fake, radius=1, row0=0, nrows=2, cap=8, lims_p=P(lims), idx_p=P(idx)):
        return lib.mi_hamming_self_range(h, row0, nrows, radius, cap, lims_p, idx_p, None, None)

    for fn in (host, dev, self_):
        for kwargs, word in [(dict(h=None), b"null handle"), (dict(radius=-1), b"radius must"), (dict(cap=-1), b"max_results"),
                             (dict(lims_p=None), b"out_lims"), (dict(idx_p=None), b"out_idx")]:
            assert fn(**kwargs) == _lib.MI_ERR_INVALID, (fn.__name__, kwargs)
            assert word in lib.mi_last_error(), (fn.__name__, kwargs, lib.mi_last_error())
    for fn in (host, dev):
        assert fn(nq=-1) == _lib.MI_ERR_INVALID and b"nq must" in lib.mi_last_error()
    assert host(bits=P(idx), memspace=5) == _lib.MI_ERR_INVALID and b"allow_memspace" in lib.mi_last_error()
    for kwargs in (dict(row0=-1), dict(nrows=-1)):
        assert self_(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert b"row range" in lib.mi_last_error()
    # nq == 0 is MI_OK, and the host form writes the one offset there is
    assert host(nq=0) == 0 and lims[0] == 0


def test_truth_against_a_triple_loop():
    rng = np.random.default_rng(3)
    g = rng.integers(0, 4, size=(9, 2), dtype=np.uint8)       # 16-bit codes with few set bits: many small distances and ties
    q = rng.integers(0, 4, size=(4, 2), dtype=np.uint8)
    allowed = np.ones(9, bool)
    allowed[[2, 5]] = False
    for radius in (0, 1, 2, 16):
        for allow in (None, allowed):
            hits = [[] for _ in q]
            for i in range(len(q)):
                for j in range(len(g)):
                    d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(q[i], g[j]))
                    if d <= radius and (allow is None or allow[j]):
                        hits[i].append((d, j + 100))
            lims, ids, dist = range_truth(g, q, radius, row_offset=100, allowed=allow)
            assert lims.dtype == np.int64 and ids.dtype == np.int64 and dist.dtype == np.int32
            assert lims.tolist() == np.concatenate([[0], np.cumsum([len(h) for h in hits])]).tolist()
            flat = [x for h in hits for x in sorted(h)]
            assert ids.tolist() == [j for _, j in flat] and dist.tolist() == [d for d, _ in flat]
        pi, pj, pd = pairs_truth(g, radius)
        want = []
        for i in range(len(g)):
            row = []
            for j in range(i + 1, len(g)):
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(g[i], g[j]))
                if d <= radius:
                    row.append((d, j))
            want += [(i, j, d) for d, j in sorted(row)]
        assert list(zip(pi.tolist(), pj.tolist(), pd.tolist())) == want
    assert len(pairs_truth(g, 16)[0]) == 36


class FakeBinary:
    """self_range of a BinaryGallery, computed by the truth helper; records its calls"""

    def __init__(self, codes, row_offset=0):
        self.codes, self.n, self.row_offset, self.calls = codes, codes.shape[0], row_offset, []

    def self_range(self, row0, nrows, radius, max_results=None):
        self.calls.append((row0, nrows, radius))
        i, j, d = pairs_truth(self.codes, radius)
        keep = (i >= row0) & (i < row0 + nrows)
        lims = np.concatenate([[0], np.cumsum(np.bincount(i[keep] - row0, minlength=nrows))]).astype(np.int64)
        return lims, j[keep], d[keep], 0.0


def test_near_duplicate_pairs_hamming_on_a_fake_index(built_lib):
    from isehr_amd.dedup import near_duplicate_pairs_hamming
    rng = np.random.default_rng(4)
    base = rng.integers(0, 256, size=(6, 4), dtype=np.uint8)
    codes = base[rng.integers(0, 6, size=50)]
    codes[7, 0] ^= 1
    codes[30, 3] ^= 0x81
    want = pairs_truth(codes, 2)
    assert len(want[0]) > 50 and set(want[2].tolist()) >= {0, 1, 2}
    for batch, ncalls in ((1, 50), (7, 8), (50, 1), (1000, 1)):
        fake = FakeBinary(codes)
        got = near_duplicate_pairs_hamming(fake, 2, batch=batch)
        assert [a.dtype for a in got] == [np.int64, np.int64, np.int32]
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), batch
        assert fake.calls == [(r, min(batch, 50 - r), 2) for r in range(0, 50, batch)] and len(fake.calls) == ncalls

    class FakeLSH:                                     # an LSHIndex is joined through its gallery
        gallery = FakeBinary(codes)
    got = near_duplicate_pairs_hamming(FakeLSH(), 2, batch=16)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError, match="row_offset 0"):
        near_duplicate_pairs_hamming(FakeBinary(codes, row_offset=5), 2)
    with pytest.raises(ValueError, match="batch"):
        near_duplicate_pairs_hamming(FakeBinary(codes), 2, batch=0)
    empty = near_duplicate_pairs_hamming(FakeBinary(codes[:0]), 2)
    assert [a.shape for a in empty] == [(0,)] * 3 and [a.dtype for a in empty] == [np.int64, np.int64, np.int32]
    one = near_duplicate_pairs_hamming(FakeBinary(codes[:1]), 2)
    assert [a.shape for a in one] == [(0,)] * 3
