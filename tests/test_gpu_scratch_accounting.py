"""Device scratch of the index handles: what `hbm_bytes` reports after every kind of call, and that a closed handle gives all
of it back.

The handles own their grow-only device buffers (csrc/device_buf.h); `hbm_bytes` is the sum of the buffers' own sizes.  The numbers
below were read from the library BEFORE the buffers owned themselves (hand-kept capacity fields and byte sums) and pin the
allocation sizes: a buffer that grows with other slack, is left out of the sum, or is counted twice changes them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, KS, NLIST, D = 8, 16, 4, 32          # PQ: 8 books of 16 codewords over 32 columns; 4 coarse lists
K = 10


def _parts(n, seed=11):
    rng = np.random.default_rng(seed)
    return {
        "n": n,
        "bcodes": rng.integers(0, 256, size=(n, 8), dtype=np.uint8),            # 64-bit binary codes
        "cb": rng.standard_normal((M, KS, D // M)).astype(np.float32),
        "coarse": rng.standard_normal((NLIST, D)).astype(np.float32),
        "codes": rng.integers(0, KS, size=(n, M), dtype=np.uint8),
        "lists": rng.integers(0, NLIST, size=n, dtype=np.uint8),
        "q": rng.standard_normal((70, D)).astype(np.float32),
        "allow": rng.random(n) < 0.5,
        "gone": rng.choice(n, size=100, replace=False).astype(np.int64),
    }


def _trace_binary(p, self_rows):
    """create, 3 queries, 70 queries under a host bitmap, radius search, self-join, 3 queries -> hbm_bytes after each.
    (A binary index has no row removal.)"""
    from isehr_amd._lib import BinaryGallery
    B = BinaryGallery.from_host(p["bcodes"])
    try:
        out = [B.hbm_bytes]
        B.search(p["bcodes"][:3], K)
        out.append(B.hbm_bytes)
        B.search(p["bcodes"][:70], K, allow=p["allow"])
        out.append(B.hbm_bytes)
        B.range_search(p["bcodes"][:70], 20)
        out.append(B.hbm_bytes)
        B.self_range(0, self_rows, 20)
        out.append(B.hbm_bytes)
        B.search(p["bcodes"][:3], K)
        out.append(B.hbm_bytes)
    finally:
        B.close()
    return out


def _trace_pq(p, kind):
    """create, 3 queries, 70 queries under a host bitmap, 100 rows removed, 3 queries -> hbm_bytes after each."""
    from isehr_amd._lib import IVFPQIndex, PQIndex
    if kind == "pq":
        X = PQIndex.from_codes(p["cb"], p["codes"])
        kw = {}
    else:
        X = IVFPQIndex.from_codes(p["coarse"], p["cb"], p["codes"], p["lists"], by_residual=(kind == "ivfpq_residual"))
        kw = {"nprobe": 2}
    try:
        out = [X.hbm_bytes]
        X.search(p["q"][:3], K, **kw)
        out.append(X.hbm_bytes)
        X.search(p["q"], K, allow=p["allow"], **kw)
        out.append(X.hbm_bytes)
        X.remove(p["gone"])
        out.append(X.hbm_bytes)
        X.search(p["q"][:3], K, **kw)
        out.append(X.hbm_bytes)
    finally:
        X.close()
    return out


def _trace(p, kind, self_rows=None):
    return _trace_binary(p, p["n"] if self_rows is None else self_rows) if kind == "binary" else _trace_pq(p, kind)


# n = 1000 rows; read on commit 09ca03e (the parent of the change that introduced DeviceBuf), one MI355X
EXPECTED = {
    "binary": [8192, 17590, 201180, 232124, 436168, 436168],
    "pq": [20560, 41320, 446924, 458400, 458400],
    "ivfpq": [38868, 44476, 117856, 118196, 118196],
    "ivfpq_residual": [38868, 46396, 162656, 162996, 162996],
}


@pytest.fixture(scope="module")
def small():
    return _parts(1000)


@pytest.fixture(scope="module")
def large():
    return _parts(200000)


@pytest.mark.parametrize("kind", sorted(EXPECTED))
def test_hbm_bytes_after_every_step(small, kind):
    got = _trace(small, kind)
    print("hbm_bytes", kind, got)
    assert all(b >= a for a, b in zip(got, got[1:])), got                # scratch only grows within a handle's life
    assert got[2] - got[1] >= (small["n"] + 63) // 64 * 8, got           # the first host bitmap has to go somewhere
    assert got == EXPECTED[kind]


def _free_after_cycles(cycle):
    import torch
    cycle()                                                  # first use: code objects, torch's own pools
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(12):
        cycle()
    torch.cuda.synchronize()
    return free0, torch.cuda.mem_get_info()[0]


@pytest.mark.parametrize("kind", sorted(EXPECTED))
def test_closed_index_returns_its_memory(large, kind):
    """n = 200 000: the Hamming and PQ distance matrices of 70 queries are tens of MiB, so one buffer missed by close() shows."""
    free0, free1 = _free_after_cycles(lambda: _trace(large, kind, self_rows=2000))
    print("free before / after 12 cycles", kind, free0, free1)
    assert free0 - free1 < 32 * 2**20, (free0, free1)


def test_closed_gallery_returns_its_scratch():
    """The gallery's own scratch: filtered search (both paths), squared-L2 search, re-ranking, range search, row removal."""
    from isehr_amd._lib import Gallery
    rng = np.random.default_rng(3)
    g = rng.standard_normal((40000, 128)).astype(np.float32)
    q = rng.standard_normal((70, 128)).astype(np.float32)
    wide, narrow = rng.random(40000) < 0.5, rng.random(40000) < 0.02
    cand = rng.integers(0, 40000, size=(70, 64)).astype(np.int64)
    gone = rng.choice(40000, size=100, replace=False).astype(np.int64)

    def cycle():
        G = Gallery.from_host(g)
        try:
            G.search_filtered(q, K, allow=wide)              # over-fetch
            G.search_filtered(q, K, allow=narrow)            # compacted sub-gallery
            G.refine(q, cand, K)
            G.range_search(q, 0.3)
            G.remove(gone)
            G.search(q[:3], K)
        finally:
            G.close()
        L = Gallery.l2_from_host(g[:20000])
        try:
            L.search_l2(q, K)
            L.search_l2(q, K, allow=wide[:20000])
        finally:
            L.close()

    free0, free1 = _free_after_cycles(cycle)
    print("free before / after 12 cycles gallery", free0, free1)
    assert free0 - free1 < 32 * 2**20, (free0, free1)
