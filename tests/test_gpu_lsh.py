"""GPU: LSH codes (csrc/lsh.hip, csrc/api_lsh.hip) and the LSH index against numpy float64.

Reference and the undecided-bit rule: p = x.astype(f64) @ R.T, s = |x| @ |R|.T.  A bit is DECIDED when
|p - t| > 2 (d + 2) 2^-53 s -- the kernel's summation bound plus numpy's own -- and every decided bit must equal p >= t.  Each
test first asserts, on the reference alone, that its inputs have no undecided bit at all, so every comparison below is ==
on whole code arrays.  The tie test uses sums that are exact in any order and needs no such rule."""
import functools

import numpy as np
import pytest

from _hamming_truth import hamming_truth

pytestmark = pytest.mark.gpu

# (n, d, nbits): n and nbits at 1, 127-130 and 257, d at 1, 16, 17 and 2048 -- the edges of the 128 x 128 tile and the 16-wide K chunk
SHAPES = [(300, 2048, 264), (129, 17, 136), (1, 1, 8), (127, 100, 4096), (257, 2048, 2048), (130, 16, 128)]
# the last two: 8 column blocks, the XCD-aware tile order of csrc/f64_tile.h, with every loader -- ragged last block, rows and K;
# then 8 full blocks
LAYOUT_SHAPES = SHAPES[:2] + [(130, 33, 1000), (129, 32, 1024)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=None)
def _rotation(d, nbits):
    from isehr_amd import _lib
    R = _lib.lsh_rotation(d, nbits)
    R.setflags(write=False)
    return R


@functools.lru_cache(maxsize=None)
def _rows(n, d, f64=False):
    x = np.random.default_rng(1000 * n + d).standard_normal((n, d))
    x = x if f64 else x.astype(np.float32)
    x.setflags(write=False)
    return x


def _truth(x, R, t=None):
    """-> packed codes uint8 [n, nbits / 8] of the float64 reference, after asserting that no bit is undecided"""
    d = x.shape[1]
    x64 = x.astype(np.float64)
    p, s = x64 @ R.T, np.abs(x64) @ np.abs(R).T
    tt = 0.0 if t is None else np.asarray(t, np.float64)[None, :]
    undecided = ~(np.abs(p - tt) > 2 * (d + 2) * 2.0 ** -53 * s)
    assert int(undecided.sum()) == 0, "the inputs of this test have %d undecided bits" % undecided.sum()
    return np.packbits(p >= tt, axis=1, bitorder="little")


def _encode_device(lib, x_t, R, t=None, out_stride=None, sentinel=0xA5):
    """x_t: a 2-D torch view on the device, any strides -> the whole output buffer uint8 [n, out_stride] as the kernel left it"""
    import torch
    n, d = x_t.shape
    nbits = R.shape[0]
    ors = nbits // 8 if out_stride is None else out_stride
    R_t = torch.from_numpy(np.array(R, dtype=np.float64)).cuda()
    t_t = None if t is None else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).cuda()
    out = torch.full((n, ors), sentinel, dtype=torch.uint8, device="cuda")
    lib.lsh_encode_device(x_t.data_ptr(), n, d, R_t.data_ptr(), nbits, out.data_ptr(), thr_ptr=None if t_t is None else t_t.data_ptr(),
                          dtype=lib.MI_F32 if x_t.dtype == torch.float32 else lib.MI_F64, row_stride=x_t.stride(0),
                          col_stride=x_t.stride(1), out_row_stride=ors, stream=torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


@pytest.mark.parametrize("n,d,nbits", SHAPES)
def test_shapes(lib, n, d, nbits):
    import torch
    x, R = _rows(n, d), _rotation(d, nbits)
    want = _truth(x, R)
    got = _encode_device(lib, torch.from_numpy(np.array(x)).cuda(), R)
    assert got.shape == (n, nbits // 8) and np.array_equal(got, want)
    assert np.array_equal(lib.lsh_encode(x, R), want)                     # host entry point


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("layout", ["rows", "padded_rows", "DN", "padded_out"])
@pytest.mark.parametrize("n,d,nbits", LAYOUT_SHAPES)
def test_layouts(lib, n, d, nbits, layout, f64):
    import torch
    x, R = _rows(n, d, f64), _rotation(d, nbits)
    want = _truth(x, R)
    nb = nbits // 8
    out_stride = None
    if layout == "padded_rows":                                         # row stride d + 5, NaN between the rows
        buf = torch.full((n, d + 5), float("nan"), dtype=torch.float64 if f64 else torch.float32, device="cuda")
        buf[:, :d] = torch.from_numpy(np.array(x)).cuda()
        x_t = buf[:, :d]
    elif layout == "DN":                                                # the reference's [D, N] matrix: row stride 1, column stride N
        x_t = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
        assert x_t.stride() == (1, n)
    else:
        x_t = torch.from_numpy(np.array(x)).cuda()
        if layout == "padded_out":
            out_stride = nb + 7
    got = _encode_device(lib, x_t, R, out_stride=out_stride)
    assert np.array_equal(got[:, :nb], want)
    assert (got[:, nb:] == 0xA5).all()                                  # bytes beyond nbits / 8 are not touched
    # the host entry point takes the same strides
    if layout == "DN":
        assert np.array_equal(lib.lsh_encode(np.ascontiguousarray(x.T).T, R), want)
    elif layout == "padded_rows":
        wide = np.full((n, d + 5), np.nan, x.dtype)
        wide[:, :d] = x
        assert np.array_equal(lib.lsh_encode(wide[:, :d], R), want)


@pytest.mark.parametrize("n,d,nbits", [SHAPES[0], SHAPES[1]])
def test_thresholds(lib, n, d, nbits):
    import torch
    x, R = _rows(n, d), _rotation(d, nbits)
    t = 0.5 * np.random.default_rng(nbits).standard_normal(nbits)
    want = _truth(x, R, t)
    assert not np.array_equal(want, _truth(x, R))                         # the thresholds matter
    assert np.array_equal(_encode_device(lib, torch.from_numpy(np.array(x)).cuda(), R, t), want)
    assert np.array_equal(lib.lsh_encode(x, R, t), want)


@pytest.mark.parametrize("f64", [False, True])
def test_exact_ties_give_one(lib, f64):
    """small-integer x, R in {-1, 0, 1}: every product and every partial sum is an integer far below 2^24, exact in any order"""
    import torch
    rng = np.random.default_rng(11)
    n, d, nbits = 130, 40, 136
    x = rng.integers(-3, 4, size=(n, d)).astype(np.float64 if f64 else np.float32)
    x[5] = 0.0                                                          # a zero row: every projection is 0
    x[6] = -0.0
    R = rng.integers(-1, 2, size=(nbits, d)).astype(np.float64)
    R[7] = 0.0                                                          # a zero direction: a tie with t = 0 for every row
    t = rng.integers(-4, 5, size=nbits).astype(np.float64)
    t[:40] = 0.0
    p = x.astype(np.float64) @ R.T
    for thr in (None, t):
        tt = 0.0 if thr is None else thr[None, :]
        ties = p == tt
        assert ties.sum() > 500 and (p > tt).sum() > 500 and (p < tt).sum() > 500
        want = np.packbits(p >= tt, axis=1, bitorder="little")
        got = _encode_device(lib, torch.from_numpy(x).cuda(), R, thr)
        assert np.array_equal(got, want)                                # no exclusions
        bits = np.unpackbits(got, axis=1, bitorder="little")
        assert (bits[ties] == 1).all()
        assert np.array_equal(lib.lsh_encode(x, R, thr), want)
    zero_t = np.unpackbits(_encode_device(lib, torch.from_numpy(x).cuda(), R), axis=1, bitorder="little")
    assert (zero_t[5] == 1).all() and (zero_t[6] == 1).all() and (zero_t[:, 7] == 1).all()


def test_nan_row_gives_a_zero_code(lib):
    import torch
    n, d, nbits = 129, 17, 136
    x, R = np.array(_rows(n, d)), _rotation(d, nbits)
    want = _truth(x, R)
    x[0], x[64], x[128] = np.nan, np.nan, np.nan
    want[[0, 64, 128]] = 0
    t = np.full(nbits, -1e300)                                          # even a threshold every finite sum clears
    want_t = np.full_like(want, 0xFF)
    want_t[[0, 64, 128]] = 0
    assert np.array_equal(_encode_device(lib, torch.from_numpy(x).cuda(), R), want)
    assert np.array_equal(_encode_device(lib, torch.from_numpy(x).cuda(), R, t), want_t)
    assert np.array_equal(lib.lsh_encode(x, R), want)


def test_host_chunks_equal_one_device_call(lib):
    """8321 float32 rows of 2048 columns are more than one 64 MiB block of the host entry point"""
    import torch
    n, d, nbits = 8192 + 129, 2048, 8
    x = _rows(n, d)
    R = np.random.default_rng(3).standard_normal((nbits, d))
    want = _truth(x, R)
    host = lib.lsh_encode(x, R)
    assert np.array_equal(host, want)
    assert np.array_equal(_encode_device(lib, torch.from_numpy(np.array(x)).cuda(), R), host)
    assert np.array_equal(lib.lsh_encode(x, R), host)                   # two calls, equal bytes


@pytest.mark.parametrize("d,nbits", [(100, 72), (17, 136)])
def test_append_in_pieces_and_capacity(lib, d, nbits):
    import torch
    pieces = [1, 63, 64, 129]
    n = sum(pieces)
    x, R = _rows(n + 1, d), _rotation(d, nbits)
    t = 0.25 * np.random.default_rng(d).standard_normal(nbits)
    want = _truth(x, R, t)
    assert np.array_equal(lib.lsh_encode(x, R, t), want)
    with lib.LSHIndex.empty(d, nbits, n, R=R, thresholds=t) as idx:
        r = 0
        for m in pieces:
            idx.add(x[r:r + m])
            r += m
            assert idx.n == r
        assert np.array_equal(idx.get_codes(), want[:n])
        assert np.array_equal(idx.encode(x), want)
        # one row more than the capacity holds: refused by the wrapper and by the library, the index stays as it was
        with pytest.raises(ValueError, match="capacity"):
            idx.add(x[n:])
        extra = torch.from_numpy(np.array(x[n:])).cuda()
        with pytest.raises(RuntimeError, match="capacity"):
            idx.add_device(extra.data_ptr(), 1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        n_lib = lib.C.c_int64()
        lib.check(lib.load().mi_hamming_info(idx.gallery._h, n_lib, None, None, None, None, None))
        assert idx.n == n_lib.value == n
        assert np.array_equal(idx.get_codes(), want[:n])


@functools.lru_cache(maxsize=None)
def _search_case(nbits):
    N, d, Q = 5000, 128, 130
    g, q = np.array(_rows(N, d)), np.array(_rows(Q, d))
    q[0], q[2] = g[N // 2], g[N - 1]                                    # distance 0 occurs
    R = _rotation(d, nbits)
    return g, q, R, _truth(g, R), _truth(q, R)


@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("nbits", [64, 256])
def test_index_search_end_to_end(lib, nbits, k):
    from isehr_amd.nnsearch import matching_LSH_hip
    g, q, R, gc, qc = _search_case(nbits)
    ids_t, dist_t, _ = hamming_truth(gc, qc, k)
    allowed = np.random.default_rng(nbits + k).random(g.shape[0]) < 0.3
    ids_a, dist_a, _ = hamming_truth(gc, qc, k, allowed=allowed)
    with lib.LSHIndex.from_host(g, nbits=nbits) as idx:               # R: lsh_rotation(d, nbits, 5), what _rotation returns
        assert idx.n == g.shape[0] and idx.hbm_bytes > 0
        assert np.array_equal(idx.get_codes(), gc)
        ids, dist, secs = idx.search(q, k)
        assert ids.dtype == np.int64 and dist.dtype == np.int32 and secs > 0.0
        assert np.array_equal(dist, dist_t) and np.array_equal(ids, ids_t)
        ids, dist, _ = idx.search(q, k, allow=allowed)
        assert np.array_equal(dist, dist_a) and np.array_equal(ids, ids_a)
    idx_m, tpq = matching_LSH_hip(k, g, q, nbits)
    assert idx_m.dtype == np.int64 and np.array_equal(idx_m, ids_t) and tpq > 0.0
