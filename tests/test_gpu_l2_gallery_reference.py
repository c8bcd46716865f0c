"""GPU: the prepared sections of a squared-L2 gallery against a float64 reference, section by section.

An L2 gallery is a raw gallery with three hidden bias columns behind the user's ud columns (csrc/l2_metric.hip):
c1 + c2 + c3 = -1/2 ||g||^2 in the float32 rows and in the swizzled 16-bit image, zeros up to dp, and the rounding norms taken
again over the augmented row.  The choice of fp16 or bf16, the search margin and the certificate rest on those bits, and the
prepared-gallery file (header word metric = 1, d = ud + 3, the sections as they lie in memory) is how they are read back.
Every case builds a gallery, saves it, reads the file on the host (tests/_gallery_file.py, nothing from the library) and runs
check_all on EVERY row and element: the checks of tests/test_gpu_gallery_reference.py over the augmented row (image = 16-bit
rounding of every stored column, padding rows and columns, rounding norms within [1 + 8e-7, 1 + 1.2e-6], header gstat3 --
norm_bounds() stays refused on an L2 gallery --, padding stats, checksums) and check_l2_columns:

 a. split   c1 == round16(float32(B)), c2 == float32(B - c1), c3 == float32(B - c1 - c2) with B = (c1 + c2) + c3 in float64,
            and the image element at column ud decodes to exactly c1.
 b. value   |B - b_ref| <= 2 (ceil(ud / 64) + 6) 2^-53 |b_ref|, b_ref = -1/2 accurate_row_sums(x x) over the stored user columns
            (derivation in check_l2_columns; + 2^-150 where |b_ref| < 2^-97, see below).
 c. user    rows_f32[:, :ud] == float32(source) bit for bit.
 d. padding columns ud + 3 .. dp of rows and image are +0.

The id of a case names the ingest kernel its width reaches with the USER's ud columns written into dp = round_up(ud + 3, 64)
wide rows (launch_ingest in csrc/ingest.hip), which is not the width those kernels were written for: ud = 2048 gives dp = 2112,
so the FULL kernel leaves 64 columns to l2_bias_kernel; ud = 2046 flips the columns-per-thread choice; ud = 4094 is row-wise.

The bias of a tiny row.  The issue that asked for this module states B == b exactly.  That holds while the float64 ulp of b,
2^-52 |b|, is no finer than float32's subnormal grid 2^-149, i.e. for |b| >= 2^-97.  The row scaled by 1e-20 has
b ~ -1e-40: c1, c2, c3 are float32 subnormals, multiples of 2^-149, and cannot hold b; c3 rounds what is left to the grid, so
|B - b| <= 2^-150 there.  check_l2_columns adds exactly that term below |b_ref| = 2^-97 and nothing above it (from the number
format; the bound was written before any GPU run).

A zero row: b = -0.5 * 0.0 = -0.0, so c1 = -0.0 (image 0x8000), c2 = f32(-0.0 - -0.0) = +0.0, c3 = +0.0; all three stats +0.0.

A row of norm 1e20: b = -5e39 is beyond float32, c1 = -inf, c2 = f32(b - c1) = +inf, c3 = f32(b + inf - inf) = NaN in rows and
image, the three stats are NaN (each sum holds the square of c3) and stay outside gstat3 (rowstat_max_kernel skips rows with a
non-finite stat), every other row is what it is without that row.  The gallery is bf16: read from the code before any run, the
fp16 pass of mi_gallery_create_l2 clamps c1 to -65504, c2 = f32(b + 65504) is -inf, the row's f32 norm is inf, and
rowstat_img_overflow_kernel looked only at rows with a FINITE f32 norm -- so with every other row inside fp16's range the
gallery would have stayed fp16 with a row whose user columns (1e19, finite in float32) are inf in the image, against DESIGN 5.11
("fp16 while ... nothing overflows").  Fixed with this module: on an L2 gallery any row with a non-finite image norm sends the
create loop to bf16 (launch_rowstat_img_overflow, any_f32).  Its score is NaN, the selection reports FLAG_SHORT and search_sync answers from the
dense float64 path, which orders NaN last: search_l2 with k = n returns the row last with its finite direct-form distance.

No section check failed on the MI355X on any other case: widths, row counts, sources, appends at row bases 0, 1 and 4, removals
and the round trip hold bit for bit; the largest |B - b_ref| stayed inside bound b.  The module takes about 10 s (75 cases)."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gallery_file as gfile  # noqa: E402
from _gallery_file import NORM_NONE  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- source rows ------------------------------------------------------------------------------------------------------------
def l2_rows(data, seed, n, ud, dtype="f32"):
    """Gaussian rows scaled to norms in [1.2, 1.8] (about 1.5: the augmented norm sqrt(x + x^2 / 4), x = ||g||^2, stays below 2.5)."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((n, ud))
    g *= (rng.uniform(1.2, 1.8, n) / np.sqrt((g * g).sum(1)))[:, None]
    g = g.astype(np.float32)

    def scale_to(row, norm):
        g[row] = (g[row].astype(np.float64) * (norm / np.linalg.norm(g[row].astype(np.float64)))).astype(np.float32)
    if data.startswith("maxnorm"):
        scale_to(1, float(data[7:]))
    elif data == "norms300to420":                           # 1/2 ||g||^2 = 45 000 .. 88 200 straddles fp16's 65 504
        for r, nm in enumerate(np.linspace(300.0, 420.0, n)):
            scale_to(r, nm)
    elif data == "elem70000":
        g[2, min(5, ud - 1)] = 70000.0
    elif data == "special":
        g[7] = 0.0                                          # zero row
        g[8] = g[9]                                         # exact duplicate
        g[10] *= np.float32(1e-20)                          # bias ~ -1e-40: float32 subnormals
        scale_to(11, 1e20)                                  # bias -5e39: beyond float32
    else:
        assert data == "gauss", data
    return g.astype(np.float64) if dtype == "f64" else g


class Case:
    def __init__(self, kernel, entry, n, ud, dtype="f32", data="gauss", f16=1, want_f16=1, **kw):
        self.kernel, self.entry, self.n, self.ud, self.dtype, self.data, self.f16, self.want_f16 = kernel, entry, n, ud, dtype, data, f16, want_f16
        self.kw = kw
        extra = "".join("-%s%s" % (k, v) for k, v in sorted(kw.items()))
        self.id = "%s-%s-n%d-ud%d-%s-%s-%s%s" % (kernel, entry, n, ud, dtype, "fp16" if want_f16 else "bf16", data, extra)


G8, G16, FULL, ROWWISE, TRANSPOSE = "generic_8", "generic_16", "FULL_dp2112", "rowwise", "transpose+rows"
CASES = []
# widths where the hidden columns cross a boundary
for _ud, _k in ((1, G8), (7, G8), (61, G8), (62, G8), (64, G8), (100, G8), (125, G8), (2045, G8), (2046, G16), (2048, FULL),
                (2500, G16), (4093, G16)):
    CASES.append(Case(_k, "dev_rows", 257, _ud))
CASES += [Case(FULL, "dev_rows", 257, 2048, "f64"), Case(ROWWISE, "dev_rows", 40, 4094)]
# row counts
for _n in (1, 255, 257, 1027):
    CASES.append(Case(G8, "dev_rows", _n, 64, tag="rows"))
    CASES.append(Case(FULL, "dev_rows", _n, 2048, tag="rows"))
# sources
for _ud, _k in ((100, G8), (2048, FULL)):
    CASES += [
        Case(_k, "host_rows", 300, _ud),
        Case(TRANSPOSE, "host_cols", 300, _ud),             # [D, N]: at 2048 not the column kernel, dp != 2048
        Case(_k, "dev_rows_strided", 300, _ud),
        Case(_k, "dev_rows", 300, _ud, "f64", tag="src"),
        Case(_k, "host_rows", 300, _ud, "f64"),
    ]
for _hi in (0, 1):
    CASES.append(Case(FULL, "host_rows", 4500, 2048, host_ingest=_hi))
# image type: the augmented norm sqrt(x + x^2 / 4), x = ||g||^2, is 4 where x^2 + 4 x - 64 = 0, x = -2 + sqrt(68) = 6.2462,
# ||g|| = 2.4992: a largest row norm of 2.45 keeps fp16 (augmented 3.873), 2.55 takes bf16 (4.127)
for _ud, _k in ((100, G8), (2048, FULL)):
    CASES += [
        Case(_k, "host_rows", 300, _ud, data="maxnorm2.45", want_f16=1),
        Case(_k, "host_rows", 300, _ud, data="maxnorm2.55", want_f16=0),
        Case(_k, "dev_rows", 300, _ud, data="norms300to420", want_f16=0),
        Case(_k, "dev_rows", 300, _ud, data="elem70000", want_f16=0),
        Case(_k, "dev_rows", 300, _ud, f16=0, want_f16=0),
        Case(_k, "dev_rows", 300, _ud, data="special", want_f16=0),
        Case(_k, "dev_rows", 300, _ud, "f64", data="special", want_f16=0),
    ]
# appends (capacity > n at creation, hence bf16): row bases 0, 1 and 4 / a [D, N] block across row 256 / whitened rows
for _spare in (0, 300):
    for _ud, _k in ((100, G8), (2048, FULL)):
        CASES.append(Case(_k + "+noncoop", "append_device", 700, _ud, want_f16=0, spare_cap=_spare))
        CASES.append(Case(TRANSPOSE, "append_host_cols", 601, _ud, want_f16=0, spare_cap=_spare))
    CASES.append(Case("whiten+rows_double_generic_8", "append_whitened", 700, 72, want_f16=0, d_in=200, spare_cap=_spare))
    CASES.append(Case("whiten+rows_double_FULL", "append_whitened", 260, 2048, want_f16=0, d_in=2048, spare_cap=_spare))


def _empty(_lib, cap, ud):
    return _lib.Gallery.l2_from_host(None, capacity=cap, d=ud)


def _build(case, rows):
    import torch
    from isehr_amd import _lib
    n, ud = case.n, case.ud
    code = _lib.MI_F64 if case.dtype == "f64" else _lib.MI_F32
    stream = torch.cuda.current_stream().cuda_stream
    e = case.entry
    if e == "dev_rows":
        keep = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        return _lib.Gallery.l2_from_device_ptr(keep.data_ptr(), n, ud, dtype=code), keep
    if e == "dev_rows_strided":
        wide = np.full((n, ud + 24), 7.0, dtype=rows.dtype)              # the 24 columns between the rows must not be read
        wide[:, :ud] = rows
        keep = torch.from_numpy(wide).cuda()
        torch.cuda.synchronize()
        return _lib.Gallery.l2_from_device_ptr(keep.data_ptr(), n, ud, dtype=code, row_stride=ud + 24), keep
    if e == "host_rows":
        return _lib.Gallery.l2_from_host(rows), None
    if e == "host_cols":
        return _lib.Gallery.l2_from_host(np.ascontiguousarray(rows.T).T), None
    g = _empty(_lib, n + case.kw["spare_cap"], ud)
    keep = None
    try:
        if e == "append_device":
            keep = torch.from_numpy(rows).cuda()
            for r0, m in ((0, 1), (1, 3), (4, n - 4)):                   # l2_bias_kernel with row0 = 0, 1, 4 and no padding rows
                g.append_device(keep.data_ptr() + r0 * ud * 4, m, stream)
            torch.cuda.synchronize()
        elif e == "append_host_cols":
            a = np.ascontiguousarray(rows.T)                             # [D, N]
            g.append(a[:, :200].T)
            g.append(a[:, 200:].T)                                       # rows 200 .. 600: across row 256
        else:
            assert e == "append_whitened"
            keep = [torch.from_numpy(a).cuda() for a in rows]            # (x, mean, P)
            x, m, P = keep
            cut = 3 if ud < 2048 else 256
            g.append_whitened_device(x.data_ptr(), cut, case.kw["d_in"], m.data_ptr(), P.data_ptr(), stream=stream)
            g.append_whitened_device(x[cut:].data_ptr(), n - cut, case.kw["d_in"], m.data_ptr(), P.data_ptr(), stream=stream)
            torch.cuda.synchronize()
    except Exception:
        g.close()
        raise
    return g, keep


def _snapshot(g, path):
    g.save(path)
    f = gfile.read_gallery_file(path)
    f.raw = open(path, "rb").read()
    os.unlink(path)
    return f


def _snapshot_and_check(g, path, ref, want_f16, n, ud, whitened=False):
    assert (g.n, g.d) == (n, ud)
    f = _snapshot(g, path)
    d = ud + 3
    assert (f.metric, f.ud, f.n, f.npad, f.d, f.dp, f.norm_mode) == (1, ud, n, -(-n // 256) * 256, d, -(-d // 64) * 64, NORM_NONE)
    assert f.img_f16 == want_f16, "the header says %s" % ("fp16" if f.img_f16 else "bf16")
    gfile.check_all(f, ref=ref, get_rows=g.get_rows(0, n), whitened=whitened)
    return f


def _same_file(a, b, what):
    """Section for section and checksum for checksum."""
    assert (a.n, a.npad, a.d, a.dp, a.img_f16, a.metric) == (b.n, b.npad, b.d, b.dp, b.img_f16, b.metric), what
    for name in ("rows_f32", "rowstat", "gstat3"):
        x, y = np.ascontiguousarray(getattr(a, name)).view(np.uint32), np.ascontiguousarray(getattr(b, name)).view(np.uint32)
        assert np.array_equal(x, y), "%s: %s differs: %s" % (what, name, gfile._where(x != y))
    assert np.array_equal(a.image_flat, b.image_flat), "%s: image differs: %s" % (what, gfile._where(a.image_bits != b.image_bits))
    assert a.header_sums == b.header_sums and a.host_sums == b.host_sums, what


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_l2_gallery_matches_the_float64_reference(case, tmp_path):
    from isehr_amd import _lib
    n, ud = case.n, case.ud
    seed = 7000 + (n * 31 + ud * 7 + len(case.id)) % 997
    whitened = case.entry == "append_whitened"
    if whitened:
        rng = np.random.default_rng(seed)
        d_in = case.kw["d_in"]
        x = rng.standard_normal((n, d_in)).astype(np.float32)
        mean = x.mean(axis=0).astype(np.float64)
        P = rng.standard_normal((d_in, d_in)) / np.sqrt(d_in)
        rows = (x, mean, P)
        ref = (x.astype(np.float64) - mean) @ P[:ud].T
    else:
        rows = l2_rows(case.data, seed, n, ud, case.dtype)
        ref = rows.astype(np.float64)
    _lib.set_global_option("image_dtype", case.f16)
    if "host_ingest" in case.kw:
        _lib.set_global_option("host_ingest", case.kw["host_ingest"])
    g = keep = None
    try:
        g, keep = _build(case, rows)
        f = _snapshot_and_check(g, str(tmp_path / "g.bin"), ref, case.want_f16, n, ud, whitened)
        if case.data == "special":
            Q = np.concatenate([rows[:3], rows[20:22] * 0.5]).astype(np.float32)
            ids, dist, dist64, _, _ = g.search_l2(Q, n)
            dids, _, ddist64, _ = g.dense64_search_l2(Q, n)
    finally:
        _lib.set_global_option("image_dtype", 1)
        _lib.set_global_option("host_ingest", 1)
        if g is not None:
            g.close()
    del keep
    if case.data != "special":
        assert np.isfinite(f.rows_f32).all() and np.isfinite(f.rowstat).all()
        return
    u32 = lambda a: np.ascontiguousarray(a).view(np.uint32)      # noqa: E731
    # zero row: bias -0.0, +0.0, +0.0 (image 0x8000, 0, 0), stats +0.0
    assert u32(f.rows_f32[7, ud:ud + 3]).tolist() == [0x80000000, 0, 0] and not f.rows_f32[7].any()
    assert f.image_bits[7, ud:ud + 3].tolist() == [0x8000, 0, 0] and not f.image_bits[7, :ud].any()
    assert not u32(f.rowstat[7]).any()
    # exact duplicates: equal bits in all three sections
    assert np.array_equal(u32(f.rows_f32[8]), u32(f.rows_f32[9])) and np.array_equal(f.image_bits[8], f.image_bits[9])
    assert np.array_equal(u32(f.rowstat[8]), u32(f.rowstat[9]))
    # the tiny row: a finite, non-zero bias of float32 subnormals
    assert np.isfinite(f.rows_f32[10]).all() and f.rows_f32[10, ud] < 0 and abs(float(f.rows_f32[10, ud])) < 2.0 ** -126
    # the row of norm 1e20: non-finite hidden columns and stats, outside gstat3, every other row untouched
    c = f.rows_f32[11, ud:ud + 3]
    assert c[0] == -np.inf and c[1] == np.inf and np.isnan(c[2]) and np.isfinite(f.rows_f32[11, :ud]).all()
    assert f.image_bits[11, ud:ud + 2].tolist() == [0xFF80, 0x7F80] and gfile.is_nan16(f.image_bits[11, ud + 2], 0)
    assert np.isnan(f.rowstat[11]).all()
    others = np.setdiff1d(np.arange(n), [11])
    assert np.isfinite(f.rows_f32[others]).all() and np.isfinite(f.rowstat[others]).all() and np.isfinite(f.gstat3).all()
    assert np.array_equal(u32(f.gstat3), u32(f.rowstat[others].max(axis=0)))
    # ... and the search still returns it, last, with its finite direct-form distance
    X = f.rows_f32[:, :ud].astype(np.float64)
    diff = Q.astype(np.float64)[:, None, :] - X[None, :, :]
    truth = gfile.accurate_row_sums((diff * diff).reshape(-1, ud)).reshape(len(Q), n)
    assert (ids[:, -1] == 11).all() and (dids[:, -1] == 11).all(), (ids[:, -3:], dids[:, -3:])
    assert np.isfinite(dist64).all() and np.isinf(dist[:, -1]).all() and (dist64[:, -1] > 9e39).all()
    assert np.array_equal(np.sort(ids, 1), np.tile(np.arange(n), (len(Q), 1))) and np.array_equal(ids, dids)
    # (the tail sums per wave, the checker per 64 x 64 tile: each within the summation bound 2 ud 2^-53 of the float64 truth)
    for got_ids, got in ((ids, dist64), (dids, ddist64)):
        want = np.take_along_axis(truth, got_ids, 1)
        assert (np.abs(got - want) <= 2.0 * ud * 2.0 ** -53 * want).all(), float((np.abs(got - want) / np.maximum(want, 1e-300)).max())
    assert (np.diff(dist64, axis=1) >= 0).all() and (dist64[:3, 0] == 0).all()


def test_an_empty_appendable_l2_gallery_in_a_recycled_buffer(tmp_path):
    """Padding rows and stats where they are at risk: an inner-product gallery of 1300 x 2048 leaves its buffers in the spare slot,
    and an empty appendable L2 gallery of ud = 2045 (d = dp = 2048, the same three sizes) adopts them and fills 1000 rows.  The
    appends write image and stats of their own rows only, so rows 1000 .. 1023 are what mi_gallery_create_l2 left there."""
    import torch
    from isehr_amd import _lib
    from isehr_amd.synth import synth_rows
    cap, n, ud = 1300, 1000, 2045
    keep = torch.from_numpy(synth_rows(78, 0, cap, 2048)).cuda()
    torch.cuda.synchronize()
    _lib.Gallery.from_device_ptr(keep.data_ptr(), cap, 2048).close()
    rows = l2_rows("gauss", 79, n, ud)
    g = _empty(_lib, cap, ud)
    try:
        dev = torch.from_numpy(rows).cuda()
        g.append_device(dev.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _snapshot_and_check(g, str(tmp_path / "g.bin"), rows.astype(np.float64), 0, n, ud)
    finally:
        g.close()


# ---- removal: the file of a fresh gallery of the surviving source rows ------------------------------------------------------------
REMOVALS = ["every_third", "trailing", "whole_tile", "all_but_one", "remove_then_append"]


@pytest.mark.parametrize("kind", REMOVALS)
@pytest.mark.parametrize("n,ud", [(1000, 100), (700, 2048)])
def test_removal_leaves_the_file_of_a_fresh_gallery(n, ud, kind, tmp_path):
    """The contract at the top of csrc/api_remove.hip, for the hidden columns too: after a removal every section holds the bits
    the same ingest path would have written for the surviving source rows alone."""
    from isehr_amd import _lib
    X = l2_rows("gauss", 500 + n + ud, n, ud)
    extra = l2_rows("gauss", 501 + n + ud, 50, ud)
    gone = np.zeros(n, bool)
    if kind in ("every_third", "remove_then_append"):
        gone[::3] = True
    elif kind == "trailing":
        gone[n - 100:] = True                                # nothing moves; rows of the last tile are cleared where they lie
    elif kind == "whole_tile":
        gone[100:400] = True                                 # npad shrinks by a tile
    else:
        gone[:] = True
        gone[5] = False
    appendable = kind == "remove_then_append"
    g = _lib.Gallery.l2_from_host(X, capacity=n + 60 if appendable else 0)
    fresh = None
    try:
        kept = g.remove(gone)
        assert np.array_equal(kept, np.flatnonzero(~gone))
        want = X[kept]
        if appendable:
            g.append(extra)
            want = np.concatenate([want, extra])
        f = _snapshot_and_check(g, str(tmp_path / "a.bin"), want.astype(np.float64), 0 if appendable else 1, len(want), ud)
        fresh = _lib.Gallery.l2_from_host(want, capacity=len(want) + 1 if appendable else 0)
        _same_file(f, _snapshot(fresh, str(tmp_path / "b.bin")), kind)
    finally:
        g.close()
        if fresh is not None:
            fresh.close()


# ---- round trip -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ud,data,f16", [(1027, 100, "gauss", 1), (700, 2048, "gauss", 1), (300, 61, "norms300to420", 0)])
def test_round_trip(n, ud, data, f16, tmp_path):
    """save -> load -> save gives identical bytes, and the loaded gallery answers like the original, bit for bit."""
    import torch
    from isehr_amd import _lib
    X = l2_rows(data, 900 + ud, n, ud)
    Q = np.concatenate([l2_rows("gauss", 901 + ud, 17, ud), X[:3]])
    k, nq = 20, 20
    rng = np.random.default_rng(5)
    cand = rng.integers(-1, n, (nq, 64))
    cents = X[rng.choice(n, 8, replace=False)]
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")

    def answers(h):
        out = list(h.search_l2(Q, k)[:3]) + list(h.dense64_search_l2(Q, k)[:3]) + list(h.refine(Q, cand, 10)[:3])
        qd = torch.from_numpy(Q).cuda()
        idx = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        d32 = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        d64 = torch.empty((nq, k), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        h.search_l2_device(qd.data_ptr(), nq, k, idx.data_ptr(), d32.data_ptr(), d64.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert h.flags() == 0
        out += [idx.cpu().numpy(), d32.cpu().numpy(), d64.cpu().numpy()]
        ivf = _lib.IVFFlatIndex.build(h, cents)
        try:
            out += list(ivf.lists())
        finally:
            ivf.close()
        return out

    g = _lib.Gallery.l2_from_host(X)
    h = None
    try:
        g.save(a)
        f = gfile.read_gallery_file(a)
        assert (f.metric, f.ud, f.img_f16) == (1, ud, f16)
        h = _lib.Gallery.load(a)
        assert (h.n, h.d, h.norm_mode) == (n, ud, NORM_NONE) and h.get_option("metric") == 1
        assert np.array_equal(h.get_rows(0, n).view(np.uint32), X.view(np.uint32))
        h.save(b)
        assert open(a, "rb").read() == open(b, "rb").read()
        for i, (x, y) in enumerate(zip(answers(g), answers(h))):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), "answer %d differs" % i
        with pytest.raises(RuntimeError, match="MI_METRIC_L2"):
            h.norm_bounds()                                              # what is refused on an L2 gallery stays refused
        with pytest.raises(RuntimeError, match="capacity"):
            h.append(X[:1])                                              # loaded with cap = n
    finally:
        g.close()
        if h is not None:
            h.close()


# ---- loader refusals ------------------------------------------------------------------------------------------------------------
OFF_D, OFF_NORM, OFF_METRIC, OFF_HSUM = 40, 48, 68, 96
assert struct.calcsize("<8s4q4i3f") == OFF_METRIC and struct.calcsize("<8s4q4i3fI3Q") == OFF_HSUM == gfile.HEADER.size - 8


def _patch_header(raw, offset, value):
    raw = bytearray(raw)
    raw[offset:offset + 4] = struct.pack("<i", value)
    h = 0xcbf29ce484222325
    for byte in raw[:OFF_HSUM]:                                          # FNV-1a of the header (csrc/api_file.hip host_sum)
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    raw[OFF_HSUM:OFF_HSUM + 8] = struct.pack("<Q", h)
    return bytes(raw)


def test_loader_refusals(tmp_path):
    from isehr_amd import _lib
    p, q = str(tmp_path / "l2.bin"), str(tmp_path / "bad.bin")
    X = l2_rows("gauss", 3, 40, 5)
    g = _lib.Gallery.l2_from_host(X)
    try:
        g.save(p)
    finally:
        g.close()
    l2 = open(p, "rb").read()
    gi = _lib.Gallery.from_host(X[:, :3], norm_mode=NORM_NONE)           # d = 3: what an L2 file of ud = 0 would look like
    try:
        gi.save(p)
    finally:
        gi.close()
    ip3 = open(p, "rb").read()
    flipped = bytearray(l2)
    flipped[gfile.HEADER.size + (7 * 64 + 5) * 4 + 1] ^= 0x10             # row 7, column ud = 5: c1
    for name, raw, word in [("metric word 2", _patch_header(l2, OFF_METRIC, 2), "inconsistent header"),
                            ("metric 1 with norm_mode 1", _patch_header(l2, OFF_NORM, 1), "inconsistent header"),
                            ("metric 1 with d = 3", _patch_header(ip3, OFF_METRIC, 1), "inconsistent header"),
                            ("flipped byte in the hidden columns", bytes(flipped), "checksum mismatch in section: f32 rows")]:
        open(q, "wb").write(raw)
        with pytest.raises(RuntimeError, match=word):
            _lib.Gallery.load(q).close()
    for raw, metric in ((l2, 1), (ip3, 0)):                              # the unpatched files load
        open(q, "wb").write(raw)
        h = _lib.Gallery.load(q)
        try:
            assert h.get_option("metric") == metric
        finally:
            h.close()
