"""GPU: the prepared gallery against a float64 reference computed from the SOURCE rows, section by section.

tests/test_gpu_ingest_bits.py pins the gallery's bits to what an earlier kernel of this project produced (stability across
kernels and layouts); this module pins them to first principles (correctness).  Every case builds a gallery, saves it, reads the
file back on the host (tests/_gallery_file.py: the documented layout, nothing from the library) and asserts on EVERY row and
element:

 1. stored rows   rows_f32[:, :d] == float32(x / ||x||) (float64, compensated sum); the other float32 neighbour only where the
                  reference lies within 1e-5 ulp of a rounding tie (the kernel's (float)((double)x * (1.0 / nrm)) with a double sum of
                  at most 4096 squares is within (dp / 2 + 3) 2^-53 < 2.3e-13 relative = 4e-6 ulp); columns d..dp are +0.0;
                  get_rows() returns the same bits.  Whitened append: |stored - ref| <= 0.5 ulp_f32(ref) + 1e-12 (the f64 GEMM sums
                  in another order; 1e-12 is what the suite holds whitenapply to).
 2. image         bit-identical to the fp16 / bf16 rounding (header img_f16) of the STORED float32 value, NaN as NaN; rows n..npad
                  and columns d..dp are zero.
 3. rounding norms  a (1 + 8e-7) <= stat <= a (1 + 1.2e-6), a = float64 norm of the stored row / the decoded image row / their
                  difference (the kernel stores (float)(sqrt(s) (1 + 1e-6)): one float32 rounding <= 6e-8, the double sum < 1e-12);
                  below a = 2^-100, |stat - a| <= 2^-149 + 1.2e-6 a; 0 where a == 0.
 4. maxima        header gstat3 and norm_bounds() == max over the rows < n whose three stats are finite, bit for bit.
 5. padding stats RowStat of rows n..npad == (0, 0, 0).
 6. checksums     the section sums recomputed on the host equal the header's.
 7. zero rows     NORM_L2: NaN row, NaN image, NaN stats; NORM_L2_EPS: zeros and zero stats; outside gstat3 either way.

The id of every case names the ingest kernel its shape and source reach (launch_ingest / ingest_takes_layout in csrc/ingest.hip,
ingest_rows_any_layout / gallery_ingest_host_blocks in csrc/api_gallery.hip).  ingest_query_kernel<T, false, PT> sits behind the
same condition as the wave-per-row kernels and is unreachable in a shipped library; the query side (ingest_query_kernel<T, true, PT>,
the per-query margin) is not visible through the C ABI.

Tiny norms (3, a < 2^-100): the `tinyraw` cases hold raw rows whose norms run from 1e-36 down to 2^-149.  stat >= a does NOT
hold there: on the MI355X the stored norm was below the float64 norm in 20 of 66 (fp16 case) and 28 of 87 (bf16 case) tiny
norms, by at most 6.97e-46 < 2^-150 -- round-to-nearest of a subnormal float32, whose spacing exceeds the 1e-6 head-room.  The
bound |stat - a| <= 2^-149 + 1.2e-6 a holds for all of them; the margin's + 1e-30f is what covers the shortfall.

Padding stats of appended galleries (5): FAILED before the fix that comes with this module, on all eleven append cases that ran
(blocks_odd, append_device, append_host; e.g. ...append_device-n1000-d2048-f32-l2-fp16-gauss-spare_cap0: 72 non-zero words in
RowStat[1000..1024), values of earlier galleries or arbitrary device memory).  mi_gallery_create_empty cleared the image and
gstat3 but not RowStat[round_up(capacity, 256)], and the append paths write the stats of the appended rows only (launch_ingest
with npad = m), while rows n..npad are saved and checksummed.  mi_gallery_create_empty now clears the stat buffer too;
test_padding_stats_of_an_appended_gallery_in_a_recycled_buffer makes the stale content deterministic (spare slot).

Raw galleries (image type): ...host_rows-n300-d2048-f32-none-fp16-elem70000 FAILED before its fix: the header said fp16 and the
image held an inf, because the maxima that decide the type skip rows with a non-finite norm.  mi_gallery_create now looks for
a row with a finite f32 norm and a non-finite image norm (rowstat_img_overflow_kernel) and re-ingests as bf16.

The module takes about 25 s on one MI355X (98 cases; most of it the host-side reference and the file round trip)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gallery_file as gfile  # noqa: E402
from _gallery_file import NORM_L2, NORM_L2_EPS, NORM_NONE  # noqa: E402

pytestmark = pytest.mark.gpu

NORM_NAME = {NORM_NONE: "none", NORM_L2: "l2", NORM_L2_EPS: "l2eps"}


# ---- source rows ------------------------------------------------------------------------------------------------------------
def source_rows(data, seed, n, d, dtype):
    from isehr_amd.synth import synth_rows
    g = synth_rows(seed, 0, n, d)
    if data == "special":                                  # the special rows of scripts/make_ingest_checksums.py case_rows
        g[7] = 0.0                                         # zero row
        g[8] = g[9]                                        # exact duplicate
        g[10] *= 1e-20                                     # tiny row
        g[11] *= 1e18                                      # huge row
        g[12, ::2] = 0.0
        g[13] = -g[13]
    elif data == "nonneg":
        g = np.abs(g)
    elif data == "fp16exact":                              # small integers / 1024: exact in fp16 (and in bf16: |k| <= 8 has 4 bits)
        g = (np.random.default_rng(seed).integers(-8, 9, (n, d)) / 1024.0).astype(np.float32)
    elif data == "single":
        g[n // 2] = 0.0
        g[n // 2, d // 3] = -2.5                           # one non-zero element: the normalised row is exactly -1
    elif data.startswith("maxnorm"):                       # raw rows: unit rows, row 1 scaled to the given norm
        g = (g / np.linalg.norm(g.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        g[1] *= np.float32(float(data[7:]))
    elif data == "elem70000":
        g = (g / np.linalg.norm(g.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        g[2, 5] = 70000.0                                  # beyond fp16's range: inf in an fp16 image
    elif data == "tinyraw":                                # raw rows whose norms run from 1e-36 down through float32's subnormals
        g = (g / np.linalg.norm(g.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        for i in range(3, 43):
            g[i] = (g[i].astype(np.float64) * 10.0 ** (-36.0 - (i - 3) / 4.0)).astype(np.float32)
        g[43] = 0.0
        g[43, 1] = 2.0 ** -149                             # the smallest float32
    else:
        assert data == "gauss", data
    return g.astype(np.float64) if dtype == "f64" else g


# ---- one case ---------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, kernel, entry, n, d, dtype="f32", norm=NORM_L2, data="gauss", f16=1, want_f16=None, **kw):
        self.kernel, self.entry, self.n, self.d, self.dtype, self.norm, self.data, self.f16 = kernel, entry, n, d, dtype, norm, data, f16
        self.want_f16 = f16 if want_f16 is None else want_f16
        self.kw = kw
        extra = "".join("-%s%s" % (k, v) for k, v in sorted(kw.items()))
        self.id = "%s-%s-n%d-d%d-%s-%s-%s-%s%s" % (kernel, entry, n, d, dtype, NORM_NAME[norm], "fp16" if f16 else "bf16", data, extra)


ROWS_FULL_F32 = "rows_kernel_float_8_PREFETCH_FULL"
ROWS_FULL_F64 = "rows_kernel_double_8_FULL"
ROWS_8 = "rows_kernel_generic_8"
ROWS_16 = "rows_kernel_generic_16"
ROWWISE = "rowwise_kernel"
COLS = "cols_kernel_coop"
TRANSPOSE = "transpose_rows_kernel+rows_kernel"

CASES = []
# ingest_rows_kernel<float, 8, PREFETCH, FULL> / <double, 8, false, FULL>: d == 2048, 16-byte aligned rows, row_base % 4 == 0
for _n in (1, 255, 257, 1027):
    CASES.append(Case(ROWS_FULL_F32, "dev_rows", _n, 2048))
    CASES.append(Case(ROWS_FULL_F64, "dev_rows", _n, 2048, "f64"))
CASES += [
    Case(ROWS_FULL_F32, "dev_rows", 1027, 2048, f16=0),
    Case(ROWS_FULL_F64, "dev_rows", 257, 2048, "f64", f16=0),
    Case(ROWS_FULL_F32, "dev_rows_strided", 257, 2048),                  # [N, d + 24] view: 8288-byte rows, still 16-byte aligned
    Case(ROWS_FULL_F32, "dev_rows", 300, 2048, data="special"),
    Case(ROWS_FULL_F64, "dev_rows", 300, 2048, "f64", data="special"),
    Case(ROWS_FULL_F32, "dev_rows", 300, 2048, norm=NORM_L2_EPS, data="special"),
    Case(ROWS_FULL_F32, "dev_rows", 300, 2048, data="special", f16=0),
    Case(ROWS_FULL_F32, "dev_rows", 300, 2048, data="nonneg"),
    Case(ROWS_FULL_F32, "dev_rows", 300, 2048, data="single"),
    Case(ROWS_FULL_F32, "dev_rows", 300, 2048, norm=NORM_NONE, data="fp16exact"),
]
# generic <T, 8> (dp <= 2048 without FULL's conditions): vec_ok 16-byte loads or element loads
for _d in (1, 7, 64, 100, 2044):
    CASES.append(Case(ROWS_8, "dev_rows", 257, _d))
    CASES.append(Case(ROWS_8, "dev_rows", 130, _d, "f64"))
CASES += [
    Case(ROWS_8, "dev_rows_off4", 257, 2048),                            # pointer offset by 4 bytes: vec_ok == 0
    Case(ROWS_8, "dev_rows_strided", 257, 100),                          # 496-byte rows: vec_ok
    Case(ROWS_8, "dev_rows_strided", 257, 7),                            # element loads
    Case(ROWS_8, "dev_rows_strided", 130, 100, "f64"),
    Case(ROWS_8, "dev_rows", 300, 100, f16=0),
    Case(ROWS_8, "dev_rows", 300, 512, data="special"),
    Case(ROWS_8, "dev_rows", 300, 512, "f64", norm=NORM_L2_EPS, data="special"),
    Case(ROWS_8, "dev_rows", 300, 100, data="single"),
    Case(ROWS_8, "dev_rows", 300, 100, norm=NORM_NONE, data="fp16exact"),
    Case(ROWS_8, "dev_rows", 300, 100, data="nonneg", f16=0),
]
# generic <T, 16> (2048 < dp <= 4096)
for _d in (2050, 2500, 4096):
    CASES.append(Case(ROWS_16, "dev_rows", 257, _d))
CASES += [
    Case(ROWS_16, "dev_rows", 130, 4096, "f64"),
    Case(ROWS_16, "dev_rows", 130, 2500, "f64", norm=NORM_L2_EPS),
    Case(ROWS_16, "dev_rows", 257, 2500, f16=0),
    Case(ROWS_16, "dev_rows", 300, 2500, data="special"),
]
# ingest_rowwise_kernel: dp > 4096 in any layout; [D, N] at d == 2048 with fewer than 16 rows (strides (1, n))
CASES += [
    Case(ROWWISE, "dev_rows", 40, 4100),
    Case(ROWWISE, "dev_cols", 40, 4100),
    Case(ROWWISE, "dev_rows", 40, 4100, "f64", data="special"),
    Case(ROWWISE, "dev_cols", 15, 2048),
    Case(ROWWISE, "host_cols", 15, 2048, "f64"),
]
# ingest_cols_kernel<T, true>: d == 2048 in the [D, N] layout, n >= 16 (panels of 16 float32 / 8 float64 rows)
for _n in (16, 17, 1000):
    for _dt in ("f32", "f64"):
        CASES.append(Case(COLS, "dev_cols", _n, 2048, _dt))
        CASES.append(Case(COLS, "host_cols", _n, 2048, _dt))
CASES += [
    Case(COLS, "dev_cols", 300, 2048, data="special"),
    Case(COLS, "dev_cols", 300, 2048, "f64", norm=NORM_L2_EPS, data="special"),
    Case(COLS, "dev_cols", 1000, 2048, f16=0),
]
# [D, N] at another width: launch_transpose_rows into a row-major scratch block, then the rows kernel
CASES += [
    Case(TRANSPOSE, "dev_cols", 300, 100),
    Case(TRANSPOSE, "dev_cols", 300, 2500),
    Case(TRANSPOSE, "dev_cols", 130, 64, "f64"),
    Case(TRANSPOSE, "host_cols", 300, 100),
]
# host block pipeline (gallery_ingest_host_blocks: 4096-row blocks at d = 2048 float32) and the staged path (host_ingest 0)
for _hi in (0, 1):
    CASES.append(Case(ROWS_FULL_F32, "host_rows", 4500, 2048, host_ingest=_hi))
    CASES.append(Case(COLS, "host_cols", 4500, 2048, host_ingest=_hi))
    CASES.append(Case(ROWS_8, "host_rows_strided", 300, 100, host_ingest=_hi))
CASES += [
    Case(ROWS_FULL_F64, "host_rows", 2500, 2048, "f64"),
    # from_blocks with an odd first block: the second append starts at a row that is no multiple of 4 (coop == 0)
    Case("cols_kernel_coop+cols_kernel_noncoop", "blocks_odd", 1000, 2048),
    Case("cols_kernel_coop+cols_kernel_noncoop", "blocks_odd", 700, 2048, "f64"),
    Case(TRANSPOSE + "_noncoop", "blocks_odd", 700, 100),
]
# append: Gallery.empty + append_device in pieces of 1, 3 and the rest (row_base 0, 1 and 4: coop, non-coop, coop)
CASES += [
    Case("rows_FULL+generic_8_noncoop+FULL", "append_device", 1000, 2048, spare_cap=0),
    Case("rows_FULL+generic_8_noncoop+FULL", "append_device", 1000, 2048, spare_cap=300),     # allocated tiles stay unused
    Case("rows_FULL+generic_8_noncoop+FULL", "append_device", 1000, 2048, data="special", f16=0, spare_cap=300),
    Case(ROWS_8, "append_device", 700, 100, spare_cap=300),
    Case(ROWS_16, "append_device", 300, 2500, spare_cap=0),
    Case(ROWS_FULL_F64 + "+generic_8_noncoop", "append_host", 601, 2048, "f64", spare_cap=300),
    Case(ROWS_8, "append_host", 601, 100, "f64", norm=NORM_L2_EPS, spare_cap=0),
    Case("whiten+rows_kernel_double_generic_8", "append_whitened", 1000, 72, norm=NORM_L2_EPS, d_in=200, spare_cap=300),
    Case("whiten+" + ROWS_FULL_F64, "append_whitened", 260, 2048, norm=NORM_L2_EPS, d_in=2048, spare_cap=0),
]
# raw rows pick their image type from the measured norms (mi_gallery_create: fp16 while max ||g|| <= 4 and the image is finite)
CASES += [
    Case(ROWS_FULL_F32, "host_rows", 300, 2048, norm=NORM_NONE, data="maxnorm3.9", want_f16=1),
    Case(ROWS_FULL_F32, "host_rows", 300, 2048, norm=NORM_NONE, data="maxnorm4.1", want_f16=0),
    Case(ROWS_FULL_F32, "host_rows", 300, 2048, norm=NORM_NONE, data="elem70000", want_f16=0),
    Case(ROWS_8, "dev_rows", 300, 100, norm=NORM_NONE, data="elem70000", want_f16=0),
    Case(ROWS_FULL_F32, "dev_rows", 300, 2048, norm=NORM_NONE, data="tinyraw"),
    Case(ROWS_8, "dev_rows", 300, 100, norm=NORM_NONE, data="tinyraw", f16=0),
]


def _build(case, rows):
    """-> (gallery, float64 reference rows or None, whitened?, objects to keep alive)"""
    import torch
    from isehr_amd import _lib
    n, d = case.n, case.d
    code = _lib.MI_F64 if case.dtype == "f64" else _lib.MI_F32
    stream = torch.cuda.current_stream().cuda_stream
    e = case.entry
    if e == "dev_rows":
        keep = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        return _lib.Gallery.from_device_ptr(keep.data_ptr(), n, d, norm_mode=case.norm, dtype=code), keep
    if e == "dev_rows_off4":
        assert rows.dtype == np.float32
        keep = torch.zeros(n * d + 1, dtype=torch.float32, device="cuda")
        keep[1:].copy_(torch.from_numpy(rows.reshape(-1)))
        torch.cuda.synchronize()
        assert (keep.data_ptr() + 4) % 16 == 4
        return _lib.Gallery.from_device_ptr(keep.data_ptr() + 4, n, d, norm_mode=case.norm, dtype=code), keep
    if e in ("dev_rows_strided", "host_rows_strided"):
        wide = np.full((n, d + 24), 7.0, dtype=rows.dtype)            # the 24 columns between the rows must not be read
        wide[:, :d] = rows
        if e == "host_rows_strided":
            return _lib.Gallery.from_host(wide[:, :d], norm_mode=case.norm), wide
        keep = torch.from_numpy(wide).cuda()
        torch.cuda.synchronize()
        return _lib.Gallery.from_device_ptr(keep.data_ptr(), n, d, norm_mode=case.norm, dtype=code, row_stride=d + 24), keep
    if e == "dev_cols":
        keep = torch.from_numpy(np.ascontiguousarray(rows.T)).cuda()   # [D, N] on the device
        torch.cuda.synchronize()
        return _lib.Gallery.from_device_ptr(keep.data_ptr(), n, d, norm_mode=case.norm, dtype=code, row_stride=1, col_stride=n), keep
    if e == "host_rows":
        return _lib.Gallery.from_host(rows, norm_mode=case.norm), None
    if e == "host_cols":
        return _lib.Gallery.from_host(np.ascontiguousarray(rows.T).T, norm_mode=case.norm), None
    if e == "blocks_odd":
        a = np.ascontiguousarray(rows.T)
        c1 = (n // 3) | 1
        return _lib.Gallery.from_blocks([a[:, :c1], a[:, c1:]], norm_mode=case.norm, chunk_rows=999), None
    cap = n + case.kw["spare_cap"]
    g = _lib.Gallery.empty(cap, d, norm_mode=case.norm)
    try:
        if e == "append_device":
            keep = torch.from_numpy(rows).cuda()
            for r0, m in ((0, 1), (1, 3), (4, n - 4)):
                g.append_device(keep.data_ptr() + r0 * d * 4, m, stream)
            torch.cuda.synchronize()
        elif e == "append_host":
            g.append(rows[:5])                                          # row_base 0: coop; then row_base 5: non-coop
            g.append(rows[5:])
            keep = None
        else:
            assert e == "append_whitened"
            keep = [torch.from_numpy(a).cuda() for a in rows]           # (x, mean, P)
            x, m, P = keep
            cut = 3 if d < 2048 else 256
            g.append_whitened_device(x.data_ptr(), cut, case.kw["d_in"], m.data_ptr(), P.data_ptr(), stream=stream)
            g.append_whitened_device(x[cut:].data_ptr(), n - cut, case.kw["d_in"], m.data_ptr(), P.data_ptr(), stream=stream)
            torch.cuda.synchronize()
    except Exception:
        g.close()
        raise
    return g, keep


def _snapshot_and_check(g, path, ref, want_f16, n, d, norm, whitened=False):
    g.save(path)
    got_rows, bounds = g.get_rows(0, n), g.norm_bounds()
    f = gfile.read_gallery_file(path)
    os.unlink(path)
    assert (f.n, f.npad, f.d, f.dp, f.norm_mode, f.img_f16) == (n, -(-n // 256) * 256, d, -(-d // 64) * 64, norm, want_f16)
    gfile.check_all(f, ref=ref, get_rows=got_rows, norm_bounds=bounds, whitened=whitened)
    return f


def _check_zero_rows(f, zero_rows, norm):
    """7: all-zero source rows."""
    for r in zero_rows:
        if norm == NORM_L2:
            assert np.isnan(f.rows_f32[r, :f.d]).all() and not f.rows_f32[r, f.d:].view(np.uint32).any(), r
            assert gfile.is_nan16(f.image_bits[r, :f.d], f.img_f16).all() and not f.image_bits[r, f.d:].any(), r
            assert np.isnan(f.rowstat[r]).all(), r
        else:
            assert not f.rows_f32[r].view(np.uint32).any() and not f.image_bits[r].any(), r
            assert not f.rowstat[r].view(np.uint32).any(), r
    assert np.isfinite(f.gstat3).all()
    others = np.setdiff1d(np.arange(f.n), zero_rows)
    assert np.isfinite(f.rows_f32[others]).all() and np.isfinite(f.rowstat[others]).all()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gallery_matches_the_float64_reference(case, tmp_path):
    from isehr_amd import _lib
    n, d = case.n, case.d
    seed = 9000 + (n * 31 + d * 7 + len(case.id)) % 997
    whitened = case.entry == "append_whitened"
    if whitened:
        rng = np.random.default_rng(seed)
        d_in = case.kw["d_in"]
        x = rng.standard_normal((n, d_in)).astype(np.float32)
        mean = x.mean(axis=0).astype(np.float64)
        P = rng.standard_normal((d_in, d_in)) / np.sqrt(d_in)
        rows = (x, mean, P)
        ref = gfile.reference_rows((x.astype(np.float64) - mean) @ P[:d].T, case.norm)
        zero_rows = []
    else:
        rows = source_rows(case.data, seed, n, d, case.dtype)
        ref = gfile.reference_rows(rows, case.norm)
        zero_rows = np.nonzero(~rows.any(axis=1))[0]
    _lib.set_global_option("image_dtype", case.f16)
    if "host_ingest" in case.kw:
        _lib.set_global_option("host_ingest", case.kw["host_ingest"])
    g = keep = None
    try:
        g, keep = _build(case, rows)
        f = _snapshot_and_check(g, str(tmp_path / "g.bin"), ref, case.want_f16, n, d, case.norm, whitened)
    finally:
        _lib.set_global_option("image_dtype", 1)
        _lib.set_global_option("host_ingest", 1)
        if g is not None:
            g.close()
    del keep
    if case.data == "special":
        assert list(zero_rows) == [7]
        _check_zero_rows(f, zero_rows, case.norm)
        assert np.array_equal(f.rows_f32[8].view(np.uint32), f.rows_f32[9].view(np.uint32))
        assert np.array_equal(f.rowstat[8].view(np.uint32), f.rowstat[9].view(np.uint32))
    if case.data == "tinyraw":                             # (reported, not asserted: see the module docstring)
        a = gfile.stored_norms(f)
        tiny = (a > 0) & (a < gfile.STAT_REL_FLOOR)
        below = tiny & (f.rowstat[:n].astype(np.float64) < a)
        print("tiny norms: %d below 2^-100, stat < norm in %d of them, largest shortfall %.3g (2^-150 = %.3g)" % (
            int(tiny.sum()), int(below.sum()), float((a - f.rowstat[:n])[tiny].max()), 2.0 ** -150))
        assert tiny.sum() >= 40
    if case.data == "fp16exact":
        assert f.img_f16 == 1 and not f.rowstat[:, 2].view(np.uint32).any(), "norm_diff of rows that are exact in fp16 must be 0"
    if case.data == "single":
        r = n // 2
        want = np.zeros(f.dp, np.float32)
        want[d // 3] = -1.0
        assert np.array_equal(f.rows_f32[r].view(np.uint32), want.view(np.uint32))
        assert f.rowstat[r, 2] == 0.0 and f.rowstat[r, 0] == f.rowstat[r, 1] == np.float32(1.0 + 1e-6)


@pytest.mark.parametrize("n,d,data", [(1027, 2048, "gauss"), (300, 100, "special"), (257, 2500, "gauss")],
                         ids=[ROWS_FULL_F32, ROWS_8, ROWS_16])
def test_reimaging_keeps_the_rows_and_rebuilds_image_and_stats(n, d, data, tmp_path):
    """set_image_dtype(0) then (1): launch_ingest over the stored rows (row stride dp, MI_NORM_NONE).  The stored rows stay bit
    for bit; image, rounding norms, maxima and padding are those of the new type (assertions 2-6)."""
    import torch
    from isehr_amd import _lib
    rows = source_rows(data, 4242 + d, n, d, "f32")
    ref = gfile.reference_rows(rows, NORM_L2)
    keep = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    g = _lib.Gallery.from_device_ptr(keep.data_ptr(), n, d)
    try:
        first = _snapshot_and_check(g, str(tmp_path / "a.bin"), ref, 1, n, d, NORM_L2)
        for f16 in (0, 1):
            g.set_image_dtype(f16)
            f = _snapshot_and_check(g, str(tmp_path / "b.bin"), ref, f16, n, d, NORM_L2)
            assert np.array_equal(f.rows_f32.view(np.uint32), first.rows_f32.view(np.uint32)), "re-imaging changed the stored rows"
        assert f.header_sums == first.header_sums and np.array_equal(f.gstat3.view(np.uint32), first.gstat3.view(np.uint32))
    finally:
        g.close()


def test_padding_stats_of_an_appended_gallery_in_a_recycled_buffer(tmp_path):
    """Assertion 5 where it is at risk: an appendable gallery adopts the buffers of the gallery destroyed last (same sizes, the
    spare slot of csrc/api_gallery.hip) and fills fewer rows than that one held.  The append paths write the stats of the appended
    rows only, so rows n..npad of RowStat are whatever mi_gallery_create_empty left there: it has to clear them (it does, together
    with the image and gstat3) -- the previous gallery's stats would otherwise be saved and checksummed."""
    import torch
    from isehr_amd import _lib
    from isehr_amd.synth import synth_rows
    cap, n, d = 1300, 1000, 2048
    rows = synth_rows(77, 0, cap, d)
    keep = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    _lib.Gallery.from_device_ptr(keep.data_ptr(), cap, d).close()         # rows 1000..1299 of its RowStat are non-zero
    g = _lib.Gallery.empty(cap, d)
    try:
        g.append_device(keep.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _snapshot_and_check(g, str(tmp_path / "g.bin"), gfile.reference_rows(rows[:n], NORM_L2), 1, n, d, NORM_L2)
    finally:
        g.close()
