"""Host-side reader of the prepared-gallery file (MI355GAL v2), a float64 reference of what gallery ingest has to leave in it,
and the assertions that compare the two (plain numpy; used by tests/test_gpu_gallery_reference.py on files the library saved
and by tests/test_gallery_reference_cpu.py on synthetic ones).

File (csrc/api_file.hip): header `<8s4q4i3fI3QQ` | f32 rows [n][dp] | 16-bit image [npad][dp] | RowStat[npad] (3 x f32).
The header's 32-bit word behind gstat3 is `metric`: 0 = inner product (the word was reserved and zero before), 1 = squared L2
(DESIGN.md 5.11), anything else is no gallery file.  In an L2 file `d` is the AUGMENTED width ud + 3: the user's ud columns, then
the three hidden bias columns c1, c2, c3 with c1 + c2 + c3 = -1/2 ||g||^2, then zeros up to dp; the sections are the memory as it
lies, so every check below runs over the augmented row, and check_l2_columns pins the hidden columns themselves.
Image layout (csrc/common.h): X[rows][dp] is stored as blocked[tile = row / 256][slice = k / 32][row % 256][32] with the four
16-byte chunks of each 64-byte row permuted, physical chunk = c ^ ((-(row >> 2)) & 3) -- so element (row, k) sits in block
(row // 256, k // 32) of 8192 elements at (row % 256) * 32 + 8 * (c ^ ((-((row % 256) >> 2)) & 3)) + k % 8, c = (k % 32) // 8.
Nothing here calls library code.

Every check_* function raises AssertionError with a message that starts with the check's name (CHECKS)."""
import math
import struct
import types

import numpy as np

HEADER = struct.Struct("<8s4q4i3fI3QQ")
NORM_NONE, NORM_L2, NORM_L2_EPS = 0, 1, 2
METRIC_IP, METRIC_L2 = 0, 1
TILE, SLICE_K, BLOCK_ELEMS = 256, 32, 8192
GOLD = np.uint64(0x9E3779B97F4A7C15)

TIE_WINDOW_ULP = 1e-5                 # stored rows: |ref - midpoint| below this many float32 ulp accepts either neighbour
STAT_LO, STAT_HI = 1.0 + 8e-7, 1.0 + 1.2e-6      # stat / float64 norm of what was stored
STAT_REL_FLOOR = 2.0 ** -100          # below: |stat - a| <= 2^-149 + 1.2e-6 a (float32 subnormal results)
BIAS_EXACT_FLOOR = 2.0 ** -97         # |b| below: the float64 ulp of b is finer than float32's 2^-149 grid (check_l2_columns b)


# ---- 16-bit number formats -----------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> bfloat16 bits, round to nearest even on the upper 16 bits (overflow to inf); NaN -> a quiet NaN."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def fp16_bits(x):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def round16_bits(x, img_f16):
    return fp16_bits(x) if img_f16 else bf16_bits(x)


def decode16(bits, img_f16):
    """16-bit image bits -> float64 values (exact)."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if img_f16:
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def is_nan16(bits, img_f16):
    bits = np.asarray(bits, dtype=np.uint16)
    return (bits & 0x7FFF) > (0x7C00 if img_f16 else 0x7F80)


# ---- checksums (csrc/ingest.hip checksum_kernel) -------------------------------------------------------------------------
def mix64(x):
    with np.errstate(over="ignore"):
        x = x + GOLD
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def section_sum(buf):
    """sum over the section's 8-byte words of mix64(word ^ index * golden ratio), mod 2^64."""
    words = np.frombuffer(buf, dtype="<u8", count=len(buf) // 8)
    with np.errstate(over="ignore"):
        idx = np.arange(words.size, dtype=np.uint64) * GOLD
        return int(np.add.reduce(mix64(words ^ idx), dtype=np.uint64))


# ---- image layout -------------------------------------------------------------------------------------------------------
def tile_offsets(dp):
    """[256, dp] offsets of element (row % 256, k) inside its tile's dp / 32 blocks."""
    r = np.arange(TILE, dtype=np.int64)[:, None]
    k = np.arange(dp, dtype=np.int64)[None, :]
    c = (k % SLICE_K) // 8
    swz = (-(r >> 2)) & 3
    return (k // SLICE_K) * BLOCK_ELEMS + r * SLICE_K + 8 * (c ^ swz) + k % 8


def decode_image(flat, npad, dp):
    """flat uint16 [npad * dp] in file order -> image_bits [npad, dp]."""
    tiles = np.asarray(flat, dtype=np.uint16).reshape(npad // TILE, TILE * dp)
    return tiles[:, tile_offsets(dp)].reshape(npad, dp)


# ---- reader -------------------------------------------------------------------------------------------------------------
def read_gallery_file(path):
    raw = open(path, "rb").read()
    h = HEADER.unpack_from(raw, 0)
    magic, version, n, npad, row_offset, d, dp, norm_mode, img_f16 = h[:9]
    assert magic == b"MI355GAL" and version == 2, (magic, version)
    metric = h[12]
    assert metric in (METRIC_IP, METRIC_L2), "header: metric word %d is neither 0 (inner product) nor 1 (squared L2)" % metric
    assert metric == METRIC_IP or (norm_mode == NORM_NONE and d >= 4), "header: an L2 file with norm_mode %d, d %d" % (norm_mode, d)
    assert npad == -(-n // TILE) * TILE and dp == -(-d // 64) * 64, (n, npad, d, dp)
    o0 = HEADER.size
    o1 = o0 + n * dp * 4
    o2 = o1 + npad * dp * 2
    o3 = o2 + npad * 12
    assert len(raw) >= o3, "truncated file"
    gf = types.SimpleNamespace(n=n, npad=npad, row_offset=row_offset, d=d, dp=dp, norm_mode=norm_mode, img_f16=img_f16,
                               metric=metric, ud=d - 3 if metric == METRIC_L2 else d)
    gf.gstat3 = np.frombuffer(raw, dtype="<f4", count=3, offset=struct.calcsize("<8s4q4i"))
    gf.header_sums = tuple(h[13:16])
    gf.rows_f32 = np.frombuffer(raw, dtype="<f4", count=n * dp, offset=o0).reshape(n, dp)
    gf.image_flat = np.frombuffer(raw, dtype="<u2", count=npad * dp, offset=o1)
    gf.image_bits = decode_image(gf.image_flat, npad, dp)
    gf.rowstat = np.frombuffer(raw, dtype="<f4", count=npad * 3, offset=o2).reshape(npad, 3)
    gf.host_sums = (section_sum(raw[o0:o1]), section_sum(raw[o1:o2]), section_sum(raw[o2:o3]))
    return gf


# ---- float64 reference ----------------------------------------------------------------------------------------------------
def accurate_row_sums(a):
    """Row sums of a float64 [n, m] array with a compensated (Neumaier) sum: as accurate as math.fsum to an ulp of the result,
    vectorised over the rows (checked against math.fsum in tests/test_gallery_reference_cpu.py)."""
    a = np.asarray(a, dtype=np.float64)
    s = np.zeros(a.shape[0])
    comp = np.zeros(a.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(a.shape[1]):
            v = a[:, j]
            t = s + v
            big = np.abs(s) >= np.abs(v)
            comp += np.where(big, (s - t) + v, (v - t) + s)
            s = t
        return s + comp


def row_norms(a):
    """float64 Euclidean norms of the rows of a (values that are float32 / 16-bit: their squares are exact in float64)."""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(accurate_row_sums(a * a))


def reference_rows(x, norm_mode):
    """The rows the gallery has to hold, in float64, from the source rows."""
    x = np.asarray(x, dtype=np.float64)
    if norm_mode == NORM_NONE:
        return x.copy()
    nrm = row_norms(x)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return x / nrm if norm_mode == NORM_L2 else x / (nrm + 1e-6)


def ulp_f32(v):
    """float32 unit in the last place at |v| (float64 in, float64 out; 2^-149 in the subnormal range)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(v)
    return np.ldexp(1.0, np.where(v > 0, np.maximum(e - 24, -149), -149))


# ---- the assertions -------------------------------------------------------------------------------------------------------
def _where(mask, limit=3):
    idx = np.argwhere(mask)
    return "%d elements, first at %s" % (len(idx), idx[:limit].tolist())


def check_checksums(gf, **_):
    assert gf.host_sums == gf.header_sums, "checksums: host %s, header %s" % (
        ["%016x" % s for s in gf.host_sums], ["%016x" % s for s in gf.header_sums])


def check_stored_rows(gf, ref=None, get_rows=None, whitened=False, **_):
    """1: rows_f32[:, :d] == float32(ref) (either neighbour within TIE_WINDOW_ULP of a tie); columns d..dp are +0.0; get_rows()
    returns the same bits.  whitened: |stored - ref| <= 0.5 ulp_f32(ref) + 1e-12 instead.  L2 file: ref and get_rows() are the
    user's ud columns; the padding columns start behind the hidden ones (d = ud + 3)."""
    n, d = gf.n, getattr(gf, "ud", gf.d)
    stored = gf.rows_f32[:, :d]
    assert not gf.rows_f32[:, gf.d:].view(np.uint32).any(), "stored rows: padding columns are not +0.0: " + _where(
        gf.rows_f32[:, gf.d:].view(np.uint32) != 0)
    if get_rows is not None:
        assert np.array_equal(np.ascontiguousarray(get_rows).view(np.uint32), np.ascontiguousarray(stored).view(np.uint32)), \
            "stored rows: get_rows() differs from the file"
    if ref is None:
        return
    assert ref.shape == (n, d), (ref.shape, n, d)
    s64 = stored.astype(np.float64)
    nan_ok = np.isnan(ref) & np.isnan(stored)
    if whitened:
        with np.errstate(invalid="ignore"):
            bad = ~(np.abs(s64 - ref) <= 0.5 * ulp_f32(ref) + 1e-12) & ~nan_ok
        assert not bad.any(), "stored rows: beyond 0.5 ulp + 1e-12 of the float64 whitened row: %s, worst %.3e" % (
            _where(bad), float(np.nanmax(np.abs(s64 - ref) - 0.5 * ulp_f32(ref))))
        return
    with np.errstate(over="ignore", invalid="ignore"):
        want = ref.astype(np.float32)
    same = (want.view(np.uint32) == np.ascontiguousarray(stored).view(np.uint32)) | nan_ok
    if same.all():
        return
    # the other neighbour is accepted where ref lies within TIE_WINDOW_ULP float32 ulp of the midpoint of the two
    r, c = np.nonzero(~same)
    a, b = stored[r, c], want[r, c]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        neighbours = np.nextafter(lo, np.float32(np.inf)) == hi
        lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
        near_tie = np.abs(ref[r, c] - 0.5 * (lo64 + hi64)) <= TIE_WINDOW_ULP * (hi64 - lo64)
    bad = ~(neighbours & near_tie & np.isfinite(lo64) & np.isfinite(hi64))
    assert not bad.any(), "stored rows: %d elements are not float32(ref), first (row, col, stored, want, ref): %s" % (
        int(bad.sum()), [(int(r[i]), int(c[i]), float(a[i]), float(b[i]), float(ref[r[i], c[i]])) for i in np.nonzero(bad)[0][:3]])


def check_image(gf, **_):
    """2: image == 16-bit rounding of the STORED float32 value for rows < n (NaN as NaN)."""
    n = gf.n
    want = round16_bits(gf.rows_f32, gf.img_f16)
    got = gf.image_bits[:n]
    ok = (got == want) | (is_nan16(got, gf.img_f16) & is_nan16(want, gf.img_f16))
    assert ok.all(), "image: not the %s rounding of the stored row: %s" % ("fp16" if gf.img_f16 else "bf16", _where(~ok))


def check_padding_columns(gf, **_):
    assert not gf.image_bits[:, gf.d:].any(), "padding column: non-zero image element in columns d..dp: " + _where(
        gf.image_bits[:, gf.d:] != 0)


def check_padding_rows(gf, **_):
    assert not gf.image_bits[gf.n:].any(), "padding row: non-zero image element in rows n..npad: " + _where(gf.image_bits[gf.n:] != 0)


def stored_norms(gf):
    """float64 norms [n, 3] of the stored float32 row, the decoded image row and their float64 difference."""
    n = gf.n
    g = gf.rows_f32.astype(np.float64)
    b = decode16(gf.image_bits[:n], gf.img_f16)
    with np.errstate(invalid="ignore"):
        diff = b - g
    return np.stack([row_norms(g), row_norms(b), row_norms(diff)], axis=1)


def check_rounding_norms(gf, **_):
    """3: a (1 + 8e-7) <= stat <= a (1 + 1.2e-6) for a >= 2^-100, |stat - a| <= 2^-149 + 1.2e-6 a below; 0 where a == 0;
    non-finite where a is."""
    a = stored_norms(gf)
    stat = gf.rowstat[:gf.n].astype(np.float64)
    fin = np.isfinite(a)
    bad = (~fin) & ~((np.isnan(a) & np.isnan(stat)) | (np.isinf(a) & np.isinf(stat) & (stat > 0)))
    assert not bad.any(), "rounding norms: the norm is not finite but the stat is (or the other way round): " + _where(bad)
    zero = fin & (a == 0)
    assert not (stat[zero] != 0).any(), "rounding norms: non-zero stat of a zero norm: " + _where(zero & (stat != 0))
    rel = fin & (a >= STAT_REL_FLOOR)
    with np.errstate(invalid="ignore"):
        bad = rel & ~((stat >= a * STAT_LO) & (stat <= a * STAT_HI))
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("rounding norms: stat / norm outside [1 + 8e-7, 1 + 1.2e-6]: %s; row %d stat %d: %.9g / %.17g = %.10f"
                             % (_where(bad), i, j, stat[i, j], a[i, j], stat[i, j] / a[i, j]))
    tiny = fin & (a > 0) & (a < STAT_REL_FLOOR)
    with np.errstate(invalid="ignore"):
        bad = tiny & ~(np.abs(stat - a) <= 2.0 ** -149 + 1.2e-6 * a)
    assert not bad.any(), "rounding norms: tiny norm, |stat - norm| > 2^-149 + 1.2e-6 norm: " + _where(bad)


def expected_maxima(rowstat, n):
    """rowstat_max_kernel: max of each stat over the rows < n whose three stats are all finite; 0 when there is none."""
    st = np.asarray(rowstat[:n], dtype=np.float32)
    keep = np.isfinite(st).all(axis=1)
    return st[keep].max(axis=0) if keep.any() else np.zeros(3, np.float32)


def check_maxima(gf, norm_bounds=None, **_):
    want = expected_maxima(gf.rowstat, gf.n)
    got = np.asarray(gf.gstat3, dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "maxima: header gstat3 %s, rows give %s" % (
        [float(v).hex() for v in got], [float(v).hex() for v in want])
    if norm_bounds is not None:
        nb = np.asarray(norm_bounds, dtype=np.float32)
        assert np.array_equal(nb.view(np.uint32), want.view(np.uint32)), "maxima: norm_bounds() %s, rows give %s" % (
            [float(v).hex() for v in nb], [float(v).hex() for v in want])


def check_padding_stats(gf, **_):
    pad = np.ascontiguousarray(gf.rowstat[gf.n:]).view(np.uint32)
    assert not pad.any(), "padding stats: RowStat of rows n..npad is not (0, 0, 0): %s, first %s" % (
        _where(pad != 0), gf.rowstat[gf.n:][np.nonzero(pad.any(axis=1))[0][:2]].tolist())


def split_bias(rows, f16):
    """numpy restatement of l2_bias_kernel (csrc/l2_metric.hip): b = -1/2 sum g^2 in float64 (plain sum); c1 = f32(b) rounded to the
    image type (kept at fp16's largest finite value where b is beyond it), c2 = f32(b - c1), c3 = f32(b - c1 - c2)
    -> (b float64 [n], c1, c2, c3 float32 [n]).  The model of tests/test_l2_search_cpu.py and tests/test_gallery_reference_cpu.py;
    check_l2_columns does not use it."""
    g = np.asarray(rows, np.float32).astype(np.float64)
    b = -0.5 * (g * g).sum(1)
    with np.errstate(over="ignore", invalid="ignore"):
        b32 = b.astype(np.float32)
        if f16:
            c1 = b32.astype(np.float16).astype(np.float32)
            c1 = np.where(np.isfinite(c1) | ~np.isfinite(b), c1, np.float32(-65504.0)).astype(np.float32)
        else:
            c1 = decode16(bf16_bits(b32), 0).astype(np.float32)
        c2 = (b - c1.astype(np.float64)).astype(np.float32)
        c3 = (b - c1.astype(np.float64) - c2.astype(np.float64)).astype(np.float32)
    return b, c1, c2, c3


def check_l2_columns(gf, ref=None, whitened=False, **_):
    """L2 files only (metric == 1), every row < n.  c1, c2, c3 = stored float32 columns ud, ud + 1, ud + 2, B = (c1 + c2) + c3 in
    float64 -- exact: the three hold at most 11 + 24 + 24 significand bits and come from one double -- and
    b_ref = -1/2 accurate_row_sums(x x) over the STORED user columns (squares of float32 values are exact in float64).

    split   from the file alone, no summation order involved: c1 == round16(float32(B)) in the header's image type,
            c2 == float32(B - c1), c3 == float32(B - c1 - c2) (values; a zero's sign is not part of it).
    image   the image element at column ud decodes to exactly c1: the image holds the leading bias term without error.
    value   |B - b_ref| <= 2 (ceil(ud / 64) + 6) 2^-53 |b_ref|.  The kernel sums per lane an FMA chain of ceil(ud / 64) exact
            squares (each step one rounding of a partial sum <= the lane's total: relative ceil(ud / 64) 2^-53 of the sum of the
            absolute terms, which for squares IS the sum), then 6 butterfly steps over the 64 lanes (6 more roundings), the
            halving is exact: (ceil(ud / 64) + 6) 2^-53 |b| to first order, the standard bound; the factor 2 is to spare and
            covers the reference's own ulp.  Below |b_ref| = 2^-97 the float64 ulp of b is finer than float32's subnormal grid
            2^-149, c3 rounds what is left to that grid, and the three columns cannot hold b: + 2^-150 there (half a grid step),
            from the number format, not from a measurement.
    user    with the source rows: rows_f32[:, :ud] == float32(source) bit for bit (stored as given; a float64 source rounded once).
    A row whose bias is beyond the image type's range (round16(float32(b_ref)) not finite: norms near 1e19 and above in bf16, which is
    what such a gallery is given) holds what the kernel's arithmetic gives, c1 = -inf, c2 = b - c1 = +inf, c3 = inf - inf = NaN;
    a stored NaN gives three NaNs.  Every other row's hidden columns are finite."""
    if getattr(gf, "metric", METRIC_IP) != METRIC_L2:
        return
    n, ud = gf.n, gf.ud
    c = gf.rows_f32[:, ud:ud + 3]
    c64 = c.astype(np.float64)
    x = gf.rows_f32[:, :ud].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        b_ref = -0.5 * accurate_row_sums(x * x)
        B = (c64[:, 0] + c64[:, 1]) + c64[:, 2]
        lead = decode16(round16_bits(b_ref.astype(np.float32), gf.img_f16), gf.img_f16)
    beyond = ~np.isfinite(lead)
    nanrow = np.isnan(b_ref)
    bad = ~beyond & ~np.isfinite(c64).all(axis=1)
    assert not bad.any(), "l2 columns: split: non-finite hidden column of a row whose bias fits the image type: rows %s" % np.nonzero(bad)[0][:5].tolist()
    over = beyond & ~nanrow
    bad = over & ~((c64[:, 0] == lead) & np.isinf(c64[:, 1]) & (c64[:, 1] == -lead) & np.isnan(c64[:, 2]))
    assert not bad.any(), "l2 columns: split: a bias beyond the image type must be stored as (-inf, +inf, NaN): rows %s hold %s" % (
        np.nonzero(bad)[0][:5].tolist(), c[bad][:3].tolist())
    bad = nanrow & ~np.isnan(c64).all(axis=1)
    assert not bad.any(), "l2 columns: split: NaN row without NaN hidden columns: rows %s" % np.nonzero(bad)[0][:5].tolist()
    fin = ~beyond
    with np.errstate(invalid="ignore", over="ignore"):
        w1 = decode16(round16_bits(B.astype(np.float32), gf.img_f16), gf.img_f16)
        w2 = (B - c64[:, 0]).astype(np.float32).astype(np.float64)
        w3 = (B - c64[:, 0] - c64[:, 1]).astype(np.float32).astype(np.float64)
    for j, (w, what) in enumerate(((w1, "c1 != round16(float32(B))"), (w2, "c2 != float32(B - c1)"), (w3, "c3 != float32(B - c1 - c2)"))):
        bad = fin & ~(c64[:, j] == w)
        if bad.any():
            r = int(np.nonzero(bad)[0][0])
            raise AssertionError("l2 columns: split: %s in %d rows, first row %d: stored (%s), want %s" % (
                what, int(bad.sum()), r, ", ".join(float(v).hex() for v in c[r]), float(w[r]).hex()))
    img = decode16(gf.image_bits[:n, ud], gf.img_f16)
    bad = fin & ~(img == c64[:, 0])
    assert not bad.any(), "l2 columns: image: the element at column ud does not decode to c1: rows %s, image %s, c1 %s" % (
        np.nonzero(bad)[0][:5].tolist(), img[bad][:3].tolist(), c64[bad][:3, 0].tolist())
    tol = 2.0 * (-(-ud // 64) + 6) * 2.0 ** -53 * np.abs(b_ref) + np.where(np.abs(b_ref) < BIAS_EXACT_FLOOR, 2.0 ** -150, 0.0)
    with np.errstate(invalid="ignore"):
        err = np.abs(B - b_ref)
        bad = fin & ~(err <= tol)
    if bad.any():
        r = int(np.nonzero(bad)[0][0])
        raise AssertionError("l2 columns: value: |B - b_ref| beyond 2 (ceil(ud / 64) + 6) 2^-53 |b_ref| in %d rows, first row %d: "
                             "B %.17g, b_ref %.17g, error %.3g of the bound" % (int(bad.sum()), r, B[r], b_ref[r], err[r] / tol[r]))
    if ref is not None and not whitened:         # (a whitened append is held to check_stored_rows' 0.5 ulp + 1e-12)
        assert ref.shape == (n, ud), (ref.shape, n, ud)
        with np.errstate(over="ignore", invalid="ignore"):
            want = np.asarray(ref, dtype=np.float64).astype(np.float32)
        stored = np.ascontiguousarray(gf.rows_f32[:, :ud])
        same = (want.view(np.uint32) == stored.view(np.uint32)) | (np.isnan(want) & np.isnan(stored))
        assert same.all(), "l2 columns: user columns are not float32(source) bit for bit: " + _where(~same)


CHECKS = {
    "checksums": check_checksums,
    "stored rows": check_stored_rows,
    "image": check_image,
    "padding column": check_padding_columns,
    "padding row": check_padding_rows,
    "rounding norms": check_rounding_norms,
    "maxima": check_maxima,
    "padding stats": check_padding_stats,
    "l2 columns": check_l2_columns,
}


def check_all(gf, ref=None, get_rows=None, norm_bounds=None, whitened=False):
    """Every assertion on every row and element; all failures are reported together."""
    failures = []
    for name, fn in CHECKS.items():
        try:
            fn(gf, ref=ref, get_rows=get_rows, norm_bounds=norm_bounds, whitened=whitened)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def fsum_norm(row):
    """The norm of one row by math.fsum (the check of accurate_row_sums)."""
    return math.sqrt(math.fsum(float(v) * float(v) for v in row))
