"""Host-side reader of the prepared-gallery file (MI355GAL v2), a float64 reference of what gallery ingest has to leave in it,
and the assertions that compare the two (plain numpy; used by tests/test_gpu_gallery_reference.py on files the library saved
and by tests/test_gallery_reference_cpu.py on synthetic ones).

File (csrc/api_file.hip): header `<8s4q4i3fI3QQ` | f32 rows [n][dp] | 16-bit image [npad][dp] | RowStat[npad] (3 x f32).
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
TILE, SLICE_K, BLOCK_ELEMS = 256, 32, 8192
GOLD = np.uint64(0x9E3779B97F4A7C15)

TIE_WINDOW_ULP = 1e-5                 # stored rows: |ref - midpoint| below this many float32 ulp accepts either neighbour
STAT_LO, STAT_HI = 1.0 + 8e-7, 1.0 + 1.2e-6      # stat / float64 norm of what was stored
STAT_REL_FLOOR = 2.0 ** -100          # below: |stat - a| <= 2^-149 + 1.2e-6 a (float32 subnormal results)


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
    assert npad == -(-n // TILE) * TILE and dp == -(-d // 64) * 64, (n, npad, d, dp)
    o0 = HEADER.size
    o1 = o0 + n * dp * 4
    o2 = o1 + npad * dp * 2
    o3 = o2 + npad * 12
    assert len(raw) >= o3, "truncated file"
    gf = types.SimpleNamespace(n=n, npad=npad, row_offset=row_offset, d=d, dp=dp, norm_mode=norm_mode, img_f16=img_f16)
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
    returns the same bits.  whitened: |stored - ref| <= 0.5 ulp_f32(ref) + 1e-12 instead."""
    n, d = gf.n, gf.d
    stored = gf.rows_f32[:, :d]
    assert not gf.rows_f32[:, d:].view(np.uint32).any(), "stored rows: padding columns are not +0.0: " + _where(
        gf.rows_f32[:, d:].view(np.uint32) != 0)
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


CHECKS = {
    "checksums": check_checksums,
    "stored rows": check_stored_rows,
    "image": check_image,
    "padding column": check_padding_columns,
    "padding row": check_padding_rows,
    "rounding norms": check_rounding_norms,
    "maxima": check_maxima,
    "padding stats": check_padding_stats,
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
