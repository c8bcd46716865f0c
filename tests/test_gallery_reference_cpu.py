"""CPU: the host-side reader / reference of the prepared-gallery file (tests/_gallery_file.py) cannot be wrong unnoticed.

A test-local numpy WRITER restates the file layout a second time, as an encoder (reshape / transpose / per-row chunk
permutation instead of the reader's offset table), and a numpy model of the ingest arithmetic fills it: the reader must return
every element where it started, the checks of tests/test_gpu_gallery_reference.py must pass on the clean file and FAIL, each by
the assertion meant for it, on a deliberately damaged one.  Squared-L2 files (header word metric == 1, d = ud + 3) are modelled
with the numpy restatement of the bias split (_gallery_file.split_bias), and every way the hidden columns can be wrong that the
suite knows of fails check_l2_columns -- or the existing check that covers it -- by name."""
import math
import os
import struct
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gallery_file as gf_mod  # noqa: E402
from _gallery_file import NORM_L2, NORM_L2_EPS, NORM_NONE  # noqa: E402


# ---- a second statement of the layout: the encoder ----------------------------------------------------------------------
def encode_image(bits):
    """image_bits [npad, dp] -> flat file order: blocked[tile][slice][row][32], 16-byte chunk c of a row at c ^ ((-(row >> 2)) & 3)."""
    npad, dp = bits.shape
    blocked = bits.reshape(npad // 256, 256, dp // 32, 4, 8).transpose(0, 2, 1, 3, 4).copy()     # [tile][slice][row][chunk][8]
    out = np.empty_like(blocked)
    for row in range(256):
        s = (-(row >> 2)) & 3
        for c in range(4):
            out[:, :, row, c ^ s, :] = blocked[:, :, row, c, :]
    return out.reshape(-1)


def write_gallery_file(path, rows_f32, image_bits, rowstat, gstat3, d, norm_mode, img_f16, sums=None, metric=0):
    n, dp = rows_f32.shape
    npad = image_bits.shape[0]
    sec = [np.ascontiguousarray(rows_f32, dtype="<f4").tobytes(), encode_image(np.ascontiguousarray(image_bits, dtype="<u2")).tobytes(),
           np.ascontiguousarray(rowstat, dtype="<f4").tobytes()]
    if sums is None:
        sums = [gf_mod.section_sum(s) for s in sec]
    head = struct.pack("<8s4q4i3fI3Q", b"MI355GAL", 2, n, npad, 0, d, dp, norm_mode, img_f16, *[float(v) for v in gstat3], metric, *sums)
    h = 0xcbf29ce484222325
    for byte in head:                                                  # FNV-1a of the header (csrc/api_file.hip host_sum)
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    with open(path, "wb") as f:
        f.write(head + struct.pack("<Q", h))
        for s in sec:
            f.write(s)


def model_gallery(x, norm_mode, img_f16):
    """numpy model of the ingest arithmetic: (float)((double)x * (1 / nrm)), 16-bit rounding, (float)(sqrt(s) (1 + 1e-6))."""
    n, d = x.shape
    dp, npad = -(-d // 64) * 64, -(-n // 256) * 256
    x = x.astype(np.float64)
    rows = np.zeros((n, dp), np.float32)
    if norm_mode == NORM_NONE:
        rows[:, :d] = x
    else:
        nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        with np.errstate(divide="ignore", invalid="ignore"):
            rows[:, :d] = x * (1.0 / nrm if norm_mode == NORM_L2 else 1.0 / (nrm + 1e-6))
    bits = np.zeros((npad, dp), np.uint16)
    bits[:n] = gf_mod.round16_bits(rows, img_f16)
    g = rows.astype(np.float64)
    b = gf_mod.decode16(bits[:n], img_f16)
    stat = np.zeros((npad, 3), np.float32)
    with np.errstate(invalid="ignore"):
        for j, v in enumerate((g, b, b - g)):
            stat[:n, j] = np.sqrt((v * v).sum(axis=1)) * (1.0 + 1e-6)
    return rows, bits, stat, gf_mod.expected_maxima(stat, n)


def _source(n, d, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


# ---- round trip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dp", [64, 2048, 2560])
@pytest.mark.parametrize("n", [1, 256, 257])
def test_writer_and_reader_agree_on_every_element(tmp_path, n, dp):
    rng = np.random.default_rng(n * 7 + dp)
    d = dp - 3
    npad = -(-n // 256) * 256
    rows = rng.standard_normal((n, dp)).astype(np.float32)
    # every image element carries its own (row, column) so that a misplaced one cannot pass by chance
    bits = ((np.arange(npad)[:, None] * 2654435761 + np.arange(dp)[None, :] * 40503) % 65521).astype(np.uint16)
    stat = rng.random((npad, 3)).astype(np.float32)
    path = str(tmp_path / "g.bin")
    write_gallery_file(path, rows, bits, stat, [1.5, 2.5, 0.25], d, NORM_L2, 1)
    g = gf_mod.read_gallery_file(path)
    assert (g.n, g.npad, g.d, g.dp, g.norm_mode, g.img_f16) == (n, npad, d, dp, NORM_L2, 1)
    assert np.array_equal(g.rows_f32, rows) and np.array_equal(g.image_bits, bits) and np.array_equal(g.rowstat, stat)
    assert g.gstat3.tolist() == [1.5, 2.5, 0.25]
    assert g.host_sums == g.header_sums
    # the documented formula, element by element, on a sample of positions (the reader uses a per-tile table)
    for r, k in [(0, 0), (n - 1, dp - 1), (npad - 1, 9), (min(5, npad - 1), 40), (npad - 4, dp - 8)]:
        c = (k % 32) // 8
        off = ((r // 256) * (dp // 32) + k // 32) * 8192 + (r % 256) * 32 + 8 * (c ^ ((-((r % 256) >> 2)) & 3)) + k % 8
        assert g.image_flat[off] == bits[r, k]


def test_checksum_is_the_documented_sum():
    rng = np.random.default_rng(5)
    buf = rng.integers(0, 256, 8 * 37, dtype=np.uint8).tobytes()
    words = struct.unpack("<37Q", buf)
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)
    want = sum(mix(w ^ ((i * 0x9E3779B97F4A7C15) & M)) for i, w in enumerate(words)) & M
    assert gf_mod.section_sum(buf) == want


# ---- number formats -------------------------------------------------------------------------------------------------------
def test_bf16_rounding_matches_torch_bit_for_bit():
    import torch
    rng = np.random.default_rng(11)
    vals = [rng.standard_normal(20000).astype(np.float32), (rng.standard_normal(5000) * 1e-39).astype(np.float32),
            (rng.standard_normal(5000) * 1e37).astype(np.float32)]
    hi = rng.integers(0, 1 << 16, 4000).astype(np.uint32) << np.uint32(16)
    ties = np.concatenate([hi | np.uint32(0x8000), hi | np.uint32(0x7FFF), hi | np.uint32(0x8001)]).view(np.float32)
    vals.append(ties[np.isfinite(ties)])
    vals.append(np.array([0.0, -0.0, np.inf, -np.inf, 3.4028235e38, -3.4028235e38, 3.3961775e38, 3.3895314e38, 1e-45, -1e-45,
                          1.1754942e-38, 9.1835e-41, 4.5918e-41], np.float32))
    x = np.concatenate(vals)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(gf_mod.bf16_bits(x), want)
    assert np.array_equal(gf_mod.decode16(want, 0), torch.from_numpy(x).to(torch.bfloat16).to(torch.float64).numpy())
    assert gf_mod.is_nan16(gf_mod.bf16_bits(np.array([np.nan], np.float32)), 0).all()
    assert not gf_mod.is_nan16(want, 0).any()


def test_fp16_rounding_and_decoding():
    x = np.array([0.0, 1.0, 65504.0, 65519.0, 65520.0, 70000.0, -70000.0, 6.0e-8, 2.98e-8, 2.9802322e-8, 1.0 + 2.0 ** -11,
                  1.0 + 3 * 2.0 ** -11], np.float32)
    b = gf_mod.fp16_bits(x)
    assert b.tolist() == [0, 0x3C00, 0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0xFC00, 1, 0, 0, 0x3C00, 0x3C02]
    assert gf_mod.decode16(b, 1)[:4].tolist() == [0.0, 1.0, 65504.0, 65504.0]
    assert gf_mod.is_nan16(gf_mod.fp16_bits(np.array([np.nan], np.float32)), 1).all() and not gf_mod.is_nan16(b, 1).any()


def test_accurate_sum_and_reference_rows():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((6, 2048))
    x[1] *= 1e-20
    x[2] *= 1e18
    x[3, 1:] *= 1e-9                                                    # one dominant element: a naive sum loses the rest
    x[4] = 0.0
    got = gf_mod.row_norms(x)
    for i in range(6):
        want = gf_mod.fsum_norm(x[i])
        assert abs(got[i] - want) <= 2.0 ** -52 * want, i
    a = np.array([[1e16, 1.0, -1e16, 1.0, 2.0 ** -30]])
    assert gf_mod.accurate_row_sums(a)[0] == math.fsum(a[0]) == 2.0 + 2.0 ** -30
    ref = gf_mod.reference_rows(x, NORM_L2)
    assert np.isnan(ref[4]).all() and abs(gf_mod.fsum_norm(ref[2]) - 1.0) < 1e-15
    assert not gf_mod.reference_rows(x, NORM_L2_EPS)[4].any()
    assert np.array_equal(gf_mod.reference_rows(x, NORM_NONE), x)
    assert gf_mod.ulp_f32(np.array([1.0, 1.5, 0.75, 2.0 ** -140, 0.0])).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -24, 2.0 ** -149,
                                                                                      2.0 ** -149]


# ---- the checks pass on a modelled gallery and fail on a damaged one ---------------------------------------------------------
def _clean(norm_mode=NORM_L2, img_f16=1, n=300, d=100, special=True):
    x = _source(n, d, seed=n + d)
    if special:
        x[7] = 0.0
        x[10] *= 1e-20
        x[11] *= 1e18
        x[12, ::2] = 0.0
    rows, bits, stat, gmax = model_gallery(x, norm_mode, img_f16)
    return x, rows, bits, stat, gmax


@pytest.mark.parametrize("img_f16", [1, 0])
@pytest.mark.parametrize("norm_mode", [NORM_L2, NORM_L2_EPS, NORM_NONE])
def test_checks_pass_on_the_model(tmp_path, norm_mode, img_f16):
    x, rows, bits, stat, gmax = _clean(norm_mode, img_f16, special=norm_mode != NORM_NONE)
    path = str(tmp_path / "g.bin")
    write_gallery_file(path, rows, bits, stat, gmax, x.shape[1], norm_mode, img_f16)
    g = gf_mod.read_gallery_file(path)
    gf_mod.check_all(g, ref=gf_mod.reference_rows(x, norm_mode), get_rows=rows[:, :x.shape[1]], norm_bounds=gmax)
    if norm_mode == NORM_L2:                                           # the zero row: NaN rows, NaN stats, outside the maxima
        assert np.isnan(g.rows_f32[7, :g.d]).all() and np.isnan(g.rowstat[7]).all() and np.isfinite(g.gstat3).all()
        assert gf_mod.is_nan16(g.image_bits[7, :g.d], img_f16).all()


def _damage(kind, rows, bits, stat, gmax, d):
    rows, bits, stat, gmax = rows.copy(), bits.copy(), stat.copy(), np.array(gmax, np.float32)
    n = rows.shape[0]
    if kind == "image element off by one 16-bit ulp":
        bits[41, 17] += 1
        return "image", rows, bits, stat, gmax
    if kind == "two swizzled chunks exchanged":
        bits[130, 32:40], bits[130, 40:48] = bits[130, 40:48].copy(), bits[130, 32:40].copy()
        return "image", rows, bits, stat, gmax
    if kind == "norm_diff scaled by 0.9":
        stat[55, 2] *= np.float32(0.9)
        return "rounding norms", rows, bits, stat, gmax
    if kind == "non-zero padding column":
        bits[3, d + 2] = 0x0001
        return "padding column", rows, bits, stat, gmax
    if kind == "non-zero padding row":
        bits[n + 1, 5] = 0x3C00
        return "padding row", rows, bits, stat, gmax
    if kind == "gstat3[2] lowered by one float32 ulp":
        gmax[2] = np.nextafter(gmax[2], np.float32(0))
        return "maxima", rows, bits, stat, gmax
    if kind == "stored element off by one float32 ulp":
        rows[20, 3] = np.nextafter(rows[20, 3], np.float32(2))
        bits[20, 3] = gf_mod.round16_bits(rows[20:21, 3:4], 1)[0, 0]
        return "stored rows", rows, bits, stat, gmax
    if kind == "non-zero padding stat":
        stat[n + 2, 1] = 1.0
        return "padding stats", rows, bits, stat, gmax
    if kind == "stale section checksum":
        return "checksums", rows, bits, stat, gmax
    raise ValueError(kind)


DAMAGES = ["image element off by one 16-bit ulp", "two swizzled chunks exchanged", "norm_diff scaled by 0.9",
           "non-zero padding column", "non-zero padding row", "gstat3[2] lowered by one float32 ulp",
           "stored element off by one float32 ulp", "non-zero padding stat", "stale section checksum"]


@pytest.mark.parametrize("kind", DAMAGES)
def test_each_damage_fails_the_check_meant_for_it(tmp_path, kind):
    x, rows, bits, stat, gmax = _clean()
    d = x.shape[1]
    check, rows, bits, stat, gmax = _damage(kind, rows, bits, stat, gmax, d)
    path = str(tmp_path / "g.bin")
    # (the section checksums are those of the damaged content, so that the named check is what catches the damage)
    write_gallery_file(path, rows, bits, stat, gmax, d, NORM_L2, 1, sums=[1, 2, 3] if check == "checksums" else None)
    g = gf_mod.read_gallery_file(path)
    kw = dict(ref=gf_mod.reference_rows(x, NORM_L2), get_rows=rows[:, :d], norm_bounds=gmax, whitened=False)
    with pytest.raises(AssertionError, match="^" + check + ":"):
        gf_mod.CHECKS[check](g, **kw)
    with pytest.raises(AssertionError, match=check + ":"):
        gf_mod.check_all(g, **kw)
    # ... and nothing else does, beyond what the same damage implies: the rounding norms are those of the STORED values, so a
    # changed image or row element moves norm_img / norm_diff, and the image check covers the padding columns of rows < n too
    implied = {"image": {"rounding norms"}, "stored rows": {"rounding norms"}, "padding column": {"image"}}.get(check, set())
    for name, fn in gf_mod.CHECKS.items():
        if name != check and name not in implied:
            fn(g, **kw)


def test_tie_window_and_whitened_tolerance():
    """The other float32 neighbour is accepted only where the reference lies within 1e-5 ulp of the tie; the whitened append's
    bound is 0.5 ulp + 1e-12."""
    lo = np.float32(0.3)
    hi = np.nextafter(lo, np.float32(1))
    ulp = float(hi) - float(lo)
    mid = 0.5 * (float(lo) + float(hi))

    def g(v):
        return types.SimpleNamespace(n=1, d=1, dp=64, rows_f32=np.array([[v] + [0.0] * 63], np.float32))
    gf_mod.check_stored_rows(g(hi), ref=np.array([[mid - 0.9e-5 * ulp]]))          # rounds to lo; hi accepted
    gf_mod.check_stored_rows(g(lo), ref=np.array([[mid + 0.9e-5 * ulp]]))
    with pytest.raises(AssertionError, match="stored rows"):
        gf_mod.check_stored_rows(g(hi), ref=np.array([[mid - 2e-5 * ulp]]))
    with pytest.raises(AssertionError, match="stored rows"):
        gf_mod.check_stored_rows(g(np.nextafter(hi, np.float32(1))), ref=np.array([[mid]]))
    gf_mod.check_stored_rows(g(hi), ref=np.array([[mid + 0.1 * ulp]]), whitened=True)    # 0.4 ulp off
    with pytest.raises(AssertionError, match="stored rows"):
        gf_mod.check_stored_rows(g(hi), ref=np.array([[float(lo) - 0.2 * ulp]]), whitened=True)
    tiny = np.float32(1e-13)
    gf_mod.check_stored_rows(g(tiny), ref=np.array([[float(tiny) + 0.9e-12]]), whitened=True)
    with pytest.raises(AssertionError, match="stored rows"):
        gf_mod.check_stored_rows(g(tiny), ref=np.array([[float(tiny) + 1.1e-12]]), whitened=True)


# ---- squared-L2 files: the hidden columns ------------------------------------------------------------------------------------
def model_l2_gallery(x, img_f16, sign=1.0, stat_cols=None):
    """numpy model of an L2 gallery: the user's rows as given, the split of -1/2 ||g||^2 behind them, zeros up to dp; image and
    rounding norms over the whole augmented row.  sign = -1 / stat_cols = ud model two of the damages."""
    n, ud = x.shape
    d = ud + 3
    dp, npad = -(-d // 64) * 64, -(-n // 256) * 256
    rows = np.zeros((n, dp), np.float32)
    rows[:, :ud] = x
    b, c1, c2, c3 = gf_mod.split_bias(rows[:, :ud], img_f16)
    rows[:, ud], rows[:, ud + 1], rows[:, ud + 2] = sign * c1, sign * c2, sign * c3
    return (rows,) + _l2_image_and_stats(rows, npad, img_f16, stat_cols)


def _l2_image_and_stats(rows, npad, img_f16, stat_cols=None):
    n = rows.shape[0]
    bits = np.zeros((npad, rows.shape[1]), np.uint16)
    bits[:n] = gf_mod.round16_bits(rows, img_f16)
    g = rows.astype(np.float64)[:, :stat_cols]
    b = gf_mod.decode16(bits[:n], img_f16)[:, :stat_cols]
    stat = np.zeros((npad, 3), np.float32)
    with np.errstate(invalid="ignore"):
        for j, v in enumerate((g, b, b - g)):
            stat[:n, j] = np.sqrt((v * v).sum(axis=1)) * (1.0 + 1e-6)
    return bits, stat, gf_mod.expected_maxima(stat, n)


def _l2_source(n=300, ud=100, scale=1.5):
    x = _source(n, ud, seed=n + ud)
    x = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True) * scale).astype(np.float32)
    x[7] = 0.0                                                          # zero row: c1 = -0.0
    x[8] = x[9]
    x[10] *= np.float32(1e-20)                                          # bias ~1e-40: below float32's normal range
    return x


@pytest.mark.parametrize("ud", [1, 61, 62, 100, 2048])
@pytest.mark.parametrize("img_f16", [1, 0])
def test_l2_checks_pass_on_the_model(tmp_path, img_f16, ud):
    x = _l2_source(300 if ud < 2048 else 40, ud)
    if not img_f16:
        x[11] *= np.float32(300.0)                                      # bias beyond fp16's range
    rows, bits, stat, gmax = model_l2_gallery(x, img_f16)
    path = str(tmp_path / "g.bin")
    write_gallery_file(path, rows, bits, stat, gmax, ud + 3, NORM_NONE, img_f16, metric=1)
    g = gf_mod.read_gallery_file(path)
    assert (g.metric, g.ud, g.d, g.dp) == (1, ud, ud + 3, -(-(ud + 3) // 64) * 64)
    gf_mod.check_all(g, ref=x.astype(np.float64), get_rows=rows[:, :ud])
    assert np.signbit(g.rows_f32[7, ud]) and not g.rows_f32[7].any() and g.image_bits[7, ud] == 0x8000
    # an inner-product file of the same rows: the new check does not run, the header word is 0
    write_gallery_file(path, rows, bits, stat, gmax, ud + 3, NORM_NONE, img_f16)
    g = gf_mod.read_gallery_file(path)
    assert (g.metric, g.ud) == (0, ud + 3)
    gf_mod.check_all(g, ref=rows[:, :ud + 3].astype(np.float64), get_rows=rows[:, :ud + 3], norm_bounds=gmax)


def test_l2_bias_beyond_float32_is_pinned_as_non_finite(tmp_path):
    """A row of norm 1e20: -1/2 ||g||^2 = -5e39 is beyond float32, the split gives (-inf, +inf, NaN), the stats are non-finite and
    stay outside the maxima; the checks accept exactly that, and only where the bias is that large."""
    x = _l2_source()
    x[11] = (x[11].astype(np.float64) / 1.5 * 1e20).astype(np.float32)
    rows, bits, stat, gmax = model_l2_gallery(x, 0)
    assert rows[11, 100] == -np.inf and rows[11, 101] == np.inf and np.isnan(rows[11, 102])
    assert not np.isfinite(stat[11]).any() and np.isfinite(gmax).all()
    path = str(tmp_path / "g.bin")
    write_gallery_file(path, rows, bits, stat, gmax, 103, NORM_NONE, 0, metric=1)
    gf_mod.check_all(gf_mod.read_gallery_file(path), ref=x.astype(np.float64), get_rows=rows[:, :100])
    rows[12, 100:103] = rows[11, 100:103]                               # the same columns on an ordinary row
    bits, stat, gmax = _l2_image_and_stats(rows, 512, 0)
    write_gallery_file(path, rows, bits, stat, gmax, 103, NORM_NONE, 0, metric=1)
    with pytest.raises(AssertionError, match="^l2 columns: split: non-finite"):
        gf_mod.check_l2_columns(gf_mod.read_gallery_file(path))


def _l2_damage(kind, x, img_f16):
    """-> (check, message pattern, checks the same damage implies, rows, bits, stat, gmax, metric)"""
    n, ud = x.shape
    rows, bits, stat, gmax = model_l2_gallery(x, img_f16)
    npad = bits.shape[0]
    rnd = lambda v: gf_mod.decode16(gf_mod.round16_bits(v, img_f16), img_f16).astype(np.float32)   # noqa: E731
    if kind == "hidden columns one chunk off in the image":
        bits[:n, ud + 8:ud + 11] = bits[:n, ud:ud + 3]
        bits[:n, ud:ud + 3] = 0
        return "l2 columns", "l2 columns: image", {"image", "padding column", "rounding norms"}, rows, bits, stat, gmax, 1
    if kind == "c2 and c3 swapped":
        rows[:, [ud + 1, ud + 2]] = rows[:, [ud + 2, ud + 1]]
        return ("l2 columns", r"l2 columns: split: c2 != float32\(B - c1\)", set(), rows) + _l2_image_and_stats(rows, npad, img_f16) + (1,)
    if kind == "c2 replaced by its 16-bit rounding":
        rows[:, ud + 1] = rnd(rows[:, ud + 1])
        return ("l2 columns", "l2 columns: (split|value)", set(), rows) + _l2_image_and_stats(rows, npad, img_f16) + (1,)
    if kind == "c1 not representable in the image type":
        b = -0.5 * (x.astype(np.float64) ** 2).sum(1)
        rows[:, ud] = b.astype(np.float32)
        rows[:, ud + 1] = (b - rows[:, ud].astype(np.float64)).astype(np.float32)
        rows[:, ud + 2] = 0.0
        return ("l2 columns", r"l2 columns: split: c1 != round16", set(), rows) + _l2_image_and_stats(rows, npad, img_f16) + (1,)
    if kind == "non-zero in column ud + 3":
        rows[5, ud + 3] = 0.25
        return ("stored rows", "stored rows: padding columns", {"padding column"}, rows) + _l2_image_and_stats(rows, npad, img_f16) + (1,)
    if kind == "non-zero image element in column ud + 3":
        bits[5, ud + 3] = 0x3C00
        return "padding column", "padding column:", {"image", "rounding norms"}, rows, bits, stat, gmax, 1
    if kind == "rounding norms over the user's columns only":
        return ("rounding norms", "rounding norms: stat / norm outside", set(), rows) + _l2_image_and_stats(rows, npad, img_f16, ud) + (1,)
    if kind == "bias of the wrong sign":
        return ("l2 columns", "l2 columns: value", set()) + model_l2_gallery(x, img_f16, sign=-1.0) + (1,)
    if kind == "metric word 2":
        return "header", "header: metric word 2", set(), rows, bits, stat, gmax, 2
    raise ValueError(kind)


L2_DAMAGES = ["hidden columns one chunk off in the image", "c2 and c3 swapped", "c2 replaced by its 16-bit rounding",
              "c1 not representable in the image type", "non-zero in column ud + 3", "non-zero image element in column ud + 3",
              "rounding norms over the user's columns only", "bias of the wrong sign", "metric word 2"]


@pytest.mark.parametrize("img_f16", [1, 0])
@pytest.mark.parametrize("kind", L2_DAMAGES)
def test_each_l2_damage_fails_the_check_meant_for_it(tmp_path, kind, img_f16):
    x = _l2_source()
    ud = x.shape[1]
    check, pattern, implied, rows, bits, stat, gmax, metric = _l2_damage(kind, x, img_f16)
    path = str(tmp_path / "g.bin")
    write_gallery_file(path, rows, bits, stat, gmax, ud + 3, NORM_NONE, img_f16, metric=metric)
    if check == "header":
        with pytest.raises(AssertionError, match="^" + pattern):
            gf_mod.read_gallery_file(path)
        return
    g = gf_mod.read_gallery_file(path)
    kw = dict(ref=x.astype(np.float64), get_rows=rows[:, :ud], norm_bounds=None, whitened=False)
    with pytest.raises(AssertionError, match="^" + pattern):
        gf_mod.CHECKS[check](g, **kw)
    with pytest.raises(AssertionError, match=pattern):
        gf_mod.check_all(g, **kw)
    for name, fn in gf_mod.CHECKS.items():
        if name != check and name not in implied:
            fn(g, **kw)
