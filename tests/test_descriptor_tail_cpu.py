"""CPU: the float64 truth and the float32 yardstick of the descriptor tail (tests/_tail_truth.py) against the reference's own
outputs -- LF.gem / LF.l2n / F.linear / extract_ms, captured in tests/golden/extractor_tail.npz by oracle/make_golden.py on the
inputs of `_feats()` / `_tail()` in test_gpu_extractor.py -- and the sweep of test_gpu_descriptor_tail.py against what it claims
to cover.  A truth that disagreed with the reference's captured outputs could not referee the kernels."""
import os

import numpy as np
import pytest
import torch

import _tail_truth as T
from isehr_amd.synth import synth_rows

ULP = 2.0 ** -23            # spacing of float32 in [0.5, 1): no entry of a unit-norm row is resolved finer than that by the goldens
F32_GOLDEN = 1e-7           # what test_oracle_golden.py asks of a float32 chain against a float32 golden


def _inputs():
    feats = [torch.from_numpy(synth_rows(60 + i, 0, 3 * 64, h * w).reshape(3, 64, h, w))
             for i, (h, w) in enumerate(((5, 7), (7, 10), (4, 5)))]
    W = torch.from_numpy(synth_rows(51, 0, 48, 64)) / 8.0
    b = torch.from_numpy(synth_rows(52, 0, 1, 48)[0]) / 8.0
    return feats, W, b


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "extractor_tail.npz"))


def test_tail_truth_vs_reference_layers(golden):
    feats, W, b = _inputs()
    for key, args in (("tail_ss", (3.0, 1e-6, W, b)), ("tail_ss_nowhiten", (2.5, 1e-6))):
        t64, t32 = T.tail64(feats[0], *args), T.tail32(feats[0], *args)
        assert t64.dtype == np.float64 and t32.dtype == np.float32 and t64.shape == t32.shape == golden[key].shape
        e64, e32 = np.abs(t64 - golden[key]).max(), np.abs(t32 - golden[key]).max()
        print("%s: |tail64 - golden| = %.3g, |tail32 - golden| = %.3g" % (key, e64, e32))
        assert e64 <= ULP
        assert e32 <= F32_GOLDEN


@pytest.mark.parametrize("msp,key", [(1.0, "v_ms1"), (2.0, "v_ms2")])
def test_multiscale_truth_vs_reference_extract_ms(golden, msp, key):
    feats, W, b = _inputs()
    m64 = T.ms64([T.tail64(f[:1], 3.0, 1e-6, W, b) for f in feats], msp)
    m32 = T.ms32([T.tail32(f[:1], 3.0, 1e-6, W, b) for f in feats], msp)
    e64, e32 = np.abs(m64[0] - golden[key]).max(), np.abs(m32[0] - golden[key]).max()
    print("%s: |ms64 - golden| = %.3g, |ms32 - golden| = %.3g" % (key, e64, e32))
    assert m64.shape == (1, 48) and e64 <= ULP
    assert e32 <= F32_GOLDEN


def test_stages_in_float64_by_hand():
    """Three numbers a reader can check with a pocket calculator."""
    x = np.array([[[[3.0, 4.0]], [[-1.0, 0.0]]]])                                   # [1, 2, 1, 2]
    assert np.allclose(T.gem64(x, 2.0, 1e-6), [[np.sqrt(12.5), 1e-6]], rtol=1e-15, atol=0)
    assert np.allclose(T.l2n64(np.array([[3.0, 4.0]])), [[3 / (5 + 1e-6), 4 / (5 + 1e-6)]], rtol=1e-15, atol=0)
    d = [np.array([[0.6, 0.8]]), np.array([[0.8, 0.6]])]
    assert np.allclose(T.ms64(d, 1.0), [[0.5 ** 0.5, 0.5 ** 0.5]], rtol=1e-15, atol=0)
    assert np.allclose(T.ms64(d, 2.0), [[0.5 ** 0.5, 0.5 ** 0.5]], rtol=1e-15, atol=0)
    W = np.array([[1.0, 0.0], [0.0, 2.0], [1.0, 1.0]])
    y = T.tail64(np.array([[[[3.0]], [[4.0]]]]), 1.0, 1e-6, W, np.array([0.0, 0.0, 1.0]))
    u = np.array([3.0, 4.0]) / (5 + 1e-6)
    v = np.array([u[0], 2 * u[1], u[0] + u[1] + 1.0])
    assert np.allclose(y, [v / (np.linalg.norm(v) + 1e-6)], rtol=1e-15, atol=0)


def test_bound_is_floor_factor_and_ceiling():
    assert T.bound(0.0) == 2.0 ** -21 and T.bound(1e-7) == 2.0 ** -21
    assert T.bound(2e-7) == 8e-7 and T.bound(2e-7, 8.0) == 1.6e-6
    assert T.bound(1e-3) == 2e-6 == T.CEILING


def test_input_builder_options():
    x = T.make_feat(1, 3, 5, 4, 6)
    assert x.shape == (3, 5, 4, 6) and x.dtype == torch.float32 and torch.equal(x, T.make_feat(1, 3, 5, 4, 6))
    assert 0.05 < (x < 1e-6).float().mean().item() < 0.3 and x.max().item() <= 1.7          # part of each map gets clamped
    assert T.make_feat(1, 3, 5, 4, 6, positive=True).min().item() >= 0.01
    z = T.make_feat(1, 3, 5, 4, 6, zero_image=1)
    assert (z[1] == 0).all() and torch.equal(z[0], x[0]) and torch.equal(z[2], x[2])
    h = T.make_feat(1, 3, 5, 4, 6, hot=(2, 3, 1e3))
    assert h[2, 3, 2, 3].item() == 1e3 and (h != x).sum().item() == 1
    big = T.make_feat(1, 3, 5, 4, 6, scale=1e4 / 1.7)
    assert 5e3 < big.max().item() <= 1e4


def test_tail_sweep_covers_what_it_claims():
    """Every listed value of every axis once with whitening and once without; the early-exit guards (b * c and c_out not
    multiples of 4, with every remainder of b * c); dynamic LDS of a full group under, at and above 64 KiB; the large-LDS widths
    only at b in {1, 8, 9}; about 40 cases of at most ~4M elements."""
    cases = T.TAIL_CASES
    assert 36 <= len(cases) <= 44 and len(set(cases)) == len(cases)
    for whiten in (True, False):
        sel = [k for k in cases if (k[2] is not None) == whiten]
        assert {k[0] for k in sel} == set(T.BS)
        assert {k[1] for k in sel} == set(T.CS)
        assert {k[3] for k in sel} == set(T.HW)
        assert {k[4] for k in sel} == set(T.PS)
    wh = [k for k in cases if k[2] is not None]
    assert {k[2] for k in wh} == set(T.COUTS)
    assert any(not k[5] for k in wh) and any(k[5] for k in wh)                     # bias = None with W given
    assert {k[0] * k[1] % 4 for k in cases} == {0, 1, 2, 3}
    assert {k[0] for k in cases if k[1] > 2048} == {1, 8, 9}
    assert {min(k[0], 8) * k[1] * 4 for k in wh} >= {65536, 8 * 2560 * 4, 8 * 4968 * 4} and any(
        57344 <= min(k[0], 8) * k[1] * 4 < 65536 for k in wh)
    assert all(k[0] * k[1] * k[3] <= 4.2e6 for k in cases)
    assert {T.stage_of(k) for k in cases} == {"gem", "linear", "full"}
    for k in cases:
        if T.stage_of(k) == "linear":                                               # GeM is the identity there
            feat = T.make_feat(0, k[0], k[1], 1, 1, positive=True)
            assert np.array_equal(T.gem64(feat, 1.0, 1e-6)[:, :, None, None], feat.double().numpy())


def test_ms_sweep_covers_what_it_claims():
    cases = T.MS_CASES
    signed = [k for k in cases if k[4]]
    assert {k[0] for k in signed} == set(T.MS_BS) and {k[1] for k in signed} == set(T.MS_DS)
    assert {k[2] for k in signed} == set(T.MS_SCALES) and {k[3] for k in signed} == {1.0, 2.0}
    assert {k[3] for k in cases if not k[4]} == {2.9137}                            # a non-integer power only on non-negative rows
    assert any(k[0] * k[1] % 256 == 0 for k in cases) and any(k[0] * k[1] % 256 for k in cases)
    assert any(k[0] * k[1] % 256 == 0 and k[0] > 1 for k in cases)


def test_yardstick_is_float32_rounding_not_more():
    """e_ref of a few sweep cases: the reference arithmetic's float32 error on unit-norm outputs stays within a few ulps, so
    max(4 * e_ref, 2^-21) is far below the 2e-6 the tail was held to before."""
    for i in (0, 2, 5, 22, 24):
        e_ref = T.tail_case(i)[6]
        print("case %d %r: e_ref = %.3g" % (i, T.TAIL_CASES[i], e_ref))
        assert 0 < e_ref < 4 * ULP and T.bound(e_ref) <= 2e-6 / 2
    for i in (1, 12):
        e_ref = T.ms_case(i)[3]
        print("ms case %d %r: e_ref = %.3g" % (i, T.MS_CASES[i], e_ref))
        assert 0 < e_ref < 4 * ULP
