"""GPU: the descriptor tail (csrc/desc_tail.hip: mi_desc_tail_device, mi_desc_ms_accumulate_device, mi_desc_ms_finish_device,
extractor.DescriptorTail, extract_ms_device) against the float64 truth of tests/_tail_truth.py at the batch and shape edges of its
kernels: batches beyond one group of 8 rows (ragged second and third groups), b * c and c_out that are no multiples of the 4 rows
a block packs, c below and across a wave, dynamic LDS under, at and above 64 KiB (c up to the 4968 the ABI accepts), hw around one
wave and long sums, p = 1 / 2.9137 / 3 / 10, no bias.  Stages are isolated by input: W = None leaves GeM -> L2N; hw = 1, p = 1 on
inputs above eps makes GeM the identity and leaves L2N -> Linear -> L2N.

Tolerance.  Every case is held to min(max(FACTOR * e_ref, 2^-21), 2e-6), where e_ref = max|tail32 - tail64| is the error of the
reference's own float32 chain (torch on the CPU) on that case's inputs, computed in the test.  FACTOR = 4 allows for another
summation tree (a 64-lane butterfly against torch's order) and for powf's few-ulp distance from torch's pow; 2^-21 is four
float32 ulps of a unit-norm entry.  Measured on an MI355X (worst kernel_err / e_ref per stage, and worst kernel_err / bound):

    GeM + L2N      (W = None)            4.19  (err 4.1e-9 on e_ref 9.8e-10: b 1, c 4968, hw 1, p 1)   0.11 of its bound
    Linear + L2N   (hw = 1, p = 1)       1.00                                                          0.08
    full chain                           1.11  (b 7, c 64 -> 5, hw 63, p 2.9137)                       0.23
    multi-scale accumulate + finish      1.80  (b 5, d 48, 2 scales, msp 2)                            0.16
    extract_ms_device, identity trunk    1.02                                                          0.15

No case needs more than the starting bound (the one ratio above 4 sits two orders below the four-ulp floor), so every factor
stays at 4.

Every sweep case runs on buffers with a guard band behind `out` and `scratch`: a block whose last rows are past b * c, or past
c_out, must leave it alone."""
import numpy as np
import pytest

import _tail_truth as T

pytestmark = pytest.mark.gpu

FACTOR = {"gem": 4.0, "linear": 4.0, "full": 4.0, "ms": 4.0}
GUARD = 64                  # floats behind every output buffer
SENTINEL = -7.5


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _guarded(n):
    import torch
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")


def _run_tail(feat, W, bias, p, eps):
    """mi_desc_tail_device on guarded buffers -> (out [b, d] numpy float32, guard bands intact?)."""
    import torch
    from isehr_amd import _lib
    b, c, h, w = feat.shape
    d = c if W is None else W.shape[0]
    fd = feat.cuda().contiguous()
    Wd = W.cuda().contiguous() if W is not None else None
    bd = bias.cuda().contiguous() if bias is not None else None
    out = _guarded(b * d)
    scratch = _guarded(b * c) if W is not None else None
    _lib.desc_tail_device(fd.data_ptr(), b, c, h * w, p, eps, Wd.data_ptr() if W is not None else None,
                          bd.data_ptr() if bias is not None else None, d,
                          scratch.data_ptr() if scratch is not None else None, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    ok = bool((out[b * d:] == SENTINEL).all()) and (scratch is None or bool((scratch[b * c:] == SENTINEL).all()))
    return out[:b * d].reshape(b, d).cpu().numpy(), ok


def _tail(p, W=None, bias=None, eps=1e-6):
    from isehr_amd.extractor import DescriptorTail
    return DescriptorTail(p, eps, W.cuda() if W is not None else None, bias.cuda() if bias is not None else None)


def _report(stage, name, err, e_ref, tol):
    print("TAILERR stage=%s case=%s err=%.3e e_ref=%.3e ratio=%.2f bound=%.3e of_bound=%.2f"
          % (stage, name, err, e_ref, err / e_ref if e_ref > 0 else float("inf"), tol, err / tol))


# ---- the sweep

@pytest.mark.parametrize("i", range(len(T.TAIL_CASES)), ids=lambda i: "b%d-c%d-o%s-hw%d-p%g-%s" % (
    T.TAIL_CASES[i][:5] + ("bias" if T.TAIL_CASES[i][5] else "nobias",)))
def test_tail_sweep_vs_float64(i):
    case = T.TAIL_CASES[i]
    feat, W, bias, p, eps, t64, e_ref = T.tail_case(i)
    got, guard_ok = _run_tail(feat, W, bias, p, eps)
    stage = T.stage_of(case)
    tol = T.bound(e_ref, FACTOR[stage])
    err = float(np.abs(got.astype(np.float64) - t64).max())
    _report(stage, repr(case), err, e_ref, tol)
    assert guard_ok, "a kernel wrote behind out [b][d] or scratch [b][c]"
    assert got.shape == t64.shape and np.isfinite(got).all()
    assert err <= tol


# ---- batch invariance, bit for bit

_INV = [(130, 66, (5, 13), 3.0), (2560, 5, (1, 3), 2.9137), (7, None, (7, 9), 10.0)]


@pytest.mark.parametrize("b", [9, 17])
@pytest.mark.parametrize("c,c_out,hw,p", _INV)
def test_rows_of_a_batch_equal_the_single_image_results(b, c, c_out, hw, p):
    """A row's arithmetic does not depend on its group of 8 or on its place in it: any difference is an indexing bug."""
    feat = T.make_feat(900 + b + c, b, c, *hw).cuda()
    W, bias = T.make_whiten(900 + c, c, c_out) if c_out else (None, None)
    tail = _tail(p, W, bias)
    whole = tail(feat).cpu().numpy()
    again = tail(feat).cpu().numpy()
    assert np.array_equal(whole, again)                                          # two calls, same bits
    for k in range(b):
        one = tail(feat[k:k + 1]).cpu().numpy()
        assert np.array_equal(whole[k], one[0]), "image %d of %d" % (k, b)
    assert np.abs(whole - T.tail64(feat, p, 1e-6, W, bias)).max() <= T.CEILING    # and they are the right rows


@pytest.mark.parametrize("c,c_out,hw,p", _INV)
def test_sixteen_rows_equal_two_calls_of_eight(c, c_out, hw, p):
    feat = T.make_feat(950 + c, 16, c, *hw).cuda()
    W, bias = T.make_whiten(950 + c, c, c_out) if c_out else (None, None)
    tail = _tail(p, W, bias)
    whole = tail(feat).cpu().numpy()
    assert np.array_equal(whole[:8], tail(feat[:8]).cpu().numpy())
    assert np.array_equal(whole[8:], tail(feat[8:]).cpu().numpy())


# ---- edge rows

@pytest.mark.parametrize("whiten", [False, True])
@pytest.mark.parametrize("p", [1.0, 2.9137, 3.0])
def test_all_zero_image(whiten, p):
    """Every value clamps to eps: GeM gives eps on every channel, L2N a constant row; finite and equal to the float64 chain."""
    feat = T.make_feat(31, 3, 66, 5, 5, zero_image=1)
    W, bias = T.make_whiten(31, 66, 13) if whiten else (None, None)
    t64 = T.tail64(feat, p, 1e-6, W, bias)
    e_ref = float(np.abs(T.tail32(feat, p, 1e-6, W, bias) - t64).max())
    got, guard_ok = _run_tail(feat, W, bias, p, 1e-6)
    err = float(np.abs(got - t64).max())
    tol = T.bound(e_ref, FACTOR["full" if whiten else "gem"])
    _report("full" if whiten else "gem", "zero-image-p%g-w%d" % (p, whiten), err, e_ref, tol)
    assert guard_ok and np.isfinite(got).all()
    if not whiten:
        assert np.abs(got[1] - 1.0 / (np.sqrt(66.0) + 1.0)).max() < 1e-6          # eps / (eps * sqrt(c) + 1e-6)
    assert err <= tol


@pytest.mark.parametrize("whiten", [False, True])
def test_one_dominant_channel(whiten):
    """One hot pixel of 1e3 in channel 5 of image 1: its pooled vector is that channel and 1e-3-sized others."""
    feat = T.make_feat(32, 3, 66, 4, 4, hot=(1, 5, 1e3))
    W, bias = T.make_whiten(32, 66, 13) if whiten else (None, None)
    t64 = T.tail64(feat, 3.0, 1e-6, W, bias)
    e_ref = float(np.abs(T.tail32(feat, 3.0, 1e-6, W, bias) - t64).max())
    got, guard_ok = _run_tail(feat, W, bias, 3.0, 1e-6)
    err = float(np.abs(got - t64).max())
    tol = T.bound(e_ref, FACTOR["full" if whiten else "gem"])
    _report("full" if whiten else "gem", "dominant-w%d" % whiten, err, e_ref, tol)
    assert guard_ok
    if not whiten:
        assert got[1, 5] > 0.999 and np.delete(got[1], 5).max() < 5e-3
    assert err <= tol


@pytest.mark.parametrize("whiten", [False, True])
@pytest.mark.parametrize("hw", [(1, 1), (64, 64)])
def test_values_up_to_1e4_stay_finite(whiten, hw):
    """x^3 reaches 1e12 and a sum over 4096 of them 4e15, far inside float32: finite wherever the reference's float32 chain is."""
    feat = T.make_feat(33, 2, 130, *hw, scale=1e4 / 1.7)
    assert 9e3 < feat.max().item() <= 1e4
    W, bias = T.make_whiten(33, 130, 5) if whiten else (None, None)
    t64 = T.tail64(feat, 3.0, 1e-6, W, bias)
    t32 = T.tail32(feat, 3.0, 1e-6, W, bias)
    e_ref = float(np.abs(t32 - t64).max())
    got, guard_ok = _run_tail(feat, W, bias, 3.0, 1e-6)
    err = float(np.abs(got - t64).max())
    tol = T.bound(e_ref, FACTOR["full" if whiten else "gem"])
    _report("full" if whiten else "gem", "big-hw%d-w%d" % (hw[0] * hw[1], whiten), err, e_ref, tol)
    assert guard_ok and np.isfinite(t32).all()
    assert np.isfinite(got[np.isfinite(t32)]).all()
    assert err <= tol


# ---- multi-scale

def _ms_by_hand(descs_dev, msp):
    import torch
    from isehr_amd import _lib
    b, d = descs_dev[0].shape
    acc = _guarded(b * d)
    for k, x in enumerate(descs_dev):
        _lib.desc_ms_accumulate_device(acc.data_ptr(), x.data_ptr(), b * d, msp, k == 0, _stream())
    _lib.desc_ms_finish_device(acc.data_ptr(), b, d, len(descs_dev), msp, _stream())
    torch.cuda.synchronize()
    return acc[:b * d].reshape(b, d).cpu().numpy(), bool((acc[b * d:] == SENTINEL).all())


@pytest.mark.parametrize("i", range(len(T.MS_CASES)), ids=lambda i: "b%d-d%d-s%d-msp%g-%s" % (
    T.MS_CASES[i][:4] + ("signed" if T.MS_CASES[i][4] else "nonneg",)))
def test_multiscale_sweep_vs_float64(i):
    descs, msp, m64, e_ref = T.ms_case(i)
    got, guard_ok = _ms_by_hand([x.cuda() for x in descs], msp)
    tol = T.bound(e_ref, FACTOR["ms"])
    err = float(np.abs(got - m64).max())
    _report("ms", repr(T.MS_CASES[i]), err, e_ref, tol)
    assert guard_ok, "a kernel wrote behind acc [b][d]"
    assert np.isfinite(got).all() and err <= tol


@pytest.mark.parametrize("b,c,c_out,hw,msp", [(9, 130, 66, (5, 13), 1.0), (5, 64, None, (8, 8), 2.9137), (17, 7, 5, (1, 1), 2.0)])
def test_extract_ms_device_with_an_identity_trunk(b, c, c_out, hw, msp):
    """ms = (1.0,) keeps interpolation out: extract_ms_device is tail -> accumulate -> finish, the bits of the three calls made
    by hand, and within the bound of ms64(tail64)."""
    import torch
    from isehr_amd.extractor import extract_ms_device
    feat = T.make_feat(60 + b, b, c, *hw)
    W, bias = T.make_whiten(60 + b, c, c_out) if c_out else (None, None)
    if W is not None and msp != 1.0:
        bias = None                                      # msp = 2: signed rows are fine, kept without a bias for variety
    tail = _tail(3.0, W, bias)
    got = extract_ms_device(lambda x: x, tail, feat.cuda(), ms=(1.0,), msp=msp)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    by_hand, _ = _ms_by_hand([tail(feat.cuda())], msp)
    assert np.array_equal(got, by_hand)
    m64 = T.ms64([T.tail64(feat, 3.0, 1e-6, W, bias)], msp)
    e_ref = float(np.abs(T.ms32([T.tail32(feat, 3.0, 1e-6, W, bias)], msp) - m64).max())
    tol = T.bound(e_ref, max(FACTOR["ms"], FACTOR["full"]))
    err = float(np.abs(got - m64).max())
    _report("ms-e2e", "b%d-c%d-o%s-msp%g" % (b, c, c_out, msp), err, e_ref, tol)
    assert err <= tol


@pytest.mark.parametrize("whiten", [False, True])
def test_layouts_and_dtypes_give_the_bits_of_the_contiguous_float32_copy(whiten):
    import torch
    W, bias = T.make_whiten(40, 66, 13) if whiten else (None, None)
    tail = _tail(3.0, W, bias)
    base = T.make_feat(40, 9, 66, 6, 10).cuda()
    want = tail(base.clone()).cpu().numpy()
    cl = base.to(memory_format=torch.channels_last)
    assert not cl.is_contiguous() and np.array_equal(tail(cl).cpu().numpy(), want)
    wide = T.make_feat(41, 9, 70, 6, 14).cuda()
    sl = wide[:, 2:68, :, 3:13]
    assert not sl.is_contiguous() and np.array_equal(tail(sl).cpu().numpy(), tail(sl.contiguous()).cpu().numpy())
    half = base.half()
    assert np.array_equal(tail(half).cpu().numpy(), tail(half.float().contiguous()).cpu().numpy())


# ---- argument checks: refused before anything is launched

def _raw_call(b, c, hw, c_out, whiten=True, scratch=True):
    import torch
    from isehr_amd import _lib
    feat = torch.ones((max(b, 1) * c * hw,), dtype=torch.float32, device="cuda")
    W = torch.ones((c_out * c,), dtype=torch.float32, device="cuda")
    out = _guarded(max(b, 1) * max(c, c_out))
    scr = _guarded(max(b, 1) * c)
    try:
        _lib.desc_tail_device(feat.data_ptr(), b, c, hw, 3.0, 1e-6, W.data_ptr() if whiten else None, None, c_out,
                              scr.data_ptr() if scratch else None, out.data_ptr(), _stream())
    finally:
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((scr == SENTINEL).all()), "a refused call wrote to its buffers"


def test_arguments_are_refused_before_a_launch():
    with pytest.raises(RuntimeError, match="c too large"):
        _raw_call(1, 4969, 1, 2)
    with pytest.raises(RuntimeError, match="bad sizes"):
        _raw_call(0, 7, 4, 2)
    with pytest.raises(RuntimeError, match="scratch"):
        _raw_call(2, 7, 4, 2, scratch=False)
    from isehr_amd.extractor import DescriptorTail
    import torch
    with pytest.raises(RuntimeError, match="c too large"):
        DescriptorTail(3.0, 1e-6, torch.ones((2, 4969), device="cuda"), None)(torch.ones((1, 4969, 1, 1), device="cuda"))
