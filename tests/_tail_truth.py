"""Float64 truth and float32 yardstick of the descriptor tail (csrc/desc_tail.hip), the shape sweep of
tests/test_gpu_descriptor_tail.py and its seeded inputs.  Shared by test_descriptor_tail_cpu.py (which pins these helpers to the
reference's own outputs in tests/golden/extractor_tail.npz and checks that the sweep covers what it claims) and
test_gpu_descriptor_tail.py.

    GeM   src/layers/functional.py:20-22      mean_hw(clamp(x, eps)^p)^(1/p)
    L2N   src/layers/functional.py:129-130    x / (||x|| + 1e-6)
    tail  src/networks/imageretrievalnet.py:183-187   L2N(GeM(x)) [-> x @ W.T + b -> L2N]
    ms    src/networks/imageretrievalnet.py:464-479   (mean_s d_s^msp)^(1/msp) / ||.||   (no eps)

`tail64` / `ms64` are numpy float64; `tail32` / `ms32` are the same chains in torch float32 on the CPU, op by op in the reference's
order.  e_ref = max|tail32 - tail64| of a case is what float32 arithmetic itself costs there: the kernels are held to a small
multiple of it (`bound`), never to a figure taken from their own output."""
import functools

import numpy as np
import torch

L2N_EPS = 1e-6
FLOOR = 2.0 ** -21          # four float32 ulps of a unit-norm entry
CEILING = 2e-6              # what tests/test_gpu_extractor.py accepts everywhere: no bound here is looser


def _np64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).astype(np.float64)


def _t32(x):
    return x.detach().cpu().float() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x, dtype=np.float32))


def gem64(feat, p, eps):
    """feat [B, C, H, W] -> [B, C] float64."""
    x = _np64(feat)
    x = x.reshape(x.shape[0], x.shape[1], -1)
    return (np.maximum(x, eps) ** p).mean(axis=2) ** (1.0 / p)


def l2n64(x):
    x = _np64(x)
    return x / (np.sqrt((x * x).sum(axis=1, keepdims=True)) + L2N_EPS)


def tail64(feat, p, eps, W=None, b=None):
    x = l2n64(gem64(feat, p, eps))
    if W is None:
        return x
    y = x @ _np64(W).T
    if b is not None:
        y = y + _np64(b)
    return l2n64(y)


def ms64(descs, msp):
    """descs: sequence of [B, D] (one per scale) -> [B, D] float64."""
    v = sum(_np64(d) ** msp for d in descs) / len(descs)
    v = v ** (1.0 / msp)
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def _l2n32(x):
    return x / (torch.norm(x, p=2, dim=1, keepdim=True) + L2N_EPS).expand_as(x)


def tail32(feat, p, eps, W=None, b=None):
    """The reference's float32 chain: LF.gem -> LF.l2n [-> F.linear -> LF.l2n], torch on the CPU -> numpy float32 [B, D]."""
    x = _t32(feat)
    x = torch.nn.functional.avg_pool2d(x.clamp(min=eps).pow(p), (x.size(-2), x.size(-1))).pow(1. / p)
    x = _l2n32(x).squeeze(-1).squeeze(-1)
    if W is not None:
        x = _l2n32(torch.nn.functional.linear(x, _t32(W), None if b is None else _t32(b)))
    return x.numpy()


def ms32(descs, msp):
    """extract_ms on float32 rows (each row of a batch is one image of the reference's batch-of-one loop)."""
    v = torch.zeros_like(_t32(descs[0]))
    for d in descs:
        v += _t32(d).pow(msp)
    v /= len(descs)
    v = v.pow(1. / msp)
    v /= v.norm(dim=1, keepdim=True)
    return v.numpy()


def bound(e_ref, factor=4.0):
    """max(factor * e_ref, four ulps), never above the project's 2e-6."""
    return min(max(factor * float(e_ref), FLOOR), CEILING)


# ---- seeded inputs

def make_feat(seed, b, c, h, w, positive=False, zero_image=None, hot=None, scale=1.0):
    """Post-ReLU-like maps: rand * 2 - 0.3 (about 15 % of each map lies below eps and is clamped).  positive: rand * 2 + 0.01
    (nothing clamps: with hw = 1, p = 1 GeM is the identity).  zero_image: index of an all-zero image.  hot: (image, channel,
    value) puts one hot pixel into an otherwise ordinary image.  scale multiplies everything (1e4 / 1.7 for values up to 1e4)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((b, c, h, w), generator=g, dtype=torch.float32) * 2.0 + (0.01 if positive else -0.3)
    x = x * scale
    if zero_image is not None:
        x[zero_image] = 0.0
    if hot is not None:
        x[hot[0], hot[1], h // 2, w // 2] = hot[2]
    return x


def make_whiten(seed, c, c_out, bias=True):
    g = torch.Generator().manual_seed(seed + 7919)
    W = torch.randn((c_out, c), generator=g, dtype=torch.float32) / c ** 0.5
    b = torch.randn((c_out,), generator=g, dtype=torch.float32) * 0.1 if bias else None
    return W, b


def make_descs(seed, nscales, b, d, signed=True):
    """nscales unit-norm [b, d] float32 rows, the kind of input the multi-scale pair sees after the tail."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(nscales):
        x = torch.randn((b, d), generator=g, dtype=torch.float32)
        if not signed:
            x = x.abs()
        out.append(x / x.norm(dim=1, keepdim=True))
    return out


# ---- the sweep of the tail: (b, c, c_out or None, (h, w), p, bias)

HW = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (1, 65), 1089: (33, 33), 4096: (64, 64)}
BS = [1, 7, 8, 9, 16, 17]
CS = [7, 64, 130, 2048, 2560, 4968]
COUTS = [1, 5, 66, 130]
PS = [1.0, 2.9137, 3.0, 10.0]

TAIL_CASES = [
    # with whitening
    (1, 7, 1, 1, 1.0, True), (7, 64, 5, 63, 2.9137, True), (8, 130, 66, 64, 3.0, True), (9, 2048, 130, 65, 10.0, True),
    (16, 64, 5, 1089, 3.0, False), (17, 130, 66, 1, 1.0, True), (1, 2560, 130, 64, 3.0, True), (8, 2560, 5, 63, 2.9137, True),
    (9, 2560, 66, 1, 1.0, False), (1, 4968, 1, 65, 3.0, True), (8, 4968, 130, 1, 1.0, True), (9, 4968, 5, 64, 10.0, True),
    (7, 130, 1, 4096, 3.0, True), (17, 2048, 66, 63, 3.0, False), (16, 7, 130, 65, 2.9137, True), (9, 7, 5, 1089, 10.0, True),
    (8, 2048, 1, 1, 10.0, True), (16, 64, 130, 4096, 1.0, True), (1, 130, 66, 1089, 2.9137, False), (7, 2048, 5, 64, 1.0, True),
    (9, 64, 66, 65, 3.0, True), (17, 7, 1, 63, 10.0, True),
    # GeM -> L2N alone
    (1, 7, None, 1, 1.0, False), (7, 64, None, 63, 2.9137, False), (8, 130, None, 64, 3.0, False),
    (9, 2048, None, 65, 10.0, False), (16, 64, None, 1089, 3.0, False), (17, 7, None, 4096, 1.0, False),
    (1, 2560, None, 1089, 3.0, False), (8, 4968, None, 65, 2.9137, False), (9, 2560, None, 1, 10.0, False),
    (1, 4968, None, 1, 1.0, False), (17, 2048, None, 64, 3.0, False), (7, 130, None, 4096, 10.0, False),
    (7, 7, None, 63, 3.0, False), (16, 2048, None, 63, 1.0, False), (8, 64, None, 1, 2.9137, False),
    (9, 130, None, 1089, 1.0, False), (1, 64, None, 4096, 2.9137, False), (17, 7, None, 65, 10.0, False),
]


def stage_of(case):
    """'gem': GeM -> L2N (no whitening).  'linear': hw = 1, p = 1 on inputs above eps, where GeM is the identity and what is left
    is L2N -> Linear -> L2N.  'full': the whole chain."""
    b, c, c_out, hw, p, bias = case
    if c_out is None:
        return "gem"
    return "linear" if hw == 1 and p == 1.0 else "full"


@functools.lru_cache(maxsize=None)
def tail_case(i):
    """-> (feat f32 [b, c, h, w], W or None, bias or None, p, eps, t64 float64 [b, d], e_ref): inputs and both references of sweep
    case i, computed once and shared (callers must not write into them)."""
    case = TAIL_CASES[i]
    b, c, c_out, hw, p, bias = case
    h, w = HW[hw]
    feat = make_feat(5000 + i, b, c, h, w, positive=stage_of(case) == "linear")
    W, bb = make_whiten(5000 + i, c, c_out, bias) if c_out is not None else (None, None)
    t64 = tail64(feat, p, 1e-6, W, bb)
    e_ref = float(np.abs(tail32(feat, p, 1e-6, W, bb).astype(np.float64) - t64).max())
    return feat, W, bb, p, 1e-6, t64, e_ref


# ---- the sweep of the multi-scale pair: (b, d, nscales, msp, signed)

MS_BS = [1, 5, 9]
MS_DS = [5, 48, 257, 2048]
MS_SCALES = [1, 2, 3, 5]
MS_CASES = [
    (1, 5, 1, 1.0, True), (5, 48, 2, 2.0, True), (9, 257, 3, 1.0, True), (1, 2048, 5, 2.0, True),      # 2048 = 8 * 256
    (5, 2048, 2, 1.0, True), (9, 5, 5, 2.0, True), (1, 48, 3, 2.0, True), (5, 257, 1, 2.0, True),       # 5 * 2048 = 40 * 256
    (9, 2048, 3, 2.0, True), (9, 48, 5, 1.0, True), (5, 5, 3, 1.0, True), (1, 257, 2, 1.0, True),
    (1, 5, 2, 2.9137, False), (5, 48, 3, 2.9137, False), (9, 257, 5, 2.9137, False), (5, 2048, 1, 2.9137, False),
]


@functools.lru_cache(maxsize=None)
def ms_case(i):
    """-> (descs: nscales x f32 [b, d], msp, m64 float64 [b, d], e_ref)."""
    b, d, nscales, msp, signed = MS_CASES[i]
    descs = make_descs(7000 + i, nscales, b, d, signed)
    m64 = ms64(descs, msp)
    e_ref = float(np.abs(ms32(descs, msp).astype(np.float64) - m64).max())
    return descs, msp, m64, e_ref
