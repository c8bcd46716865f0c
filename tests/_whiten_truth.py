"""Shared helpers of the scatter-matrix GPU tests (tests/test_gpu_whitenlearn.py, tests/test_gpu_input_layouts_proj.py):
mi_scatter_matrix_device on torch tensors, the float64 numpy scatter and the any-order bound |C_ij - ref_ij| <= 2 n u
sqrt(C_ii C_jj), u = 2^-53 (Cauchy-Schwarz on the standard dot-product error bound)."""
import numpy as np

U = 2.0 ** -53


def _torch():
    import torch
    return torch


class DevScatter:
    """mi_scatter_matrix_device on torch tensors."""

    def __init__(self, lib, d):
        torch = _torch()
        self.lib, self.d = lib, d
        self.ws_bytes = lib.scatter_workspace_bytes(d)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda")

    def __call__(self, rows, centre=None, pairs=None, into=None):
        """rows: CUDA tensor view [n, d]; centre: numpy [d] | None; pairs: (q, p) numpy int64; into: accumulate onto it."""
        torch = _torch()
        n, d = rows.shape
        C = into if into is not None else torch.empty((d, d), dtype=torch.float64, device="cuda")
        c = None if centre is None else torch.from_numpy(np.ascontiguousarray(centre, dtype=np.float64)).cuda()
        q = p = None
        if pairs is not None:
            q = torch.from_numpy(np.ascontiguousarray(pairs[0], dtype=np.int64)).cuda()
            p = torch.from_numpy(np.ascontiguousarray(pairs[1], dtype=np.int64)).cuda()
        self.lib.scatter_matrix_device(rows.data_ptr(), n, d, C.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                       None if c is None else c.data_ptr(), None if q is None else q.data_ptr(),
                                       None if p is None else p.data_ptr(), 0 if q is None else q.numel(),
                                       into is not None, self.lib.MI_F32 if rows.dtype == torch.float32 else self.lib.MI_F64,
                                       rows.stride(0), rows.stride(1), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return C


def _check(C, ref, n, what):
    """Asserts the any-order bound, exact symmetry; returns the largest observed ratio error / bound."""
    assert np.array_equal(C, C.T), what + ": C != C.T"
    dg = np.sqrt(np.abs(np.diag(ref)))
    bound = 2.0 * n * U * np.outer(dg, dg)
    err = np.abs(C - ref)
    ok = err <= bound
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    assert ok.all(), "%s: %d entries beyond 2 n u sqrt(C_ii C_jj), largest ratio %.3f" % (what, int((~ok).sum()), ratio)
    return ratio


def _ref_scatter(x, centre):
    xc = x.astype(np.float64) - (0.0 if centre is None else centre[None, :])
    return xc.T @ xc
