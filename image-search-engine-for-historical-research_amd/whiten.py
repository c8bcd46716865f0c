"""Whitening through the HIP path, float64 like the reference (src/utils/whiten.py).

Applying: whitenapply (:4-12) -> whitenapply_hip: X[D,N], m[D,1], P[D,D] -> P[:dimensions] @ (X - m), columns divided by
(||.|| + 1e-6).

Learning: pcawhitenlearn (:14-30) -> pcawhitenlearn_hip, whitenlearn (:32-48) -> whitenlearn_hip.  Both spend their time in a
[D, N] x [N, D] float64 product over all descriptors; that product (the scatter matrix, csrc/scatter.hip) is computed on the
device, centred while the descriptors are loaded, and only D x D matrices reach the host, where numpy / LAPACK factorise
them.  Neither function creates an N x D float64 array, on the host or on the device.

Where this differs from the reference's text, not from its mathematics:
  * the reference calls the general `numpy.linalg.eig` on a symmetric matrix (slower, may hand back a complex dtype, unordered);
    `numpy.linalg.eigh` is used here: the same eigen-decomposition, real and sorted.  Rows of P are defined up to sign;
  * whitenlearn materialises df = Pc (X - m) and multiplies df df^T; here D = Pc C_m Pc^T with C_m the scatter matrix of all
    columns about m -- the same matrix, df df^T = Pc (X - m)(X - m)^T Pc^T;
  * rank-deficient data (N <= D, constant coordinates) raises a ValueError instead of returning inf / nan rows.
"""
import numpy as np

from . import _lib


def whitenapply_hip(X, m, P, dimensions=None, device=0):
    X = np.asarray(X)
    if not dimensions:
        dimensions = np.shape(P)[0]
    out = _lib.whiten_apply(X.T, m, P, int(dimensions), 1e-6, device)      # [N, dims]
    return out.T


# ---- host side of the learners: D x D only -----------------------------------------------------------------------------
def _eigh_descending(A):
    eigval, eigvec = np.linalg.eigh(A)
    order = eigval.argsort()[::-1]
    return eigval[order], eigvec[:, order]


def pca_from_scatter(C, N):
    """C = sum_n (x_n - m)(x_n - m)^T (float64 [D, D], symmetric) of N descriptors -> P [D, D] of pcawhitenlearn:
    diag(eigval^-1/2) @ eigvec.T of C / N, eigenvalues descending.  An eigenvalue that is not positive beyond rounding
    (<= D * 2^-52 * largest) means rank-deficient data: ValueError naming how many.  Also returns the eigenvalues."""
    C = np.asarray(C, dtype=np.float64)
    eigval, eigvec = _eigh_descending(C / N)
    floor = C.shape[0] * np.finfo(np.float64).eps * max(float(eigval[0]), 0.0)
    bad = int(np.count_nonzero(~(eigval > floor)))
    if bad:
        raise ValueError("PCA whitening: %d of %d eigenvalues of the covariance are not positive (rank-deficient data: "
                         "fewer descriptors than dimensions, or constant coordinates)" % (bad, C.shape[0]))
    P = eigvec.T / np.sqrt(eigval)[:, None]
    return P, eigval


def cholesky_jitter(S):
    """The reference's rule (src/utils/whiten.py:50-65): Cholesky factor of S + alpha I with alpha = 0, then 1e-10, then ten
    times more each time, until the matrix is positive definite.  -> (L, alpha)."""
    S = np.asarray(S, dtype=np.float64)
    eye = np.eye(S.shape[0])
    alpha = 0.0
    while True:
        try:
            return np.linalg.cholesky(S + alpha * eye), alpha
        except np.linalg.LinAlgError:
            alpha = 1e-10 if alpha == 0.0 else alpha * 10.0
            if not np.isfinite(alpha) or not np.all(np.isfinite(S)):
                raise ValueError("whitenlearn: the pair scatter matrix is not finite")


def supervised_from_scatter(S, C_m):
    """S = pair scatter / number of pairs, C_m = scatter of all descriptors about m -> P [D, D] of whitenlearn."""
    L, _ = cholesky_jitter(S)
    Pc = np.linalg.inv(L)
    Dm = Pc @ np.asarray(C_m, dtype=np.float64) @ Pc.T
    Dm = (Dm + Dm.T) / 2
    _, eigvec = _eigh_descending(Dm)
    return eigvec.T @ Pc


# ---- device side ---------------------------------------------------------------------------------------------------------
def _is_cuda_tensor(X):
    return hasattr(X, "is_cuda") and bool(X.is_cuda)


class _DeviceRows:
    """The [D, N] CUDA tensor X seen as N strided rows, with the scatter workspace."""

    def __init__(self, X):
        import torch
        if X.dim() != 2 or X.dtype not in (torch.float32, torch.float64):
            raise ValueError("expected a 2-D float32 / float64 tensor [D, N]")
        if X.stride(0) < 0 or X.stride(1) < 0:
            X = X.contiguous()
        self.torch, self.X = torch, X
        self.d, self.n = int(X.shape[0]), int(X.shape[1])
        self.code = _lib.MI_F32 if X.dtype == torch.float32 else _lib.MI_F64
        self.ws_bytes = _lib.scatter_workspace_bytes(self.d)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=X.device)
        self.stream = torch.cuda.current_stream(X.device).cuda_stream

    def column_mean(self, T=None):
        T = self.X if T is None else T
        out = self.torch.empty(self.d, dtype=self.torch.float64, device=self.X.device)
        _lib.column_sum_device(T.data_ptr(), int(T.shape[1]), self.d, out.data_ptr(), self.code, T.stride(1), T.stride(0),
                               self.stream)
        return out / int(T.shape[1])

    def scatter(self, centre=None, q=None, p=None):
        C = self.torch.empty((self.d, self.d), dtype=self.torch.float64, device=self.X.device)
        _lib.scatter_matrix_device(self.X.data_ptr(), self.n, self.d, C.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                   None if centre is None else centre.data_ptr(),
                                   None if q is None else q.data_ptr(), None if p is None else p.data_ptr(),
                                   0 if q is None else int(q.numel()), False, self.code, self.X.stride(1), self.X.stride(0),
                                   self.stream)
        return C.cpu().numpy()


def _host_column_mean(rows, device, block_bytes=64 << 20):
    """float64 mean of the rows of a host array, column sums taken on the device block by block."""
    n, d = rows.shape
    step = max(1, block_bytes // (d * rows.dtype.itemsize))
    s = np.zeros(d, dtype=np.float64)
    for r0 in range(0, n, step):
        s += _lib.column_sum(rows[r0:r0 + step], device)
    return s / n


def _pairs(qidxs, pidxs, n):
    q = np.asarray(qidxs).reshape(-1).astype(np.int64)
    p = np.asarray(pidxs).reshape(-1).astype(np.int64)
    if q.size == 0 or q.size != p.size:
        raise ValueError("whitenlearn: qidxs and pidxs must be non-empty and of one length")
    q = np.where(q < 0, q + n, q)           # numpy indexing of X[:, qidxs] counts negative indices from the end
    p = np.where(p < 0, p + n, p)
    if q.min() < 0 or q.max() >= n or p.min() < 0 or p.max() >= n:
        raise ValueError("whitenlearn: pair index outside [0, %d)" % n)
    return q, p


def pcawhitenlearn_hip(X, device=0):
    """pcawhitenlearn(X) of the reference: X [D, N] (numpy float32 / float64 of either memory order, or a CUDA tensor, which
    is read in place) -> (m [D, 1], P [D, D]) float64."""
    if _is_cuda_tensor(X):
        dev = _DeviceRows(X)
        n = dev.n
        m_dev = dev.column_mean()
        C = dev.scatter(m_dev)
        m = m_dev.cpu().numpy()
    else:
        rows = _lib._strided(np.asarray(X).T)[0]
        n = rows.shape[0]
        m = _host_column_mean(rows, device)
        C = _lib.scatter_matrix(rows, centre=m, device=device)
    P, _ = pca_from_scatter(C, n)
    return m.reshape(-1, 1), P


def whitenlearn_hip(X, qidxs, pidxs, device=0):
    """whitenlearn(X, qidxs, pidxs) of the reference: X [D, N] as for pcawhitenlearn_hip, index lists of matching pairs ->
    (m [D, 1], P [D, D]) float64."""
    if _is_cuda_tensor(X):
        dev = _DeviceRows(X)
        torch = dev.torch
        q, p = _pairs(qidxs, pidxs, dev.n)
        q_dev, p_dev = torch.from_numpy(q).to(X.device), torch.from_numpy(p).to(X.device)
        m_dev = dev.column_mean(dev.X.index_select(1, q_dev))
        S = dev.scatter(None, q_dev, p_dev) / q.size
        C_m = dev.scatter(m_dev)
        m = m_dev.cpu().numpy()
    else:
        rows = _lib._strided(np.asarray(X).T)[0]
        q, p = _pairs(qidxs, pidxs, rows.shape[0])
        m = np.asarray(rows[q], dtype=np.float64).mean(axis=0)
        S = _lib.scatter_matrix(rows, pairs=(q, p), device=device) / q.size
        C_m = _lib.scatter_matrix(rows, centre=m, device=device)
    return m.reshape(-1, 1), supervised_from_scatter(S, C_m)
