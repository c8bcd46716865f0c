"""GPU: every typed, strided entry point of the PQ family (mi_pq, mi_pqw, mi_ivfpq and its residual form, mi_pq_graph, the
trainers), fed each layout of tests/_layouts.py.  Every output must equal, byte for byte, the answer for the contiguous float32
array; that answer is itself pinned, bit for bit, to the family's numpy truths (tests/_pq_truth.py, _pq_wide_truth.py,
_pq_train_truth.py, _ivfpq_truth.py, _ivfpq_residual_truth.py, _pq_graph_truth.py).

This is the family whose header sentence is "never rounded to float32": float64 input that float32 cannot hold must give the
truth fed that float64 input, and inputs are planted so that this differs from the answer for the rounded input:
  row 0   book 0 lies exactly midway between codewords 0 and 1 (the tie goes to 0); the float64 offset tips it to 1
  row 1   lies exactly midway between coarse centroids 0 and 1; the offset tips it to list 1
  row 2   is the concatenation of codewords (j mod Ks) (and a coarse centroid): its table entries / residuals are 0 until offset
  rows 3, 5 (trainers) are the only members of codeword 0 of book 0 and adjacent floats: their float64 mean is a float32 tie"""
import numpy as np
import pytest

import _ivfpq_residual_truth as IR
import _ivfpq_truth as IV
import _layouts as L
import _pq_graph_truth as PG
import _pq_train_truth as PT
import _pq_truth as P
import _pq_wide_truth as PW

pytestmark = pytest.mark.gpu

N, K, EF, R_GRAPH, NLIST, NPROBE, ITERS = 600, 10, 16, 8, 8, 3, 2
# (M, L): d = 35 and 130 (neither a multiple of 4 or 64, 130 crosses one 128-wide slice), and d = 1
BOOKS = [(5, 7), (10, 13), (1, 1)]
NQS = [70, 1]
KS = {"pq": 16, "pqw": 300}                     # 300 codewords: codes that need uint16


@pytest.fixture(scope="module")
def lib():
    return L.load_lib()


def _grid(rng, shape):
    """standard normal values on a 2^-10 grid: float32 values whose small sums and differences are exact"""
    return (np.round(rng.standard_normal(shape) * 1024.0) / 1024.0).astype(np.float32)


class Problem:
    """codebooks, coarse centroids and planted rows of one (kind, M, L)"""

    def __init__(self, kind, M, Ls):
        self.kind, self.M, self.Ls, self.Ks, self.d = kind, M, Ls, KS[kind], M * Ls
        rng = np.random.default_rng(1000 * M + Ls + self.Ks)
        C = _grid(rng, (M, self.Ks, Ls))
        C[C == 0] = 0.5
        C[0, 0, 0], C[0, 1, 0] = 40.5, 42.5
        C[0, 1, 1:] = C[0, 0, 1:]
        self.C = C
        G = _grid(rng, (NLIST, self.d))
        G[G == 0] = 0.5
        G[0, 0], G[1, 0] = 40.5, 42.5
        G[1, 1:] = G[0, 1:]
        self.G = G
        self.codes = rng.integers(0, self.Ks, size=(N, M)).astype(np.uint16 if kind == "pqw" else np.uint8)
        self.codes[:NLIST] = np.arange(M) % self.Ks                      # the rows query 2 reconstructs, one per list
        self.lists = (np.arange(N) % NLIST).astype(np.uint8)

    def rows(self, n, seed=0):
        """float32 [n, d] with the planted rows 0, 1, 2 (as far as n goes)"""
        rng = np.random.default_rng(seed + n + self.d)
        x = _grid(rng, (n, self.d))
        x[x == 0] = 0.25
        plant = np.empty((3, self.d), np.float32)
        plant[0] = x[0]
        plant[0, :self.Ls] = self.C[0, 0]
        plant[0, 0] = 41.5
        plant[1] = self.G[0]
        plant[1, 0] = 41.5
        plant[2] = np.concatenate([self.C[j, j % self.Ks] for j in range(self.M)])
        for i in range(min(n, 3)):
            x[(i + 2) % 3 if n >= 3 else i] = plant[(i + 2) % 3 if n >= 3 else i]
        if n < 3:
            x[0] = plant[2]                                              # one row: the one every entry point distinguishes
        return x

    def beyond(self, x):
        return L.beyond_float32(x, range(min(len(x), 3)), [0])


@pytest.fixture(scope="module")
def ctxs(lib):
    made = {}

    def get(kind, M, Ls):
        key = (kind, M, Ls)
        if key not in made:
            p = Problem(kind, M, Ls)
            cls = lib.WidePQIndex if kind == "pqw" else lib.PQIndex
            p.lib = lib
            p.cls = cls
            p.index = cls.from_codes(p.C, p.codes)
            if kind == "pq":
                p.ivf = lib.IVFPQIndex.from_codes(p.G, p.C, p.codes, p.lists)
                p.ivfr = lib.IVFPQIndex.from_codes(p.G, p.C, p.codes, p.lists, by_residual=True)
                p.graph = lib.PQGraphIndex.build(p.index, R=R_GRAPH, n_entry=4)
            made[key] = p
        return made[key]
    yield get
    for p in made.values():
        for name in ("graph", "ivfr", "ivf", "index"):
            if hasattr(p, name):
                getattr(p, name).close()


def _mem(lib, x):
    """(x_ptr, dtype code, row stride, col stride) of a torch device tensor"""
    import torch
    return x.data_ptr(), lib.MI_F32 if x.dtype == torch.float32 else lib.MI_F64, x.stride(0), x.stride(1)


def _is_host(x):
    return isinstance(x, np.ndarray)


# ---- calls: call(p, x) -> tuple of arrays, x a numpy view or a torch device tensor --------------------------------------------
def _add(p, x, make, read):
    idx = make()
    try:
        if _is_host(x):
            idx.add(x)
        else:
            ptr, code, rs, cs = _mem(p.lib, x)
            idx.add_device(ptr, x.shape[0], dtype=code, row_stride=rs, col_stride=cs)
        return read(idx)
    finally:
        idx.close()


def _pq_add(p, x):
    return _add(p, x, lambda: p.cls.empty(p.C, x.shape[0]), lambda i: (i.get_codes(),))


def _ivf_add(p, x, residual=False):
    return _add(p, x, lambda: p.lib.IVFPQIndex.empty(p.G, p.C, x.shape[0], by_residual=residual), lambda i: tuple(i.get_rows()))


def _encode(p, x):
    if _is_host(x):
        return (p.index.encode(x),)
    import ctypes as C
    ptr, code, rs, cs = _mem(p.lib, x)
    out = np.empty((x.shape[0], p.M), p.cls._CODE)
    p.lib.check(p.cls._fn("encode")(p.index._h, C.c_void_p(ptr), x.shape[0], code, rs, cs, p.lib.MI_DEVICE, C.c_void_p(out.ctypes.data)))
    return (out,)


def _residual_rows(p, x):
    import ctypes as C
    if _is_host(x):
        a, code, rs, cs = p.lib._strided(x)
        ptr, mem = a.ctypes.data, p.lib.MI_HOST
    else:
        ptr, code, rs, cs = _mem(p.lib, x)
        mem = p.lib.MI_DEVICE
    outs = ()
    li = (np.arange(x.shape[0]) % NLIST).astype(np.uint8)
    if mem == p.lib.MI_DEVICE:                                           # list_ids live where the rows live (api_ivfpq.hip)
        import torch
        li_dev = torch.from_numpy(li).cuda()
        torch.cuda.synchronize()
        li_ptr = li_dev.data_ptr()
    else:
        li_ptr = li.ctypes.data
    for lists in (None, li_ptr):
        out = np.empty((x.shape[0], p.d), np.float32)
        p.lib.check(p.lib.load().mi_ivfpq_residual_rows(p.ivfr._h, C.c_void_p(ptr), x.shape[0], code, rs, cs, mem,
                                                        None if lists is None else C.c_void_p(lists),
                                                        C.c_void_p(out.ctypes.data), p.lib.MI_HOST))
        outs += (out,)
    return outs


def _train_init(p, x32):
    """initial codebooks: the default rows, but codeword 0 of book 0 starts on the planted pair (rows 3 and 5, no default initial rows)"""
    C0 = PT.default_init(x32, p.M, p.Ks).astype(np.float32).copy()
    C0[0, 0] = x32[3, :p.Ls]
    return C0


def _train_rows(p, n=N):
    x = p.rows(n, seed=9)
    x[:3] = x[6:9]                                                       # (the planted rows of the encoders would join the pair)
    x[3, :p.Ls] = 90.0
    x[5, :p.Ls] = 90.0
    x[3, 0], x[5, 0] = 64.0, np.nextafter(np.float32(64.0), np.float32(128.0))
    return x


def _train(p, x):
    x32 = _train_rows(p)
    fn = "mi_pqw_train" if p.kind == "pqw" else "mi_pq_train"
    C0 = _train_init(p, x32)
    if _is_host(x):
        a, code, rs, cs = p.lib._strided(x)
        return p.lib._pq_train_call(a.ctypes.data, N, p.d, code, rs, cs, p.lib.MI_HOST, p.M, p.Ks, ITERS, C0, 0, fn)
    ptr, code, rs, cs = _mem(p.lib, x)
    return p.lib._pq_train_call(ptr, N, p.d, code, rs, cs, p.lib.MI_DEVICE, p.M, p.Ks, ITERS, C0, 0, fn)


def _graph_search(p, x):
    ids, dist, _, vis = p.graph.search(x, K, ef=EF, return_visited=True)
    return ids, dist, vis


# ---- truths: truth(p, x) -> the tuple call(p, x) must give, x float32 or float64 contiguous ------------------------------------
def _encode_truth(p, x):
    return (PW.encode_truth16(x, p.C) if p.kind == "pqw" else P.encode_truth(x, p.C),)


def _graph_truth(p, x):
    ids, dist, vis = PG.search_truth(x, p.C, p.codes, p.graph.neighbors, p.graph.entries, K, EF)
    return ids, np.asarray(dist, np.float32), vis


def _ivf_add_truth(p, x):
    lists = IV.probe_truth(x, p.G, 1)[:, 0].astype(np.uint8)
    return P.encode_truth(x, p.C), lists


def _train_truth(p, x):
    fn = PW.train_truth16 if p.kind == "pqw" else PT.train_truth
    return fn(x, p.M, p.Ks, ITERS, _train_init(p, _train_rows(p)))[:2]


def _residual_rows_truth(p, x):
    li = (np.arange(x.shape[0]) % NLIST).astype(np.uint8)
    return (IR.residual_rows_truth(x, p.G, IV.probe_truth(x, p.G, 1)[:, 0]), IR.residual_rows_truth(x, p.G, li))


# name -> (kind, argument: "q" queries (host only; bcast32 too) | "x" rows (host and device) | "train", call, truth)
ROWS = {
    "mi_pq_dtable": ("pq", "q", lambda p, x: (p.index.dtable(x),), lambda p, x: (P.dtable64(x, p.C)[1],)),
    "mi_pq_search": ("pq", "q", lambda p, x: p.index.search(x, K)[:2], lambda p, x: P.pq_truth(x, p.C, p.codes, K)),
    "mi_pq_encode": ("pq", "x", _encode, _encode_truth),
    "mi_pq_add": ("pq", "x", _pq_add, _encode_truth),
    "mi_pq_train": ("pq", "train", _train, _train_truth),
    "mi_pqw_dtable": ("pqw", "q", lambda p, x: (p.index.dtable(x),), lambda p, x: (P.dtable64(x, p.C)[1],)),
    "mi_pqw_search": ("pqw", "q", lambda p, x: p.index.search(x, K)[:2], lambda p, x: P.pq_truth(x, p.C, p.codes, K)),
    "mi_pqw_encode": ("pqw", "x", _encode, _encode_truth),
    "mi_pqw_add": ("pqw", "x", _pq_add, _encode_truth),
    "mi_pqw_train": ("pqw", "train", _train, _train_truth),
    "mi_pq_graph_search": ("pq", "q", _graph_search, _graph_truth),
    "mi_ivfpq_probe": ("pq", "q", lambda p, x: (p.ivf.probe(x, NPROBE),), lambda p, x: (IV.probe_truth(x, p.G, NPROBE),)),
    "mi_ivfpq_search": ("pq", "q", lambda p, x: p.ivf.search(x, K, nprobe=NPROBE)[:2] + p.ivfr.search(x, K, nprobe=NPROBE)[:2],
                        lambda p, x: IV.ivfpq_truth(x, p.C, p.codes, p.lists, IV.probe_truth(x, p.G, NPROBE), K)
                        + IR.residual_ivfpq_truth(x, p.G, p.C, p.codes, p.lists, IV.probe_truth(x, p.G, NPROBE), K)),
    "mi_ivfpq_add": ("pq", "x", lambda p, x: _ivf_add(p, x) + _ivf_add(p, x, True),
                     lambda p, x: _ivf_add_truth(p, x) + IR.residual_encode_truth(x, p.G, p.C)),
    "mi_ivfpq_residual_rows": ("pq", "x", _residual_rows, _residual_rows_truth),
}


_same = L.same


_differs = L.differs


def _cases(p, arg):
    """the contiguous float32 inputs of a row at one problem"""
    if arg == "train":
        return [_train_rows(p)]
    if arg == "q":
        return [p.rows(nq) for nq in NQS]
    return [p.rows(N), p.rows(1)]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_layouts_give_the_contiguous_answer_and_the_truth(lib, ctxs, name):
    """queries from host memory (no memspace; bcast32, rs = 0, included: stage_host_rows of api_internal.h packs host rows
    element by element from x + r rs + c cs, so the table and probe kernels see packed rows); rows and training sets from host and from device memory"""
    import torch
    kind, arg, call, truth = ROWS[name]
    for M, Ls in BOOKS:
        p = ctxs(kind, M, Ls)
        for a in _cases(p, arg):
            want = call(p, a)
            what = "%s, M %d, L %d, %d rows" % (name, M, Ls, len(a))
            _same(want, truth(p, a), what + ", contiguous float32 against the truth")
            poison = 1e30 if arg == "train" else np.nan                 # (a training set is checked for finite values whole)
            for lay in L.layouts(a, poison, bcast=arg == "q"):
                ref = want if lay.name != "bcast32" else call(p, L.expected(lay, a))
                _same(call(p, lay.view), ref, "%s, %s, host" % (what, lay.name))
                if arg != "q":
                    t = L.on_device(lay)
                    torch.cuda.synchronize()
                    _same(call(p, t), want, "%s, %s, device" % (what, lay.name))


@pytest.mark.parametrize("name", sorted(ROWS))
def test_float64_beyond_float32_is_kept(lib, ctxs, name):
    """"never rounded to float32" (include/mi355_retrieval.h): the answer for a64 is the truth fed a64 itself, and it differs from
    the answer for a64.astype(float32)"""
    import torch
    kind, arg, call, truth = ROWS[name]
    for M, Ls in BOOKS:
        p = ctxs(kind, M, Ls)
        a = _cases(p, arg)[0]
        if arg == "train":
            a64 = L.beyond_float32(a, [3], [0])
        else:
            a64 = p.beyond(a)
        what = "%s, M %d, L %d, float64 beyond float32" % (name, M, Ls)
        got = call(p, a64)
        _same(got, truth(p, a64), what)
        assert _differs(got, call(p, a)), what + ": the planted values do not tell the float64 answer from the rounded one"
        for lay in L.layouts(a, 1e30 if arg == "train" else np.nan):
            if lay.name in ("t64", "col64"):
                lay.view[...] = a64
                _same(call(p, lay.view), got, what + ", " + lay.name)
                if arg != "q":
                    t = L.on_device(lay)
                    torch.cuda.synchronize()
                    _same(call(p, t), got, what + ", " + lay.name + ", device")


def test_negative_strides_are_refused(lib, ctxs):
    import ctypes as C
    p = ctxs("pq", 5, 7)
    q = p.rows(3)
    out = np.empty((3, p.M, p.Ks), np.float32)
    assert lib.load().mi_pq_dtable(p.index._h, C.c_void_p(q.ctypes.data), 3, lib.MI_F32, -p.d, 1, C.c_void_p(out.ctypes.data)) == lib.MI_ERR_INVALID
    lists = np.empty((3, 1), np.int32)
    assert lib.load().mi_ivfpq_probe(p.ivf._h, C.c_void_p(q.ctypes.data), 3, lib.MI_F32, p.d, -1, 1, C.c_void_p(lists.ctypes.data)) == lib.MI_ERR_INVALID
