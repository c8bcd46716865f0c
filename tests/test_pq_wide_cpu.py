"""CPU: the wide PQ index (mi_pqw, WidePQIndex, matching_Nano_PQ_wide_hip).  Header, SIGNATURES and the library agree, the C entry
points answer bad arguments before a device is touched, and every refusal of the Python layer is a ValueError before the library
is loaded.  The byte index's surface stays where it was."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "image-search-engine-for-historical-research_amd")

ENTRY_POINTS = ("create", "append_codes", "add", "encode", "dtable", "search", "search_device", "info", "get_codes", "get_codebooks",
                "decode", "destroy", "train")


@pytest.fixture(scope="module")
def built_lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    return _lib.load(), _lib


def _declared_args(code, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_signatures_and_symbols_agree(built_lib):
    lib, _lib = built_lib
    hdr = open(os.path.join(ROOT, "include", "mi355_retrieval.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef\s+struct\s+mi_pqw\s+mi_pqw\s*;", code)
    for name in ENTRY_POINTS:
        wide, byte = "mi_pqw_" + name, "mi_pq_" + name
        assert hasattr(lib, wide) and wide in _lib.SIGNATURES, wide
        args, byte_args = _declared_args(code, wide), _declared_args(code, byte)
        assert len(args) == len(byte_args) == len(_lib.SIGNATURES[wide][1]), wide          # one for one with mi_pq
        assert getattr(lib, wide).restype == C.c_int
    assert "mi_pqw_remove_rows" not in code and not hasattr(lib, "mi_pqw_remove_rows")     # out of scope
    assert "uint16_t* out_codes_host" in " ".join(_declared_args(code, "mi_pqw_encode"))
    assert "uint16_t* out_host" in " ".join(_declared_args(code, "mi_pqw_get_codes"))
    assert _lib.PQW_MAX_WORDS == 8192 and _lib.PQ_MAX_WORDS == 256


def test_slab_constant_is_the_kernel_s():
    from isehr_amd import _lib
    src = open(os.path.join(PKG, "csrc", "pq_wide.hip")).read()
    threads = int(re.search(r"PW_THREADS = (\d+)", src).group(1))
    rpl = int(re.search(r"PW_RPL = (\d+)", src).group(1))
    assert _lib.PQW_SLAB_ROWS == threads * rpl


def test_create_answers_bad_arguments_without_a_device(built_lib):
    lib, _lib = built_lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    cb = np.zeros((4, 16, 2), np.float32)
    codes = np.zeros((5, 4), np.uint16)
    out = C.c_void_p()

    def create(cbp=P(cb), d=8, m=4, ks=16, cp=P(codes), n=5, stride=4, memspace=_lib.MI_HOST, cap=0, op=C.byref(out)):
        return lib.mi_pqw_create(cbp, d, m, ks, cp, n, stride, memspace, 0, 0, cap, op)

    bad_cb = cb.copy()
    bad_cb[3, 15, 1] = np.nan
    bad_codes = codes.copy()
    bad_codes[4, 3] = 16
    cases = [(dict(op=None), b"out"), (dict(cbp=None), b"codebooks_host"), (dict(m=0), b"m (books)"), (dict(m=65, d=130), b"m (books)"),
             (dict(ks=1), b"[2, 8192]"), (dict(ks=8193), b"[2, 8192]"), (dict(d=0), b"d must be in"), (dict(d=4100), b"d must be in"),
             (dict(m=3), b"multiple of m"), (dict(n=-1), b"negative"), (dict(cap=3), b"capacity below"), (dict(cp=None), b"codes"),
             (dict(n=0, cp=None), b"needs a capacity"), (dict(stride=3), b"row_stride below m"), (dict(memspace=2), b"memspace"),
             (dict(cbp=P(bad_cb)), b"finite"), (dict(cp=P(bad_codes)), b"a code is >= ks")]
    for kwargs, word in cases:
        assert create(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
        assert not out.value


def test_handle_entry_points_answer_null_and_k_without_a_device(built_lib):
    lib, _lib = built_lib
    buf = np.zeros(64, np.float32)
    P = buf.ctypes.data_as(C.c_void_p)
    assert lib.mi_pqw_destroy(None) == 0
    calls = [lambda: lib.mi_pqw_append_codes(None, P, 1, 4, _lib.MI_HOST), lambda: lib.mi_pqw_add(None, P, 1, _lib.MI_F32, 8, 1, _lib.MI_HOST),
             lambda: lib.mi_pqw_encode(None, P, 1, _lib.MI_F32, 8, 1, _lib.MI_HOST, P), lambda: lib.mi_pqw_dtable(None, P, 1, _lib.MI_F32, 8, 1, P),
             lambda: lib.mi_pqw_search(None, P, 1, _lib.MI_F32, 8, 1, 1, None, 0, P, P, None),
             lambda: lib.mi_pqw_search_device(None, P, 1, 1, None, P, P, None),
             lambda: lib.mi_pqw_info(None, None, None, None, None, None, None, None, None), lambda: lib.mi_pqw_get_codes(None, 0, 0, P),
             lambda: lib.mi_pqw_get_codebooks(None, P), lambda: lib.mi_pqw_decode(None, 0, 0, P)]
    for call in calls:
        assert call() == _lib.MI_ERR_INVALID
        assert b"null handle" in lib.mi_last_error()
    # what is checked behind the handle needs one: any non-null pointer will do, the refusal comes before it is read
    fake = C.c_void_p(buf.ctypes.data)
    for k in (0, 2049):
        assert lib.mi_pqw_search(fake, P, 1, _lib.MI_F32, 8, 1, k, None, 0, P, P, None) == _lib.MI_ERR_INVALID
        assert b"k must be in [1, 2048]" in lib.mi_last_error()
        assert lib.mi_pqw_search_device(fake, P, 1, k, None, P, P, None) == _lib.MI_ERR_INVALID
        assert b"k must be in [1, 2048]" in lib.mi_last_error()
    assert lib.mi_pqw_search(fake, None, 1, _lib.MI_F32, 8, 1, 1, None, 0, P, P, None) == _lib.MI_ERR_INVALID
    assert b"null pointer: queries" in lib.mi_last_error()
    assert lib.mi_pqw_search(fake, P, 1, _lib.MI_F32, 8, 1, 1, None, 0, None, P, None) == _lib.MI_ERR_INVALID
    assert b"null pointer: out_idx" in lib.mi_last_error()
    assert lib.mi_pqw_search(fake, P, 1, _lib.MI_F32, 8, 1, 1, P, 2, P, P, None) == _lib.MI_ERR_INVALID
    assert b"allow_memspace" in lib.mi_last_error()
    assert lib.mi_pqw_append_codes(fake, P, 1, 4, 2) == _lib.MI_ERR_INVALID
    assert b"memspace" in lib.mi_last_error()
    assert lib.mi_pqw_add(fake, P, 1, 2, 8, 1, _lib.MI_HOST) == _lib.MI_ERR_INVALID
    assert b"dtype" in lib.mi_last_error()


def test_train_answers_bad_arguments_without_a_device(built_lib):
    lib, _lib = built_lib
    P = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    x = np.random.default_rng(0).standard_normal((20, 8)).astype(np.float32)
    out = np.zeros((4, 16, 2), np.float32)

    def train(xp=P(x), n=20, d=8, dtype=_lib.MI_F32, rs=8, cs=1, memspace=_lib.MI_HOST, m=4, ks=16, iters=3, ip=None, op=P(out)):
        return lib.mi_pqw_train(xp, n, d, dtype, rs, cs, memspace, m, ks, iters, ip, 0, op, None, None)

    bad_rows = x.copy()
    bad_rows[19, 7] = np.nan
    cases = [(dict(xp=None), b"rows"), (dict(op=None), b"out_codebooks_host"), (dict(dtype=2), b"dtype"), (dict(memspace=2), b"memspace"),
             (dict(m=0), b"m (books)"), (dict(m=65, d=130), b"m (books)"), (dict(ks=1), b"[2, 8192]"), (dict(ks=8193), b"[2, 8192]"),
             (dict(ks=257), b"n >= ks"), (dict(d=0), b"d must be in"), (dict(m=3), b"multiple of m"), (dict(n=15), b"n >= ks"),
             (dict(iters=0), b"iters"), (dict(xp=P(bad_rows)), b"finite")]
    for kwargs, word in cases:
        assert train(**kwargs) == _lib.MI_ERR_INVALID, kwargs
        assert word in lib.mi_last_error(), (kwargs, lib.mi_last_error())
    # the byte entry point keeps its limit and its words
    assert lib.mi_pq_train(P(x), 300, 8, _lib.MI_F32, 8, 1, _lib.MI_HOST, 4, 257, 3, None, 0, P(out), None, None) == _lib.MI_ERR_INVALID
    assert b"[2, 256]" in lib.mi_last_error()


def _refuses(monkeypatch):
    from isehr_amd import _lib

    def no_device():
        raise AssertionError("the library was loaded: the refusal came too late")
    monkeypatch.setattr(_lib, "load", no_device)
    return _lib


def test_index_and_training_refuse_before_the_device(monkeypatch):
    _lib = _refuses(monkeypatch)
    W = _lib.WidePQIndex
    codes = np.zeros((3, 4), np.uint16)
    with pytest.raises(ValueError, match="Ks = 8193"):
        W.from_codes(np.zeros((4, 8193, 2), np.float32), codes)
    with pytest.raises(ValueError, match="Ks = 1 "):
        W.from_codes(np.zeros((4, 1, 2), np.float32), codes)
    with pytest.raises(ValueError, match="M = 65"):
        W.empty(np.zeros((65, 4, 1), np.float32), 10)
    with pytest.raises(ValueError, match="d = M \\* L = 4100"):
        W.empty(np.zeros((4, 4, 1025), np.float32), 10)
    with pytest.raises(ValueError, match="finite"):
        W.empty(np.full((4, 4, 2), np.inf, np.float32), 10)
    with pytest.raises(ValueError, match=r"\[0, Ks = 300\)"):
        W.from_codes(np.zeros((4, 300, 2), np.float32), codes + 300)
    with pytest.raises(ValueError, match="integer array"):
        W.from_codes(np.zeros((4, 300, 2), np.float32), codes.astype(np.float32))
    with pytest.raises(ValueError, match="needs a capacity"):
        W.empty(np.zeros((4, 300, 2), np.float32), 0)
    with pytest.raises(ValueError, match="capacity 2 below"):
        W.from_codes(np.zeros((4, 300, 2), np.float32), codes, capacity=2)
    with pytest.raises(ValueError, match="Ks = 257"):                   # the byte index's refusal, word for word
        _lib.PQIndex.from_codes(np.zeros((4, 257, 2), np.float32), codes)
    x = np.random.default_rng(1).standard_normal((40, 8)).astype(np.float32)
    with pytest.raises(ValueError, match="Ks = 8193"):
        _lib.pqw_train(np.zeros((9000, 8), np.float32), 4, 8193)
    with pytest.raises(ValueError, match="n = 40 training rows, Ks = 8192"):
        _lib.pqw_train(x, 4, 8192)
    with pytest.raises(ValueError, match="no multiple of M"):
        _lib.pqw_train(x, 3, 4)
    with pytest.raises(ValueError, match="iters = 0"):
        _lib.pqw_train(x, 4, 4, iters=0)
    with pytest.raises(ValueError, match="finite"):
        _lib.pqw_train(np.where(np.arange(8) == 3, np.nan, x), 4, 4)
    with pytest.raises(ValueError, match=r"\[M, Ks, L\]"):
        _lib.pqw_train(x, 4, 4, init=np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match="n = 3"):
        _lib.pqw_train_device(4096, 3, 8, 4, 300, 2)
    with pytest.raises(ValueError, match="no multiple of M"):
        W.fit(x, 3, 4)
    with pytest.raises(ValueError, match="Ks = 257"):                   # ... and the byte trainer's
        _lib.pq_train(np.zeros((300, 8), np.float32), 4, 257)


def test_wide_code_rows_keep_a_uint16_stride():
    from isehr_amd import _lib
    wide = np.full((5, 7), 0xFFFF, np.uint16)
    wide[:, :3] = 2
    a, stride = _lib.pq_code_rows(wide[:, :3], 3, 300, np.uint16)
    assert stride == 7 and a.ctypes.data == wide.ctypes.data
    a, stride = _lib.pq_code_rows(np.full((5, 3), 299, np.int64), 3, 300, np.uint16)
    assert a.dtype == np.uint16 and stride == 3 and int(a.max()) == 299
    a, stride = _lib.pq_code_rows(np.zeros((5, 3), np.uint8), 3, 256)                      # the byte form is what it was
    assert a.dtype == np.uint8 and stride == 3


def test_matcher_is_registered_with_the_reference_s_defaults():
    from isehr_amd import nnsearch
    from isehr_amd.nnsearch import matching_Nano_PQ_hip, matching_Nano_PQ_wide_hip
    assert nnsearch.MATCHING_METHODS["PQ13"] is matching_Nano_PQ_wide_hip
    assert nnsearch.MATCHING_METHODS["PQ"] is matching_Nano_PQ_hip
    params = inspect.signature(matching_Nano_PQ_wide_hip).parameters
    assert list(params) == ["K", "embedded_features_train", "embedded_features_test", "dataset", "N_books", "n_bits_perbook", "ifgenerate"]
    assert (params["N_books"].default, params["n_bits_perbook"].default) == (16, 13)
    assert params["dataset"].default is None and params["ifgenerate"].default is True
    assert inspect.signature(matching_Nano_PQ_hip).parameters["n_bits_perbook"].default == 8


def test_matcher_refuses_before_the_device(monkeypatch, tmp_path):
    _refuses(monkeypatch)
    from isehr_amd.nnsearch import matching_Nano_PQ_wide_hip as match
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(2)
    train = rng.standard_normal((40, 8)).astype(np.float32)
    test = rng.standard_normal((3, 8)).astype(np.float32)
    for bits in (0, 14):
        with pytest.raises(ValueError, match="n_bits_perbook = %d" % bits):
            match(2, train, test, None, 4, bits)
    with pytest.raises(ValueError, match="n = 40 training rows, Ks = 8192"):
        match(2, train, test, None, 4)                                   # the default: 13 bits
    with pytest.raises(ValueError, match="n = 40 training rows, Ks = 512"):
        match(2, train, test, None, 4, 9)
    with pytest.raises(ValueError, match="no multiple of M"):
        match(2, train, test, None, 3, 2)
    with pytest.raises(ValueError, match="K = 0"):
        match(0, train, test, None, 4, 2)
    with pytest.raises(ValueError, match="K = 41"):
        match(41, train, test, None, 4, 2)
    with pytest.raises(ValueError, match="K <= 2048"):
        match(2049, np.ones((3000, 8), np.float32), test, None, 4, 2)
    with pytest.raises(ValueError, match="finite and non-zero"):
        match(2, np.where(np.arange(8) == 3, np.inf, train), test, None, 4, 2)
    with pytest.raises(ValueError, match="finite and non-zero"):
        match(2, train, np.zeros((3, 8), np.float32), None, 4, 2)
    with pytest.raises(ValueError, match="expected rows"):
        match(2, train, test[:, :4], None, 4, 2)
    with pytest.raises(ValueError, match="give one"):
        match(2, train, test, None, 4, 2, ifgenerate=False)
    with pytest.raises(FileNotFoundError):
        match(2, train, test, "never/generated", 4, 2, ifgenerate=False)
    assert not os.path.exists(tmp_path / "outputs")
    # a stored codebook file of another shape: the byte matcher's file does not serve, and a wide file of another L is refused
    from isehr_amd import nnsearch
    path = nnsearch._pq_books_path("some/set", 4, 4, "mi355_pqw")
    assert os.path.basename(path) == "mi355_pqw_M4_Ks4.npz" and os.path.basename(nnsearch._pq_books_path("some/set", 4, 4)) == "mi355_pq_M4_Ks4.npz"
    os.makedirs(os.path.dirname(path))
    np.savez(path, codebooks=np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match="stored codebooks of shape"):
        match(2, train, test, "some/set", 4, 2, ifgenerate=False)
