"""GPU: the scatter-matrix kernel (csrc/scatter.hip) against float64 numpy, and the whitening learners built on it
(whiten.pcawhitenlearn_hip / whitenlearn_hip) against the reference's own outputs (tests/golden/whitenlearn.npz, written by
scripts/make_whitenlearn_golden.py).

Bounds.  Every entry of the scatter matrix is a length-n float64 dot product, so for ANY summation order
|C_ij - ref_ij| <= 2 n u sqrt(C_ii C_jj), u = 2^-53 (Cauchy-Schwarz on the standard dot-product error bound).  The learners
are allowed 16 x the distance the fixture stores between the reference and a second correct float64 CPU implementation that
sums in another order (floor 1e-13): the device sums in yet another order, and one order of magnitude covers that and nothing
else."""
import os
import pickle
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _whitenlearn_inputs as wi  # noqa: E402
from _whiten_truth import U, DevScatter, _check, _ref_scatter, _torch  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from isehr_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "whitenlearn.npz")))


def _layouts(x):
    """The same [n, d] values as a row-major tensor, as the reference's [D, N] array seen as .T, and as a general-stride view."""
    torch = _torch()
    t = torch.from_numpy(x).cuda()
    wide = torch.zeros((x.shape[0], 2 * x.shape[1]), dtype=t.dtype, device="cuda")
    wide[:, ::2] = t
    return {"rows": t, "DN": t.t().contiguous().t(), "strided": wide[:, ::2]}


# ---- 1. scatter matrix against float64 numpy -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", [24, 64, 200, 2048])
def test_scatter_matches_float64_numpy(lib, d, dtype):
    from isehr_amd.synth import synth_rows
    dev = DevScatter(lib, d)
    worst = 0.0
    for n in (1, 15, 16, 129, 5000):
        x = synth_rows(100 + d, 0, n, d).astype(dtype)
        x = np.abs(x) if n % 2 else x                      # non-negative rows too: where x x^T - n c c^T would cancel
        centre = x.astype(np.float64).mean(axis=0) + 0.01
        lay = _layouts(x)
        for cen in (None, centre):
            ref = _ref_scatter(x, cen)
            first = None
            for name, t in lay.items():
                what = "d=%d n=%d %s %s centre=%s" % (d, n, np.dtype(dtype).name, name, cen is not None)
                C = dev(t, cen).cpu().numpy()
                worst = max(worst, _check(C, ref, n, what))
                again = dev(t, cen).cpu().numpy()
                assert np.array_equal(C, again), what + ": two calls differ"
                if first is None:
                    first = C
    print("scatter d=%d %s: largest |C - ref| / (2 n u sqrt(C_ii C_jj)) = %.2e" % (d, np.dtype(dtype).name, worst))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_scatter_pairs_mode(lib, dtype):
    from isehr_amd.synth import synth_rows
    worst = 0.0
    for d, n, npairs in ((64, 300, 1), (200, 500, 1000), (2048, 700, 333)):
        dev = DevScatter(lib, d)
        x = synth_rows(5, 0, n, d).astype(dtype)
        rng = np.random.default_rng(d)
        q = rng.integers(0, n, npairs)
        p = rng.integers(0, n, npairs)
        q[: npairs // 3] = q[0]                              # repeated indices
        p[npairs // 2:: 7] = q[npairs // 2:: 7]              # q == p: a zero difference
        df = x[q].astype(np.float64) - x[p].astype(np.float64)
        ref = df.T @ df
        for name, t in _layouts(x).items():
            C = dev(t, None, (q, p)).cpu().numpy()
            worst = max(worst, _check(C, ref, npairs, "pairs d=%d %s" % (d, name)))
            assert np.array_equal(C, dev(t, None, (q, p)).cpu().numpy())
        # the host entry point moves only the named rows
        Ch = lib.scatter_matrix(x, pairs=(q, p))
        worst = max(worst, _check(Ch, ref, npairs, "pairs host d=%d" % d))
        Ch = lib.scatter_matrix(np.asfortranarray(x), pairs=(q, p))
        worst = max(worst, _check(Ch, ref, npairs, "pairs host [D,N] d=%d" % d))
    print("pairs %s: largest ratio to the bound = %.2e" % (np.dtype(dtype).name, worst))
    with pytest.raises(RuntimeError, match="pair index"):
        lib.scatter_matrix(x, pairs=(np.array([0, n]), np.array([0, 1])))


def test_scatter_accumulate_over_uneven_blocks(lib):
    from isehr_amd.synth import synth_rows
    torch = _torch()
    d = 200
    dev = DevScatter(lib, d)
    x = synth_rows(9, 0, 1000 + 37 + 4001, d)
    centre = x.astype(np.float64).mean(axis=0)
    t = torch.from_numpy(x).cuda()
    C = None
    for r0, r1 in ((0, 1000), (1000, 1037), (1037, x.shape[0])):
        C = dev(t[r0:r1], centre, into=C)
    ref = _ref_scatter(x, centre)
    r = _check(C.cpu().numpy(), ref, x.shape[0], "accumulate")
    one = dev(t, centre).cpu().numpy()
    _check(one, ref, x.shape[0], "one call")
    print("accumulate over 3 uneven blocks: ratio %.3f; max |blocks - one call| = %.3e" %
          (r, np.max(np.abs(C.cpu().numpy() - one))))


@pytest.mark.parametrize("order", ["C", "F"])
def test_scatter_host_streaming(lib, order):
    from isehr_amd.synth import synth_rows
    d, n = 200, 2500
    x = synth_rows(12, 0, n, d).astype(np.float64 if order == "F" else np.float32)
    x = np.asfortranarray(x) if order == "F" else x
    centre = x.astype(np.float64).mean(axis=0)
    ref = _ref_scatter(x, centre)
    lib.set_global_option("scatter_block_rows", 700)        # 4 blocks, the last one short
    try:
        assert lib.get_global_option("scatter_block_rows") == 700
        C = lib.scatter_matrix(x, centre=centre)
        again = lib.scatter_matrix(x, centre=centre)
    finally:
        lib.set_global_option("scatter_block_rows", 0)
    r = _check(C, ref, n, "host streaming " + order)
    assert np.array_equal(C, again)
    whole = lib.scatter_matrix(x, centre=centre)
    _check(whole, ref, n, "host one block " + order)
    gen = lib.scatter_matrix(x[:, ::2], centre=centre[::2])
    _check(gen, ref[::2, ::2], n, "host general strides " + order)
    print("host streaming (%s order, 4 blocks): ratio %.3f" % (order, r))


# ---- 2. / 3. the learners against the reference's own outputs ----------------------------------------------------------
CASES = [(k, t) for k in wi.KINDS for t in ("f64", "f32")]


def _allow(golden, key):
    return max(16.0 * float(golden[key]), 1e-13)


@pytest.fixture(scope="module")
def learned(lib, golden):
    """Every case once, through the host path (numpy [D, N], both memory orders) and the device path (CUDA tensor)."""
    from isehr_amd import whiten
    torch = _torch()
    out = {}
    for kind, dt in CASES:
        X64, q, p = wi.make_input(kind, int(golden["seed"]))
        X = wi.as_dtype(X64, dt)
        out[kind, dt] = {
            "X": X, "q": q, "p": p,
            "host": (whiten.pcawhitenlearn_hip(X), whiten.whitenlearn_hip(np.asfortranarray(X), q, p)),
            "device": (whiten.pcawhitenlearn_hip(torch.from_numpy(X).cuda()),
                       whiten.whitenlearn_hip(torch.from_numpy(X).cuda(), q, p)),
        }
    return out


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("kind,dt", CASES)
def test_learners_match_the_reference(golden, learned, kind, dt, path):
    case = learned[kind, dt]
    X = case["X"]
    pre = "%s_%s_" % (kind, dt)
    for tag, (m, P) in zip(("pca", "sup"), case[path]):
        m_ref, P_ref = golden[pre + "m_" + tag], golden[pre + "P_" + tag]
        assert m.shape == m_ref.shape and P.shape == P_ref.shape and m.dtype == np.float64 and P.dtype == np.float64
        m_err = float(np.max(np.abs(m - m_ref)))
        assert m_err <= 4 * X.shape[1] * U * float(np.max(np.abs(X))), (tag, m_err)
        dr, dg = wi.rows_distance(P, P_ref), wi.gram_distance(P, P_ref)
        print("%s %s %s %s: m err %.2e; rows %.3e (stored CPU distance %.3e), P.T P %.3e (stored %.3e)" %
              (kind, dt, path, tag, m_err, dr, float(golden[pre + "dev_rows_" + tag]), dg, float(golden[pre + "dev_gram_" + tag])))
        assert dr <= _allow(golden, pre + "dev_rows_" + tag), (tag, dr)
        assert dg <= _allow(golden, pre + "dev_gram_" + tag), (tag, dg)


@pytest.mark.parametrize("kind,dt", CASES)
def test_whitened_descriptors_agree_with_the_reference_pair(golden, learned, kind, dt):
    from isehr_amd import whiten
    case = learned[kind, dt]
    X = case["X"]
    pre = "%s_%s_" % (kind, dt)
    for tag, (m, P) in zip(("pca", "sup"), case["device"]):
        m_ref, P_ref = golden[pre + "m_" + tag], golden[pre + "P_" + tag]
        for dims in (wi.D, 16):
            G = wi.whitened_gram(whiten.whitenapply_hip(X, m, P, dims))
            G_ref = wi.whitened_gram(whiten.whitenapply_hip(X, m_ref, P_ref, dims))
            dist = float(np.max(np.abs(G - G_ref)))
            key = pre + "dev_whitened_gram_%s_%d" % (tag, dims)
            compared, differ, left_out = wi.top10_sets(G, G_ref)
            print("%s %s %s dims %d: whitened Gram distance %.3e (stored %.3e); top-10 sets differ on %d of %d columns, "
                  "%.2f %% left out by the guard" % (kind, dt, tag, dims, dist, float(golden[key]), differ, compared, 100 * left_out))
            assert dist <= _allow(golden, key)
            assert left_out <= 0.01
            assert differ == 0


# ---- 4. whitening property at size ---------------------------------------------------------------------------------------
def test_whitening_property_at_size(lib):
    from isehr_amd import whiten
    torch = _torch()
    n, d = 200000, 2048
    x = torch.empty((n, d), dtype=torch.float32, device="cuda")
    lib.synth_fill_device(x.data_ptr(), 21, 0, n, d)
    torch.cuda.synchronize()
    scales = torch.logspace(0, -1.5, d, device="cuda", dtype=torch.float32)
    x.mul_(scales[None, :]).add_(0.25)                    # anisotropic, non-zero mean
    torch.cuda.synchronize()
    ws_bytes = lib.scatter_workspace_bytes(d)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    free0 = torch.cuda.mem_get_info()[0]
    m, P = whiten.pcawhitenlearn_hip(x.t())               # [D, N] view of the device rows: read in place
    peak = torch.cuda.max_memory_allocated() - base
    lib_delta = free0 - torch.cuda.mem_get_info()[0]      # what the library (or the caching allocator) still holds
    budget = ws_bytes + 4 * d * d * 8
    print("learner device memory: torch peak %.1f MiB, free-memory delta %.1f MiB, budget (workspace + 4 d^2 doubles) %.1f MiB"
          % (peak / 2 ** 20, lib_delta / 2 ** 20, budget / 2 ** 20))
    assert peak <= budget and lib_delta <= budget + (64 << 20)      # + the caching allocator's block rounding
    assert peak < n * d * 8 // 4                           # nowhere near an N x D float64 array
    ev = 1.0 / np.sum(P * P, axis=1)                       # eigenvalues the learner saw (rows of P have norm eigval^-1/2)
    cond = float(ev.max() / ev.min())
    md, Pd = torch.from_numpy(m.reshape(-1)).cuda(), torch.from_numpy(np.ascontiguousarray(P)).cuda()
    C = torch.zeros((d, d), dtype=torch.float64, device="cuda")
    dev = DevScatter(lib, d)
    step = 50000
    y = torch.empty((step, d), dtype=torch.float64, device="cuda")
    for r0 in range(0, n, step):
        lib.whiten_apply_device(x[r0:r0 + step].data_ptr(), step, d, md.data_ptr(), Pd.data_ptr(), d, y.data_ptr(), eps=-1.0,
                                stream=torch.cuda.current_stream().cuda_stream)
        C = dev(y, None, into=C) if r0 else dev(y, None)
    I = (C / n).cpu().numpy()
    err = float(np.max(np.abs(I - np.eye(d))))
    tol = 64 * cond * d * U
    print("whitening property: max |C / N - I| = %.3e, allowed 64 cond d u = %.3e (cond %.1f)" % (err, tol, cond))
    assert err <= tol


# ---- 5. gallery scatter, learn_whitening -> main_retrieve ---------------------------------------------------------------
def test_gallery_scatter(lib):
    from isehr_amd.synth import synth_rows
    n, d = 3000, 200
    g = lib.Gallery.from_host(np.abs(synth_rows(3, 0, n, d)), norm_mode=lib.NORM_L2)
    try:
        rows = g.get_rows(0, n)
        centre = rows.astype(np.float64).mean(axis=0)
        for cen in (None, centre):
            r = _check(g.scatter(cen), _ref_scatter(rows, cen), n, "gallery scatter")
            print("gallery scatter centre=%s: ratio %.3f" % (cen is not None, r))
    finally:
        g.close()


def test_learn_whitening_feeds_main_retrieve(tmp_path, monkeypatch, capsys):
    """entry/learn_whitening -> Lw.pkl -> entry/main_retrieve --whitening, on a planted dataset laid out like the one the
    main_retrieve driver test builds."""
    from isehr_amd import _lib, whiten
    from isehr_amd.entry import learn_whitening, main_retrieve
    from isehr_amd.synth import planted_dataset
    monkeypatch.chdir(tmp_path)
    d, n, nq = 64, 3000, 10
    vecs, qvecs, gnd = planted_dataset(79, n, d, nq)
    os.makedirs("outputs", exist_ok=True)
    os.makedirs("data/test/rparis6k", exist_ok=True)
    np.save("outputs/rparis6k_vecs.npy", vecs)
    np.save("outputs/rparis6k_qvecs.npy", qvecs)
    with open("data/test/rparis6k/gnd_rparis6k.pkl", "wb") as f:
        pickle.dump({"gnd": gnd, "imlist": ["im%d" % i for i in range(n)], "qimlist": ["q%d" % i for i in range(nq)]}, f)
    qi = [int(g["easy"][0]) for g in gnd if len(g["easy"]) >= 2] + [int(g["hard"][0]) for g in gnd if len(g["hard"]) >= 2]
    pi = [int(g["easy"][1]) for g in gnd if len(g["easy"]) >= 2] + [int(g["hard"][1]) for g in gnd if len(g["hard"]) >= 2]
    with open("db.pkl", "wb") as f:
        pickle.dump({"qidxs": qi, "pidxs": pi}, f)
    assert learn_whitening.main(["--features", "outputs/rparis6k_vecs.npy", "--out", "Lw.pkl"]) == 0
    assert learn_whitening.main(["--features", "outputs/rparis6k_vecs.npy", "--pairs", "db.pkl", "--out", "Lw_sup.pkl"]) == 0
    g = _lib.Gallery.from_host(vecs.T, norm_mode=_lib.NORM_L2)
    g.save("rparis6k.gal")
    g.close()
    assert learn_whitening.main(["--gallery", "rparis6k.gal", "--out", "Lw_gal.pkl"]) == 0
    out = capsys.readouterr().out
    assert out.count("factorisation") == 3 and "scatter" in out, out
    Lw = {}
    for name in ("Lw.pkl", "Lw_sup.pkl", "Lw_gal.pkl"):
        with open(name, "rb") as f:
            Lw[name] = pickle.load(f)
        assert Lw[name]["m"].shape == (d, 1) and Lw[name]["P"].shape == (d, d) and np.all(np.isfinite(Lw[name]["P"]))
    m, P = whiten.pcawhitenlearn_hip(vecs)
    # the driver is the function (the mean is a float64 sum whose order is not fixed: 4 N u max|X| each)
    assert np.max(np.abs(Lw["Lw.pkl"]["m"] - m)) <= 8 * n * U * float(np.max(np.abs(vecs)))
    assert wi.gram_distance(Lw["Lw.pkl"]["P"], P) <= 1e-9
    assert main_retrieve.main(["--datasets", "rparis6k", "--whitening", "Lw.pkl"]) == 0
    lines = capsys.readouterr().out.splitlines()
    map_lines = [ln for ln in lines if "mAP E:" in ln]
    assert len(map_lines) == 2 and "rparis6k + whiten" in map_lines[1]
    print("\n".join(map_lines))


# ---- 6. degenerate input -----------------------------------------------------------------------------------------------
def test_degenerate_inputs(lib):
    from isehr_amd import whiten
    from isehr_amd.synth import synth_rows
    d = 48
    X = synth_rows(2, 0, d, d).astype(np.float64).T          # N == D: the centred data has rank <= D - 1
    with pytest.raises(ValueError, match="eigenvalues of the covariance are not positive"):
        whiten.pcawhitenlearn_hip(X)
    Xc = synth_rows(2, 0, 500, d).astype(np.float64).T
    Xc[5] = 0.75                                           # a constant coordinate
    with pytest.raises(ValueError, match="1 of 48"):
        whiten.pcawhitenlearn_hip(Xc)
    # three pairs in 48 dimensions: S has rank 3, the jitter rule makes it positive definite
    X = synth_rows(4, 0, 600, d).astype(np.float64).T
    m, P = whiten.whitenlearn_hip(X, [0, 1, 2], [3, 4, 5])
    assert m.shape == (d, 1) and P.shape == (d, d) and np.all(np.isfinite(P))
