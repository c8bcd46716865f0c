"""GPU: the truncated graph diffusion (csrc/diffusion.hip, mi_diffusion_* in csrc/api_aux.hip) pinned to float64 on every
row and edge.  The graph and the solve are checked apart: the kNN lists the device diffused on are checked against
float64 scores, and the reference Laplacian and solves are then computed from those very lists (oracle.diffusion_solve_nodes,
itself pinned to scipy's cg and the reference's recorded solve in test_diffusion_reference_cpu.py), so that no row is
excused by a near-tie.  The online half is compared with the plain float64 combination under a derived rounding bound.
The only conditions are on the inputs, each asserted: distance of the reference residuals from tol, presence of
self-loop rows, of negative similarities, of an isolated node and of both exits of the CG loop."""
import numpy as np
import pytest

from _diffusion_checks import (SCORE_TOL, check_graph, check_offline_rows, check_online, clustered)
from isehr_amd.synth import synth_rows

pytestmark = pytest.mark.gpu


def _gallery(f):
    from isehr_amd._lib import Gallery, NORM_NONE
    return Gallery.from_host(f, norm_mode=NORM_NONE)


def _offline_all_rows(f, T, kd, label="", **params):
    """features -> device graph checked -> every row compared.  -> (ids, sims, vals, reference iteration counts)."""
    G = _gallery(f)
    try:
        ids, vals, sims = G.diffusion_offline(T, kd, return_sims=True, **params)
    finally:
        G.close()
    check_graph(f, ids, sims)
    _, its, xs = check_offline_rows(ids, sims, vals, kd, np.arange(len(f)), label=label, **params)
    return ids, sims, vals, its, xs


def _offline_node_ranges(f, T, kd, ranges, label="", **params):
    G = _gallery(f)
    try:
        for lo, hi in ranges:
            ids, vals, sims = G.diffusion_offline_nodes(T, kd, lo, hi, return_sims=True, **params)
            if lo == ranges[0][0]:
                check_graph(f, ids, sims)
                ids0, sims0 = ids, sims
            else:
                assert np.array_equal(ids, ids0) and np.array_equal(sims, sims0)
            check_offline_rows(ids, sims, vals, kd, np.arange(lo, hi), label="%s [%d,%d)" % (label, lo, hi), **params)
    finally:
        G.close()


def _self_loop_rows(ids, kd):
    """Nodes that are not their own nearest neighbour but appear later within their first kd columns: the rows whose
    affinity has a self entry, which laplacian_kernel folds into diag[i]."""
    me = np.arange(len(ids))[:, None]
    return np.flatnonzero((ids[:, 0] != me[:, 0]) & (ids[:, 1:kd] == me).any(axis=1))


# ------------------------------------------------------------------------------------------------ offline
@pytest.mark.parametrize("T", [2, 63, 64, 65, 255, 256, 257])
def test_offline_every_row_at_the_edges_of_n_trunc_and_kd(T):
    n = max(T + 37, 300)
    f = clustered(21 + T, n, 48)
    for kd in sorted({1, 2, T // 3, T} - {0}):
        ids, sims, vals, its, xs = _offline_all_rows(f, T, kd)
        assert (ids[:, 0] == np.arange(n)).all()           # distinct unit rows: every node heads its own list
        if kd == 1:                                        # position 0 is always dropped: L = I, x = e0 exactly
            assert (vals[:, 0] == 1).all() and not vals[:, 1:].any()
        else:
            assert np.abs(xs[:, 1:]).max() > 1e-3          # a real diffusion, not the identity


def test_offline_n_trunc_1000_on_node_ranges():
    n, T = 1100, 1000
    f = clustered(33, n, 64)
    for kd in (1, 2, T // 3, T):
        _offline_node_ranges(f, T, kd, [(0, 16), (500, 524), (1090, 1100)])


def test_offline_duplicated_rows_fold_the_self_entry_into_the_diagonal():
    n, T, kd = 600, 128, 24
    f = clustered(41, n, 32)
    src = np.arange(40) * 7
    f[300 + np.arange(40)] = f[src]                        # 40 rows twice ...
    f[400 + np.arange(12)] = f[src[:12]]                   # ... 12 of them three times
    ids, sims, vals, its, xs = _offline_all_rows(f, T, kd, label="duplicates")
    loops = _self_loop_rows(ids, kd)
    assert len(loops) >= 52, len(loops)                    # every later copy lists an earlier one first, itself after
    assert set(loops.tolist()) >= set(range(300, 340)) | set(range(400, 412))
    # b = e0 is the first-listed node: the solution's head belongs to ids[i, 0], not to i
    assert (xs[loops, 0] > 0.5).all()


def test_offline_unnormalised_rows():
    """Every third row scaled to a norm in (0.1, 1]: a scaled row is led by a longer row of its cluster, and those scaled
    little enough still list themselves within the first kd columns.  (The reference drops position 0 whoever stands
    there, so its Laplacian is not symmetric on such data; with all rows scaled its solutions reach 1e5 and no float32
    result can hold 5e-6.  Here they stay below 4.)"""
    n, T, kd = 700, 160, 40
    f = clustered(343, n, 32, k=8).astype(np.float64)
    u = synth_rows(344, 0, n, 1).astype(np.float64)[:, 0] * 0.37 % 1.0
    f = (f * np.where(np.arange(n) % 3 == 0, 10.0 ** -u, 1.0)[:, None]).astype(np.float32)
    norms = np.linalg.norm(f, axis=1)
    assert norms.max() / norms.min() > 8
    ids, sims, vals, its, xs = _offline_all_rows(f, T, kd, label="un-normalised")
    loops = _self_loop_rows(ids, kd)                       # the self-loop path, here without exact ties
    assert len(loops) >= 10, len(loops)
    assert np.abs(xs).max() < 8


def _hemisphere(seed, n):
    """Unit rows in 3-d, weakly clustered, all on the side x . c > 0 of one direction c, and one row at -c: pairs more
    than a right angle apart are common (negative similarities inside the lists), and the row at -c has a negative
    similarity with every other row."""
    c = np.array([0.6, -0.48, 0.64])
    g = synth_rows(seed, 0, n, 3).astype(np.float64) + 0.6 * synth_rows(seed + 1, 0, 6, 3).astype(np.float64)[np.arange(n) % 6]
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g[g @ c < 0] *= -1
    g += 0.15 * c
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    g[n // 2] = -c
    return g.astype(np.float32)


def test_offline_negative_similarities_and_an_isolated_node():
    n, T = 500, 460
    kd = T
    f = _hemisphere(47, n)
    ids, sims, vals, its, xs = _offline_all_rows(f, T, kd, label="negative sims")
    share = (sims[:, :kd] < 0).mean()
    assert share > 0.10, share                             # the clamp of affinity_kernel decides many entries
    lone = n // 2
    assert ids[lone, 0] == lone and (sims[lone, 1:] < 0).all()
    assert vals[lone, 0] == 1 and not vals[lone, 1:].any()      # no mutual neighbour with weight: x = e0 exactly
    assert np.array_equal(xs[lone], np.eye(T)[0])


def test_offline_at_the_maximum_n_trunc():
    """n_trunc = 4096: 36 bytes of dynamic LDS per column, 147 520 bytes of the 160 KiB; N above the 1024-query block of
    dense_search_device; node ranges at the start, across a multiple of the grid size 512, and at the end."""
    n, T, kd = 4200, 4096, 200
    f = clustered(51, n, 32, k=20)
    _offline_node_ranges(f, T, kd, [(0, 5), (509, 515), (4195, 4200)], label="max n_trunc")
    G = _gallery(f)
    try:
        with pytest.raises(RuntimeError):
            G.diffusion_offline_nodes(4097, kd, 0, 1)
    finally:
        G.close()


def test_offline_other_parameters_and_both_exits_of_the_cg_loop():
    n, T, kd = 300, 200, 40
    f = clustered(61, n, 24, noise=0.8, pull=1.1)          # the rows of tests/golden/diffusion_solve.npz
    default = dict(alpha=0.99, gamma=3, maxiter=20, tol=1e-6)
    on_tol = on_maxiter = 0
    exits = {}
    for change in (dict(gamma=1), dict(gamma=2), dict(alpha=0.5), dict(alpha=0.999), dict(maxiter=1), dict(maxiter=5),
                   dict(maxiter=200), dict(tol=1e-3), dict(tol=1e-10), dict()):
        p = dict(default, **change)
        ids, sims, vals, its, xs = _offline_all_rows(f, T, kd, label=str(change), **p)
        on_tol += int((its < p["maxiter"]).sum())
        on_maxiter += int((its == p["maxiter"]).sum())
        exits[str(change)] = (int((its < p["maxiter"]).sum()), int((its == p["maxiter"]).sum()))
        if change == dict(maxiter=200):
            assert (its < 200).all() and its.max() > 20      # converges, past the default limit
    print("CG exits per case (on tol, on maxiter):", exits)
    assert exits[str(dict())][0] > 0 and exits[str(dict())][1] > 0      # the default parameters alone take both exits
    assert on_tol > 0 and on_maxiter > 0, (on_tol, on_maxiter)


def test_offline_node_ranges_bit_for_bit():
    """Any partition of the nodes gives the rows of the full call bit for bit: ends that are no multiples of the grid
    size 512, a range of one node at N - 1, an empty range."""
    n, d, T, kd = 1203, 40, 200, 32
    f = clustered(61, n, d, k=25, noise=0.7, pull=1.1)
    G = _gallery(f)
    try:
        ids, vals = G.diffusion_offline(T, kd)
        for cuts in ((0, 513, 700, 700, 1202, 1203), (0, 1, 511, 1025, 1203)):
            parts = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                pid, pv = G.diffusion_offline_nodes(T, kd, lo, hi)
                assert np.array_equal(pid, ids) and pv.shape == (hi - lo, T)
                parts.append(pv)
            assert np.array_equal(np.concatenate(parts), vals)
        pid, pv = G.diffusion_offline_nodes(T, kd, n - 1, n)
        assert np.array_equal(pv[0], vals[n - 1])
    finally:
        G.close()


# ------------------------------------------------------------------------------------------------ online
_N, _D, _T, _KD = 900, 48, 200, 40


def _positive_clustered(seed, n, d):
    """Clustered unit rows with a common component: every pair has a clearly positive similarity, so the negated rows
    have a clearly negative similarity to all their neighbours."""
    f = clustered(seed, n, d).astype(np.float64) + 0.8 * synth_rows(seed + 5, 0, 1, d).astype(np.float64) / np.sqrt(d)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return f.astype(np.float32)


@pytest.fixture(scope="module")
def installed():
    """A gallery with the offline result it computed itself, and that result read back."""
    f = _positive_clustered(71, _N, _D)
    G = _gallery(f)
    ids, vals, sims = G.diffusion_offline(_T, _KD, return_sims=True)
    check_graph(f, ids, sims)
    check_offline_rows(ids, sims, vals, _KD, np.arange(_N), label="online fixture")
    yield G, f, ids, vals
    G.close()


def _queries(seed, nq, d, f):
    """Perturbed gallery rows, un-normalised (the queries are used as given)."""
    base = f[(np.arange(nq) * 37) % len(f)].astype(np.float64)
    q = base + 0.25 * synth_rows(seed, 0, nq, d).astype(np.float64) / np.sqrt(d)
    return q.astype(np.float32)


@pytest.mark.parametrize("kq,nq,trunc", [(3, 70, _T), (1, 1, 1), (50, 129, _T // 2), (3, 300, _N - 1), (1, 300, _T),
                                         (50, 1, _N - 1), (3, 129, 1)])
def test_online_scores_and_ranks(installed, kq, nq, trunc):
    G, f, ids, vals = installed
    q = _queries(100 + kq + nq, nq, _D, f)
    ranks, scores = G.diffusion_online(q, kq, 3, trunc)
    check_online(G, f, ids, vals, q, kq, 3, trunc, ranks, scores)


def test_online_float64_and_strided_queries(installed):
    G, f, ids, vals = installed
    q = _queries(131, 70, _D, f)
    r0, s0 = G.diffusion_online(q, 3, 3, _T)
    q64 = q.astype(np.float64) * (1 + 2.0 ** -30)          # not representable in float32
    r1, s1 = G.diffusion_online(q64, 3, 3, _T)
    check_online(G, f, ids, vals, q64, 3, 3, _T, r1, s1, label="float64")
    qt = np.asfortranarray(q)                              # element (i, j) at j * nq + i: a transposed view
    assert qt.strides == (4, 4 * 70)
    r2, s2 = G.diffusion_online(qt, 3, 3, _T)
    check_online(G, f, ids, vals, qt, 3, 3, _T, r2, s2, label="strided")
    assert np.array_equal(r2, r0) and np.array_equal(s2, s0)
    qv = np.ascontiguousarray(q.T).T[::2]                  # every other query of a [D, nq] array
    assert qv.strides == (8, 4 * 70)
    r3, s3 = G.diffusion_online(qv, 3, 3, _T)
    check_online(G, f, ids, vals, qv, 3, 3, _T, r3, s3, label="strided, every other")


@pytest.mark.parametrize("gamma", [3, 2])
def test_online_negative_query_similarities(installed, gamma):
    """An odd gamma keeps the sign of a query similarity (unlike the affinity, which clamps): the reached columns score
    below the exact zeros of the unreached ones."""
    G, f, ids, vals = installed
    q = -f[::13][:60]
    s = q.astype(np.float64) @ f.astype(np.float64).T
    assert s.max() < -0.02                                 # negative to every row, away from zero
    ranks, scores = G.diffusion_online(q, 3, gamma, _N - 1)
    check_online(G, f, ids, vals, q, 3, gamma, _N - 1, ranks, scores, label="negated rows")
    # at most 3 * T columns are reached: the rest are exact zeros (their order, ascending id, is checked above)
    assert ((scores == 0).sum(axis=1) >= _N - 1 - 3 * _T).all()
    if gamma == 3:
        assert (scores.min(axis=1) < 0).all()


def test_online_overlapping_and_disjoint_neighbour_rows(installed):
    G, f, ids, vals = installed
    # queries from inside one cluster: their neighbours' offline rows overlap heavily
    members = np.flatnonzero(np.arange(_N) % 12 == 5)[:40]
    q = (f[members].astype(np.float64) + 0.1 * synth_rows(141, 0, 40, _D).astype(np.float64) / np.sqrt(_D)).astype(np.float32)
    didx, _, _ = G.search(q, 3)
    overlap = np.mean([len(set(ids[a]) & set(ids[b])) / _T for a, b, _ in didx])
    assert overlap > 0.5, overlap
    ranks, scores = G.diffusion_online(q, 3, 3, _T)
    check_online(G, f, ids, vals, q, 3, 3, _T, ranks, scores, label="overlapping rows")
    # a synthetic offline result on a fresh handle: short windows of ids, so that the rows of neighbours are disjoint;
    # signed values; trunc differs from the installed n_trunc
    t = 8
    sid = (np.arange(_N)[:, None] + np.arange(t)[None, :]) % _N
    sval = synth_rows(142, 0, _N, t)
    G2 = _gallery(f)
    try:
        G2.diffusion_set_offline(sid, sval)
        didx, _, _ = G2.search(q, 3)
        for row in didx:
            cols = sid[row].ravel()
            assert len(set(cols.tolist())) == 3 * t        # disjoint
        for trunc in (1, 5, 24, 25, 600, _N - 1):
            ranks, scores = G2.diffusion_online(q, 3, 3, trunc)
            check_online(G2, f, sid, sval, q, 3, 3, trunc, ranks, scores, label="disjoint rows")
    finally:
        G2.close()


def test_online_argument_errors(installed):
    G, f, ids, vals = installed
    q = _queries(151, 4, _D, f)
    for trunc in (_N, 4097, 0):
        with pytest.raises(RuntimeError):
            G.diffusion_online(q, 3, 3, trunc)
    fresh = _gallery(f)
    try:
        with pytest.raises(RuntimeError, match="no offline"):
            fresh.diffusion_online(q, 3, 3, 10)
    finally:
        fresh.close()
    fb = clustered(153, 4300, 16)
    sid = np.tile(np.arange(4, dtype=np.int64), (4300, 1))
    big = _gallery(fb)
    try:
        big.diffusion_set_offline(sid, np.ones((4300, 4), np.float32))
        with pytest.raises(RuntimeError):
            big.diffusion_online(q[:, :16], 3, 3, 4097)
        r, s = big.diffusion_online(q[:, :16], 3, 3, 4096)      # min(N - 1, 4096) is legal
        check_online(big, fb, sid, np.ones((4300, 4), np.float32), q[:, :16], 3, 3, 4096, r, s, label="trunc 4096")
    finally:
        big.close()


def test_set_offline_round_trip_and_repeated_column(installed):
    G, f, ids, vals = installed
    q = _queries(161, 129, _D, f)
    r0, s0 = G.diffusion_online(q, 3, 3, _T)
    G2 = _gallery(f)
    try:
        G2.diffusion_set_offline(ids, vals)
        r1, s1 = G2.diffusion_online(q, 3, 3, _T)
        assert np.array_equal(r1, r0) and np.array_equal(s1, s0)
        # the combine kernel adds a row's columns without synchronisation: a row that lists a column twice is refused
        bad = ids.copy()
        bad[417, 150] = bad[417, 3]
        with pytest.raises(RuntimeError, match="twice"):
            G2.diffusion_set_offline(bad, vals)
        bad = ids.copy()
        bad[0, 0] = _N
        with pytest.raises(RuntimeError):
            G2.diffusion_set_offline(bad, vals)
    finally:
        G2.close()
