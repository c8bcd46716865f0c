"""Shared checkers of the diffusion GPU tests: the device's kNN graph against float64 scores, every offline row against the
dense float64 solve on that very graph (oracle.diffusion_solve_nodes), and the online answer against the plain float64
combination with a derived rounding bound.  Nothing here leaves a row, a query or a position out."""
import numpy as np

import oracle

SCORE_TOL = 2e-6        # the project's tolerance for an f32 inner product against float64
SOLVE_CEILING = 5e-6    # float32-stored solution against the float64 solve (test_diffusion_offline_at_the_reference_size)
MARGIN = 1e-6           # least relative distance of any tested residual norm from tol, reference side


def clustered(seed, n, d, k=12, noise=0.9, pull=2.0):
    """Unit-norm rows around k centres: a graph with real mutual neighbours."""
    from isehr_amd.synth import synth_rows
    f = synth_rows(seed, 0, n, d).astype(np.float64)
    centers = synth_rows(seed + 1, 0, k, d).astype(np.float64)
    f = noise * f + pull * centers[np.arange(n) % k]
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    return f.astype(np.float32)


def check_graph(f, ids, sims):
    """The kNN lists the device diffused on: exact top-T by float64 score up to SCORE_TOL, T distinct ids per row, the
    listed similarity is the float64 score of the listed id, rows sorted by (similarity descending, id ascending)."""
    f64 = np.asarray(f, dtype=np.float64)
    s64 = f64 @ f64.T
    n, T = ids.shape
    assert sims.shape == (n, T) and ids.dtype == np.int64 and sims.dtype == np.float32
    assert ids.min() >= 0 and ids.max() < n
    assert oracle.check_topk_parity(ids, s64, T, SCORE_TOL) == []
    assert (np.diff(np.sort(ids, axis=1), axis=1) > 0).all(), "a row lists an id twice"
    listed = np.take_along_axis(s64, ids, axis=1)
    assert np.abs(sims.astype(np.float64) - listed).max() <= SCORE_TOL
    step = np.diff(sims, axis=1)
    assert (step <= 0).all(), "similarities increase along a row"
    assert (np.diff(ids, axis=1)[step == 0] > 0).all(), "equal similarities not in ascending id"
    return s64


def check_offline_rows(ids, sims, vals, kd, nodes, alpha=0.99, gamma=3, maxiter=20, tol=1e-6, label=""):
    """vals [len(nodes), T]: the device's solutions of `nodes`, all compared with the float64 solve on the device's own
    graph.  -> (max |error|, reference iteration counts, reference solutions)."""
    nodes = np.asarray(nodes, dtype=np.int64)
    assert vals.shape == (len(nodes), ids.shape[1]) and vals.dtype == np.float32
    # exact_power: the affinity's power rounded once to float32; numpy's own float32 power is one ulp off that for a fifth
    # of the entries, differently from build to build, and a two-node component (kd = 2) carries one ulp of a Laplacian
    # entry into 1e-3 of its solution (50.25, 49.75)
    xs, its, margins, _ = oracle.diffusion_solve_nodes(sims, ids, kd, nodes, alpha, gamma, maxiter, tol, exact_power=True)
    # a condition on the input: no reference residual passes within rounding of tol, so both sides take the same exit
    assert margins.min() > MARGIN, "residual %.3e of tol away from tol: pick another seed" % margins.min()
    err = float(np.abs(vals.astype(np.float64) - xs).max())
    print("diffusion offline %s N=%d T=%d kd=%d nodes=%d alpha=%g gamma=%d maxiter=%d tol=%g: iterations %d..%d, "
          "max |x| %.3f, max |error| %.3e" % (label, len(ids), ids.shape[1], kd, len(nodes), alpha, gamma, maxiter, tol,
                                             its.min(), its.max(), np.abs(xs).max(), err))
    assert np.isfinite(vals).all()
    assert err < SOLVE_CEILING, err
    return err, its, xs


def online_bound(kq, gamma, mag, dsens):
    """Per-entry bound of the device's float32 combination against the float64 one.  The device raises a float32
    similarity to gamma by repeated multiplication, multiplies by the float32 offline value and adds kq such products in
    float32: at most kq + gamma + 2 roundings of 2**-24 relative to sum_j |w_j v_j| (`mag`).  Its similarity may be
    SCORE_TOL away from the float64 one, which the power carries on as gamma |s|**(gamma-1) SCORE_TOL |v| per term (`dsens`
    is that sum without the SCORE_TOL factor)."""
    return (kq + gamma + 2) * 2.0 ** -24 * mag + SCORE_TOL * dsens


def check_online(G, f, off_ids, off_vals, queries, kq, gamma, trunc, ranks, scores, label=""):
    """ranks/scores [Q,trunc] as mi_diffusion_online returned them for `queries` on gallery handle G (rows f, installed
    offline lists off_ids/off_vals).  Every query and every position is compared.  -> largest error / bound ratio."""
    n = len(f)
    q64 = np.asarray(queries, dtype=np.float64)
    nq = q64.shape[0]
    assert ranks.shape == (nq, trunc) and scores.shape == (nq, trunc)
    assert ranks.dtype == np.int64 and scores.dtype == np.float32
    s64 = q64 @ np.asarray(f, dtype=np.float64).T
    # the query neighbours: mi_diffusion_online runs the handle's own search, so Gallery.search returns its choice
    didx, dsims, _ = G.search(queries, kq)
    assert oracle.check_topk_parity(didx, s64, kq, SCORE_TOL) == []
    assert np.abs(dsims.astype(np.float64) - np.take_along_axis(s64, didx, axis=1)).max() <= SCORE_TOL
    idx = np.argsort(-s64, axis=1, kind="stable")[:, :kq]
    moved = 0
    for q in range(nq):
        if set(idx[q].tolist()) != set(didx[q].tolist()):      # a near-tie at the k-th place: the device's set is as good
            idx[q] = didx[q]
            moved += 1
    nn_sims = np.take_along_axis(s64, idx, axis=1)
    dense, mag, dsens = oracle.diffusion_online_dense(idx, nn_sims, off_ids, off_vals, n, gamma)
    bound = online_bound(kq, gamma, mag, dsens)
    got = scores.astype(np.float64)
    want = np.take_along_axis(dense, ranks, axis=1)
    err = np.abs(got - want)
    b = np.take_along_axis(bound, ranks, axis=1)
    assert (err[b == 0] == 0).all(), "an entry no neighbour row reaches is not exactly zero"
    ratio = float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    print("diffusion online %s N=%d T=%d nq=%d k_query=%d gamma=%d trunc=%d: %d queries on the device's neighbour set, "
          "max |error| %.3e, max error/bound %.4f" % (label, n, off_ids.shape[1], nq, kq, gamma, trunc, moved, err.max(),
                                                      ratio))
    assert ratio < 1.0, ratio
    for q in range(nq):
        bad = oracle.check_topk_parity(ranks[q:q + 1], dense[q:q + 1], trunc, float(bound[q].max()))
        assert bad == [], (q, bad)
    step = np.diff(scores, axis=1)
    assert (step <= 0).all(), "scores increase along a row"
    assert (np.diff(ranks, axis=1)[step == 0] > 0).all(), "equal scores not in ascending id"
    return ratio
