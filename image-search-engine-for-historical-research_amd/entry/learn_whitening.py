"""Counterpart of the whitening-learning step of src/main_train.py:658-670: descriptors -> {m, P}, the pickle
`main_retrieve --whitening` evaluates.  The [D, N] x [N, D] float64 product of both learners runs on the GPU (csrc/scatter.hip);
the D x D factorisation is numpy / LAPACK on the host.

  python -m isehr_amd.entry.learn_whitening --features outputs/roxford5k_vecs.npy --out Lw.pkl            (PCA)
  python -m isehr_amd.entry.learn_whitening --features ... --pairs db.pkl --out Lw.pkl                     (supervised)
  python -m isehr_amd.entry.learn_whitening --gallery outputs/roxford5k.gal --out Lw.pkl                   (PCA of the stored rows)

--features: a [D, N] `.npy` array (memory-mapped: it moves to the GPU in row blocks), a `.pt` tensor file (features.load_torch_vecs)
or a feature-store pickle {'path', 'feature'} (features.save_path_feature).  --pairs: a pickle with `qidxs` / `pidxs` like the
reference's `<name>-whiten.pkl`; absent = PCA whitening.  --gallery: a prepared-gallery file; PCA only (the rows are the
gallery's normalised ones).
"""
import argparse
import pickle
import time

import numpy as np

from .. import whiten

parser = argparse.ArgumentParser(prog="learn_whitening", description="Learn a whitening {m, P} on the GPU")
parser.add_argument("--features", default="", help="[D, N] descriptors: .npy, .pt or a feature-store .pkl")
parser.add_argument("--gallery", default="", help="prepared-gallery file (mi_gallery_save); PCA only")
parser.add_argument("--pairs", default="", help="pickle with 'qidxs' and 'pidxs' (supervised whitening); absent = PCA")
parser.add_argument("--out", "-o", required=True, help="output pickle {'m': [D,1], 'P': [D,D]}")
parser.add_argument("--gpu-id", "-g", default="0")


def load_features(path):
    if path.endswith(".npy"):
        X = np.load(path, mmap_mode="r")
    elif path.endswith(".pt"):
        from .features import load_torch_vecs
        X = load_torch_vecs(path)
    else:
        with open(path, "rb") as f:
            X = np.asarray(pickle.load(f)["feature"])
    if X.ndim != 2:
        raise ValueError("expected a [D, N] array, got %s" % (X.shape,))
    return X


def load_pairs(path):
    with open(path, "rb") as f:
        db = pickle.load(f)
    if "qidxs" not in db or "pidxs" not in db:
        raise ValueError("%s holds no 'qidxs' / 'pidxs'" % path)
    return np.asarray(db["qidxs"], dtype=np.int64), np.asarray(db["pidxs"], dtype=np.int64)


def scatter_features(X, pairs, device):
    """-> (m [D], N, C_m, S | None): everything the factorisation needs, all from the device."""
    from .. import _lib
    rows = _lib._strided(np.asarray(X).T)[0]              # a view: a memory-mapped file stays on disk until its blocks are packed
    n = rows.shape[0]
    if pairs is None:
        m = whiten._host_column_mean(rows, device)
        return m, n, _lib.scatter_matrix(rows, centre=m, device=device), None
    q, p = whiten._pairs(pairs[0], pairs[1], n)
    m = np.asarray(rows[q], dtype=np.float64).mean(axis=0)
    S = _lib.scatter_matrix(rows, pairs=(q, p), device=device) / q.size
    return m, n, _lib.scatter_matrix(rows, centre=m, device=device), S


def scatter_gallery(path, device):
    from .. import _lib
    g = _lib.Gallery.load(path, device=device)
    try:
        m = np.zeros(g.d)
        step = max(1, (64 << 20) // (4 * g.d))
        for r0 in range(0, g.n, step):
            m += g.get_rows(r0, min(step, g.n - r0)).sum(axis=0, dtype=np.float64)
        m /= g.n
        return m, g.n, g.scatter(m), None
    finally:
        g.close()


def main(argv=None):
    args = parser.parse_args(argv)
    if bool(args.features) == bool(args.gallery):
        parser.error("give exactly one of --features and --gallery")
    if args.gallery and args.pairs:
        parser.error("--gallery learns PCA whitening only (the pairs index the source array, not the stored rows)")
    dev = int(args.gpu_id)
    pairs = load_pairs(args.pairs) if args.pairs else None
    t0 = time.time()
    if args.gallery:
        m, n, C, S = scatter_gallery(args.gallery, dev)
    else:
        m, n, C, S = scatter_features(load_features(args.features), pairs, dev)
    t1 = time.time()
    P = whiten.pca_from_scatter(C, n)[0] if S is None else whiten.supervised_from_scatter(S, C)
    t2 = time.time()
    Lw = {"m": np.ascontiguousarray(m.reshape(-1, 1)), "P": P}
    with open(args.out, "wb") as f:
        pickle.dump(Lw, f)
    print(">> {} whitening of {} descriptors x {} dimensions: scatter {:.3f} s, factorisation {:.3f} s -> {}".format(
        "supervised" if S is not None else "PCA", n, m.shape[0], t1 - t0, t2 - t1, args.out))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
