#!/usr/bin/env python3
"""Timing of the PQ index (mi_pq_search_device, mi_pq_add) on one MI355X -> profiles/pq_bench.json.

K = 100, M = 16 books of Ks = 256 codewords, d = 2048 (L = 128); N = 1 005 994 and 10^7 codes generated on the device; 1, 70 and
1024 Gaussian queries.  Per case: warm-up steps, then `--steps` timed steps between two HIP events (one search_device call each),
median and spread, beside the roofs the step is compared with:

  lookups   nq * N * M table lookups; one LDS read of 4 QT bytes serves the QT queries of a tile, and a random-address read runs
            at 32 lanes per clock and CU before bank conflicts (ds_read_b32 / b64; ds_read_b128: 16 lanes), i.e.
            256 CUs x 2.4 GHz x (32 | 16) x QT lookups / s
  matrix    the float32 matrix [nq][N] is written once by the scan and read by the selection (11 passes of launch_dense_topk:
            4 + 4 radix passes, 2 counts, 1 collect), against 8 TB/s -- the selection's passes mostly hit the 4 MB row in L2

The encode case times mi_pq_add of `--encode-rows` device rows (N x Ks x d float64 term-steps of 3 instructions against the
vector f64 rate 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz / 2).  The "greedyhash-sized" case is the shape of
scripts/hamming_bench.py (1 005 994 rows of d = 2048, 70 queries) for a side-by-side of queries/s.

The train case (`--cases train`, written to profiles/pq_train_bench.json) times mi_pq_train on 1 005 994 x 2048 float32 rows
generated on the device, M = 16, Ks = 256, 20 iterations from the default initial rows: the library's HIP events around the
assignment and the update of every iteration (mi_pq_train_timing), the move counts, the whole call; then the host variant
on a prefix of the same rows (`--train-host-rows`) for the upload, and scipy.cluster.vq.kmeans2 on one book of a 100 000-row
subsample for scale -- one thread, one book.

The ivf cases (`--cases ivf`, written to profiles/ivfpq_bench.json) time mi_ivfpq_search_device on 1 005 994 codes in nlist = 256
lists whose sizes lie within 2x of each other, nq in {1, 70, 1024} x nprobe in {1, 8, 32, 256}, and in the SAME process the step
of mi_pq_search_device on the same codes -- the exhaustive step every ratio is taken against -- beside the mean candidates per
query.  The first child checks one case against PQIndex.search with the equivalent allow bitmap before anything is timed.

The ivf_residual cases (`--cases ivf_residual`, written to profiles/ivfpq_residual_bench.json) run the shapes of the ivf cases on
a RESIDUAL index over the same codes and lists (mi_ivfpq_create_residual): the step of mi_ivfpq_search_device, in the SAME process
the step of the non-residual index, and the table kernel and the scan-and-select apart (HIP events of
mi_ivfpq_search_stages_device), with the table kernel's share of the float64 vector rate: 3 instructions per (table entry, column).
The first child checks, before anything is timed, that a residual index with zero centroids answers bit for bit as the plain one.

Every case runs in a child process of its own under `timeout`; the driver stops at the first case that fails."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "pq_bench.json")
TRAIN_OUT = os.path.join(ROOT, "profiles", "pq_train_bench.json")
IVF_OUT = os.path.join(ROOT, "profiles", "ivfpq_bench.json")
IVF_RES_OUT = os.path.join(ROOT, "profiles", "ivfpq_residual_bench.json")
IVF_N, IVF_LISTS = 1005994, 256

CLOCK, CUS = 2.4e9, 256
HBM_ROOF = 8e12                            # bytes / s
F64_VALU = CUS * 4 * 16 * CLOCK / 2        # float64 vector instructions / s (half rate)
M, KS, D, K = 16, 256, 2048, 100
SELECT_PASSES = 11


def device_index(_lib, torch, n):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    books = torch.randn((M, KS, D // M), dtype=torch.float32, device=dev, generator=gen).cpu().numpy()
    codes = torch.randint(0, KS, (n, M), dtype=torch.uint8, device=dev, generator=gen)
    torch.cuda.synchronize()
    idx = _lib.PQIndex.from_device_ptr(books, codes.data_ptr(), n)
    del codes
    torch.cuda.empty_cache()
    return idx, gen


def search_case(_lib, torch, n, nq, steps, warmup):
    dev = torch.device("cuda", 0)
    idx, gen = device_index(_lib, torch, n)
    q = torch.randn((nq, D), dtype=torch.float32, device=dev, generator=gen)
    out_i = torch.empty((nq, K), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, K), dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for _ in range(warmup):
        idx.search_device(q.data_ptr(), nq, K, out_i.data_ptr(), out_d.data_ptr(), stream=s)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        idx.search_device(q.data_ptr(), nq, K, out_i.data_ptr(), out_d.data_ptr(), stream=s)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    qt = 1 if nq == 1 else (2 if nq == 2 else 4)
    lanes = 16 if qt == 4 else 32
    npad = (n + 63) // 64 * 64
    lookups = float(nq) * n * M
    lds_floor = lookups / qt / (CUS * CLOCK * lanes)
    mat_bytes = float(nq) * npad * 4 * (1 + SELECT_PASSES)
    med = float(np.median(ms))
    rec = {"case": "search", "n": n, "m": M, "ks": KS, "d": D, "queries": nq, "k": K, "steps": steps, "warmup": warmup,
           "ms_per_batch_median": med, "ms_per_batch_min": float(ms.min()), "ms_per_batch_max": float(ms.max()),
           "queries_per_s": nq / (med * 1e-3), "query_tile": qt, "lookups": lookups, "lds_floor_ms": lds_floor * 1e3,
           "matrix_bytes": mat_bytes, "matrix_hbm_floor_ms": mat_bytes / HBM_ROOF * 1e3,
           "step_over_floor": med / (max(lds_floor, mat_bytes / HBM_ROOF) * 1e3), "hbm_bytes_index": idx.hbm_bytes,
           "note": "step = one mi_pq_search_device call (table, scan, selection and emit per chunk of queries)"}
    idx.close()
    return rec


def encode_case(_lib, torch, rows, steps):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    books = torch.randn((M, KS, D // M), dtype=torch.float32, device=dev, generator=gen).cpu().numpy()
    x = torch.randn((rows, D), dtype=torch.float32, device=dev, generator=gen)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps + 1):                                          # the first call allocates: not timed
        with _lib.PQIndex.empty(books, rows) as idx:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            idx.add_device(x.data_ptr(), rows)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    ms = np.array(ms[1:])
    steps64 = float(rows) * KS * D
    med = float(np.median(ms))
    return {"case": "encode", "rows": rows, "m": M, "ks": KS, "d": D, "steps": steps, "ms_median": med, "ms_min": float(ms.min()),
            "rows_per_s": rows / (med * 1e-3), "f64_term_steps": steps64, "f64_valu_floor_ms": 3 * steps64 / F64_VALU * 1e3,
            "over_floor": med / (3 * steps64 / F64_VALU * 1e3),
            "note": "mi_pq_add of device rows (synchronous call between two events on the default stream)"}


def timed_steps(torch, call, steps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return np.array(ms)


def ivf_case(_lib, torch, nq, nprobe, steps, warmup, check):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, nlist = IVF_N, IVF_LISTS
    books = torch.randn((M, KS, D // M), dtype=torch.float32, device=dev, generator=gen).cpu().numpy()
    coarse = torch.randn((nlist, D), dtype=torch.float32, device=dev, generator=gen).cpu().numpy()
    codes = torch.randint(0, KS, (n, M), dtype=torch.uint8, device=dev, generator=gen)
    # list sizes within 2x of each other: weights uniform in [1, 1.6), a row draws its list by weight.  The expected sizes span
    # at most 1.6x, and a list of some 3 000 rows strays from its expectation by about 2 % (one standard deviation)
    w = 1.0 + 0.6 * torch.rand(nlist, device=dev, generator=gen)
    lists = torch.multinomial(w, n, replacement=True, generator=gen).to(torch.uint8)
    q = torch.randn((nq, D), dtype=torch.float32, device=dev, generator=gen)
    torch.cuda.synchronize()
    flat = _lib.PQIndex.from_device_ptr(books, codes.data_ptr(), n)
    ivf = _lib.IVFPQIndex.from_device_ptr(coarse, books, codes.data_ptr(), lists.data_ptr(), n)
    sizes = ivf.list_sizes()
    assert sizes.max() < 2 * sizes.min(), (sizes.min(), sizes.max())
    probes = ivf.probe(q.cpu().numpy(), nprobe)
    if check:                                                           # before anything is timed
        qs = q[:min(nq, 4)].cpu().numpy()
        host_lists = lists.cpu().numpy()
        for i in range(qs.shape[0]):
            a = ivf.search(qs[i:i + 1], K, nprobe=nprobe)[:2]
            b = flat.search(qs[i:i + 1], K, allow=np.isin(host_lists, probes[i]))[:2]
            if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))):
                raise SystemExit("ivf answer differs from PQIndex.search under the equivalent allow bitmap: nothing is timed")
    out_i = torch.empty((nq, K), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, K), dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    ms = timed_steps(torch, lambda: ivf.search_device(q.data_ptr(), nq, K, out_i.data_ptr(), out_d.data_ptr(), nprobe=nprobe, stream=s),
                     steps, warmup)
    ex = timed_steps(torch, lambda: flat.search_device(q.data_ptr(), nq, K, out_i.data_ptr(), out_d.data_ptr(), stream=s), steps, warmup)
    med, exmed = float(np.median(ms)), float(np.median(ex))
    rec = {"case": "ivf", "n": n, "m": M, "ks": KS, "d": D, "nlist": nlist, "list_rows_min": int(sizes.min()),
           "list_rows_max": int(sizes.max()), "queries": nq, "nprobe": nprobe, "k": K, "steps": steps, "warmup": warmup,
           "candidates_per_query_mean": float(sizes[probes].sum(1).mean()), "checked_against_pq_search": bool(check),
           "ms_per_batch_median": med, "ms_per_batch_min": float(ms.min()), "ms_per_batch_max": float(ms.max()),
           "exhaustive_ms_median": exmed, "exhaustive_ms_min": float(ex.min()), "exhaustive_ms_max": float(ex.max()),
           "exhaustive_over_ivf": exmed / med, "queries_per_s": nq / (med * 1e-3), "hbm_bytes_index": ivf.hbm_bytes,
           "note": "step = one mi_ivfpq_search_device call (probe, prefix, table, scan + select, merge per chunk of queries); "
                   "exhaustive = one mi_pq_search_device call on the same codes in the same process"}
    ivf.close()
    flat.close()
    return rec


def ivf_residual_case(_lib, torch, nq, nprobe, steps, warmup, check):
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    n, nlist = IVF_N, IVF_LISTS
    books = torch.randn((M, KS, D // M), dtype=torch.float32, device=dev, generator=gen).cpu().numpy()
    coarse = torch.randn((nlist, D), dtype=torch.float32, device=dev, generator=gen).cpu().numpy()
    codes = torch.randint(0, KS, (n, M), dtype=torch.uint8, device=dev, generator=gen)
    w = 1.0 + 0.6 * torch.rand(nlist, device=dev, generator=gen)          # the lists of ivf_case
    lists = torch.multinomial(w, n, replacement=True, generator=gen).to(torch.uint8)
    q = torch.randn((nq, D), dtype=torch.float32, device=dev, generator=gen)
    torch.cuda.synchronize()
    plain = _lib.IVFPQIndex.from_device_ptr(coarse, books, codes.data_ptr(), lists.data_ptr(), n)
    res = _lib.IVFPQIndex.from_device_ptr(coarse, books, codes.data_ptr(), lists.data_ptr(), n, by_residual=True)
    sizes = res.list_sizes()
    probes = res.probe(q.cpu().numpy(), nprobe)
    if check:                                                           # before anything is timed
        # with every centroid zero a residual index answers, bit for bit, as a plain one over the same codes and lists: the
        # probes of the real centroids, given explicitly to both
        zero = np.zeros_like(coarse)
        qs = q[:min(nq, 4)].cpu().numpy()
        with _lib.IVFPQIndex.from_device_ptr(zero, books, codes.data_ptr(), lists.data_ptr(), n, by_residual=True) as rz, \
                _lib.IVFPQIndex.from_device_ptr(zero, books, codes.data_ptr(), lists.data_ptr(), n) as pz:
            a = rz.search(qs, K, probes=probes[:qs.shape[0]])[:2]
            b = pz.search(qs, K, probes=probes[:qs.shape[0]])[:2]
        if not (np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and (a[0] >= 0).all()):
            raise SystemExit("the residual index with zero centroids differs from the plain index: nothing is timed")
    out_i, out_d = (torch.empty((nq, K), dtype=torch.int64, device=dev), torch.empty((nq, K), dtype=torch.float32, device=dev))
    pout_i, pout_d = torch.empty_like(out_i), torch.empty_like(out_d)    # the plain index writes into buffers of its own
    s = torch.cuda.current_stream().cuda_stream
    ms = timed_steps(torch, lambda: res.search_device(q.data_ptr(), nq, K, out_i.data_ptr(), out_d.data_ptr(), nprobe=nprobe, stream=s),
                     steps, warmup)
    pl = timed_steps(torch, lambda: plain.search_device(q.data_ptr(), nq, K, pout_i.data_ptr(), pout_d.data_ptr(), nprobe=nprobe, stream=s),
                     steps, warmup)
    ref_i, ref_d, pref_i, pref_d = out_i.clone(), out_d.clone(), pout_i.clone(), pout_d.clone()
    stages = np.array([res.search_stages_device(q.data_ptr(), nq, K, out_i.data_ptr(), out_d.data_ptr(), nprobe=nprobe, stream=s)
                       for _ in range(steps)])
    pstages = np.array([plain.search_stages_device(q.data_ptr(), nq, K, pout_i.data_ptr(), pout_d.data_ptr(), nprobe=nprobe, stream=s)
                        for _ in range(steps)])
    torch.cuda.synchronize()
    if not (torch.equal(ref_i, out_i) and torch.equal(ref_d.view(torch.int32), out_d.view(torch.int32)) and
            torch.equal(pref_i, pout_i) and torch.equal(pref_d.view(torch.int32), pout_d.view(torch.int32))):
        raise SystemExit("the measured variant answers differently from mi_ivfpq_search_device")
    med, plmed = float(np.median(ms)), float(np.median(pl))
    table_ms, scan_ms = (float(v) for v in np.median(stages, axis=0))
    f64_instructions = 3.0 * nq * nprobe * KS * D
    rec = {"case": "ivf_residual", "n": n, "m": M, "ks": KS, "d": D, "nlist": nlist, "queries": nq, "nprobe": nprobe, "k": K,
           "steps": steps, "warmup": warmup, "checked_against_plain_index_at_zero_centroids": bool(check), "candidates_per_query_mean": float(sizes[probes].sum(1).mean()),
           "ms_per_batch_median": med, "ms_per_batch_min": float(ms.min()), "ms_per_batch_max": float(ms.max()),
           "plain_ms_median": plmed, "plain_ms_min": float(pl.min()), "plain_ms_max": float(pl.max()), "residual_over_plain": med / plmed,
           "table_ms_median": table_ms, "scan_ms_median": scan_ms, "plain_table_ms_median": float(np.median(pstages[:, 0])),
           "plain_scan_ms_median": float(np.median(pstages[:, 1])), "table_f64_instructions": f64_instructions,
           "table_fraction_of_f64_vector_rate": f64_instructions / (table_ms * 1e-3) / F64_VALU,
           "queries_per_s": nq / (med * 1e-3), "hbm_bytes_index": res.hbm_bytes,
           "note": "step = one mi_ivfpq_search_device call on the residual index; plain = the non-residual index over the same codes "
                   "and lists in the same process; table / scan = HIP events of mi_ivfpq_search_stages_device, summed over the chunks"}
    res.close()
    plain.close()
    return rec


def train_case(_lib, torch, rows, iters, host_rows):
    import time
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    L = D // M
    # clustered rows: 256 centres per book and noise, so that the iteration has something to find
    cent = torch.randn((M, KS, L), dtype=torch.float32, device=dev, generator=gen)
    lab = torch.randint(0, KS, (rows, M), device=dev, generator=gen)
    x = torch.empty((rows, D), dtype=torch.float32, device=dev)
    for j in range(M):
        x[:, j * L:(j + 1) * L] = cent[j][lab[:, j]]
    del lab
    step = 1 << 17
    for r in range(0, rows, step):
        x[r:r + step] += 0.5 * torch.randn((min(step, rows - r), D), dtype=torch.float32, device=dev, generator=gen)
    torch.cuda.synchronize()
    _lib.pq_train_device(x.data_ptr(), 4096, D, M, KS, 1)               # the first call loads the code objects: not timed
    t0 = time.time()
    books, moved = _lib.pq_train_device(x.data_ptr(), rows, D, M, KS, iters)
    call_s = time.time() - t0
    assign, update = _lib.pq_train_timing()
    rec = {"case": "train", "rows": rows, "m": M, "ks": KS, "d": D, "iters": iters, "init": "default rows floor(c n / ks)",
           "call_seconds": call_s, "moved": moved.tolist(), "assign_ms": [float(v) for v in assign], "update_ms": [float(v) for v in update],
           "assign_ms_median": float(np.median(assign)), "update_ms_median": float(np.median(update)),
           "update_hbm_floor_ms": float(rows) * D * 4 / HBM_ROOF * 1e3,
           "assign_f64_valu_floor_ms": [2 * float(rows) * KS * D / F64_VALU * 1e3, 3 * float(rows) * KS * D / F64_VALU * 1e3],
           "note": "device rows; assignment = pq_encode_kernel + the move count, update = code columns + pq_update_kernel, both "
                   "between HIP events of the library (mi_pq_train_timing)"}
    if host_rows > 0:
        hx = x[:host_rows].cpu().numpy()
        t0 = time.time()
        _lib.pq_train(hx, M, KS, iters=1)
        host_s = time.time() - t0
        t0 = time.time()
        _lib.pq_train_device(x.data_ptr(), host_rows, D, M, KS, 1)
        dev_s = time.time() - t0
        rec["host_variant"] = {"rows": host_rows, "bytes": host_rows * D * 4, "iters": 1, "host_call_seconds": host_s,
                               "device_call_seconds": dev_s, "upload_and_checks_seconds": host_s - dev_s,
                               "note": "pageable host rows; the difference holds the finite check on the host and the one upload"}
    try:
        from scipy.cluster.vq import kmeans2
        sub = x[:100000, :L].double().cpu().numpy()
        c0 = sub[(np.arange(KS) * sub.shape[0]) // KS]
        t0 = time.time()
        kmeans2(sub, c0, iter=iters, minit="matrix")
        rec["scipy_kmeans2"] = {"rows": int(sub.shape[0]), "books": 1, "iters": iters, "seconds": time.time() - t0,
                                "note": "one thread, ONE book of a 100 000-row subsample on the host of the GPU"}
    except ImportError:
        rec["scipy_kmeans2"] = None
    return rec


def run_child(args):
    import torch
    import isehr_amd  # noqa: F401
    from isehr_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device and has no other path")
    kind, *rest = args.child.split(":")
    if kind == "search":
        rec = search_case(_lib, torch, int(rest[0]), int(rest[1]), args.steps, args.warmup)
    elif kind == "ivf":
        rec = ivf_case(_lib, torch, int(rest[0]), int(rest[1]), args.steps, args.warmup, rest[2] == "1")
    elif kind == "ivfres":
        rec = ivf_residual_case(_lib, torch, int(rest[0]), int(rest[1]), args.steps, args.warmup, rest[2] == "1")
    elif kind == "train":
        rec = train_case(_lib, torch, int(rest[0]), args.train_iters, min(args.train_host_rows, int(rest[0])))
    else:
        rec = encode_case(_lib, torch, int(rest[0]), max(1, args.steps // 4))
    rec["device"] = torch.cuda.get_device_name(0)
    print("PQBENCH " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1m,10m,encode", help="comma list of: 1m / 10m (1 005 994 / 10^7 codes at 1, 70 and 1024 "
                                                              "queries), 1m-<Q> / 10m-<Q> (one batch size), encode, train, ivf, "
                                                              "ivf-<Q>-<nprobe>, ivf_residual, ivf_residual-<Q>-<nprobe>")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--encode-rows", type=int, default=1005994)
    ap.add_argument("--train-rows", type=int, default=1005994)
    ap.add_argument("--train-iters", type=int, default=20)
    ap.add_argument("--train-host-rows", type=int, default=250000, help="rows of the host variant (0 = skip it)")
    ap.add_argument("--train-out", default=TRAIN_OUT)
    ap.add_argument("--ivf-out", default=IVF_OUT)
    ap.add_argument("--ivf-residual-out", default=IVF_RES_OUT)
    ap.add_argument("--case-timeout", type=int, default=240, help="seconds each child process may take")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return run_child(args)
    sizes = {"1m": 1005994, "10m": 10 ** 7}
    children = []
    for c in args.cases.split(","):
        if c in sizes:
            children += ["search:%d:%d" % (sizes[c], nq) for nq in (1, 70, 1024)]
        elif "-" in c and c.split("-")[0] in sizes:
            children.append("search:%d:%d" % (sizes[c.split("-")[0]], int(c.split("-")[1])))
        elif c == "encode":
            children.append("encode:%d" % args.encode_rows)
        elif c == "train":
            children.append("train:%d" % args.train_rows)
        elif c == "ivf":
            # the first ivf child of a run checks its case against PQIndex.search before anything is timed
            children += ["ivf:%d:%d:%d" % (nq, nprobe, not any(ch.startswith("ivf:") for ch in children) and (nq, nprobe) == (1, 1))
                         for nq in (1, 70, 1024) for nprobe in (1, 8, 32, 256)]
        elif c == "ivf_residual":
            # the first child checks the residual index against the plain one at zero centroids before anything is timed
            children += ["ivfres:%d:%d:%d" % (nq, nprobe, (nq, nprobe) == (1, 1)) for nq in (1, 70, 1024) for nprobe in (1, 8, 32, 256)]
        elif c.startswith("ivf_residual-"):
            children.append("ivfres:%d:%d:1" % tuple(int(v) for v in c.split("-")[1:3]))
        elif c.startswith("ivf-"):
            children.append("ivf:%d:%d:1" % tuple(int(v) for v in c.split("-")[1:3]))
        else:
            raise SystemExit("unknown case " + c)
    results = []
    for child in children:
        cmd = ["timeout", "-k", "10", str(args.case_timeout), sys.executable, os.path.abspath(__file__), "--child", child,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--train-iters", str(args.train_iters),
               "--train-host-rows", str(args.train_host_rows)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("PQBENCH ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            raise SystemExit("case %s ended with status %d: nothing more is started" % (child, r.returncode))
        results.append(json.loads(line[0][len("PQBENCH "):]))
        print(json.dumps(results[-1]), flush=True)
    trained = [r for r in results if r["case"] == "train"]
    inverted = [r for r in results if r["case"] == "ivf"]
    residual = [r for r in results if r["case"] == "ivf_residual"]
    results = [r for r in results if r["case"] not in ("train", "ivf", "ivf_residual")]
    if residual:
        os.makedirs(os.path.dirname(args.ivf_residual_out), exist_ok=True)
        json.dump({"f64_valu_instructions_per_s": F64_VALU, "cases": residual}, open(args.ivf_residual_out, "w"), indent=1)
    if inverted:
        os.makedirs(os.path.dirname(args.ivf_out), exist_ok=True)
        json.dump({"cases": inverted}, open(args.ivf_out, "w"), indent=1)
    if trained:
        os.makedirs(os.path.dirname(args.train_out), exist_ok=True)
        json.dump({"hbm_roof_bytes_per_s": HBM_ROOF, "f64_valu_instructions_per_s": F64_VALU, "cases": trained},
                  open(args.train_out, "w"), indent=1)
    if not results:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump({"lds_roof": "256 CUs x 2.4 GHz x (32 | 16 at ds_read_b128) lanes per clock, before bank conflicts",
               "hbm_roof_bytes_per_s": HBM_ROOF, "f64_valu_instructions_per_s": F64_VALU, "cases": results},
              open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
