#!/usr/bin/env python3
"""Timing of the LSH encoder (mi_lsh_encode_device, csrc/lsh.hip) on one MI355X -> profiles/lsh_bench.json.

Shape: 1 005 994 x 2048 float32 descriptors (generated on the device) -> 2048, 1024 and 256 bits, R = standard normal float64
(the time does not depend on the directions).  Per nbits, in ONE process and alternating step by step:
  encode   one mi_lsh_encode_device call: X -> packed codes, nothing else written
  whiten   the route to the same operands without this kernel: mi_whiten_apply_device(eps < 0, zero mean) into an [rows][nbits]
           float64 buffer (the comparison and the packing would still have to follow); on the largest row chunk that fits in
           free memory, scaled to the full row count
Each step lies between two HIP events on the stream the kernel is launched on; warm-up steps first, then the median of
`--steps` (>= 10) and the spread.  Work from the shapes: 2 n d nbits flop against the 78.6 TFLOP/s f64 matrix peak; algorithmic
bytes (X once, R once, output once) against 8 TB/s.  The codes of the first 131 072 rows are compared with the sign bits of
the whitening route's float64 products (same K order: no bit may differ).
End to end: LSHIndex.search (upload, encoding of the queries, Hamming search, download) at 1024 queries and K = 100 on an
index of the same rows, steady state; and one whole matching_LSH_hip call from host arrays (its timer spans the search only,
on a fresh index, i.e. including the first-use allocations of the search buffers)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "lsh_bench.json")

F64_MATRIX_PEAK = 78.6e12                 # flop / s (AMD's MI355X data sheet)
HBM_ROOF = 8e12                           # bytes / s


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max())}


def bench_bits(_lib, torch, X, nbits, steps, warmup):
    n, d = X.shape
    dev = X.device
    s = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(100 + nbits)
    R = torch.randn((nbits, d), dtype=torch.float64, device=dev, generator=gen)
    mean = torch.zeros(d, dtype=torch.float64, device=dev)
    codes = torch.empty((n, nbits // 8), dtype=torch.uint8, device=dev)
    free, _ = torch.cuda.mem_get_info()
    wrows = int(min(n, (free * 0.8) // (nbits * 8)) // 128 * 128) or 128
    wrows = min(wrows, n)
    Y = torch.empty((wrows, nbits), dtype=torch.float64, device=dev)

    def encode():
        _lib.lsh_encode_device(X.data_ptr(), n, d, R.data_ptr(), nbits, codes.data_ptr(), stream=s)

    def whiten():
        _lib.whiten_apply_device(X.data_ptr(), wrows, d, mean.data_ptr(), R.data_ptr(), nbits, Y.data_ptr(), eps=-1.0, stream=s)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(warmup):
        encode()
        whiten()
    torch.cuda.synchronize()
    enc, whi = [], []
    for _ in range(steps):
        enc.append(timed(encode))
        whi.append(timed(whiten))
    # same operands, same K order: the sign bits of the whitening route's products are the codes
    chk = min(wrows, 131072)
    w = (2 ** torch.arange(8, device=dev, dtype=torch.int32)).view(1, 1, 8)
    ref = ((Y[:chk] >= 0).view(chk, nbits // 8, 8).to(torch.int32) * w).sum(dim=2).to(torch.uint8)
    differing = int((ref != codes[:chk]).sum().item())
    flop = 2.0 * n * d * nbits
    e, wh = stats(enc), stats(whi)
    scale = n / wrows
    enc_bytes = n * d * X.element_size() + nbits * d * 8.0 + n * nbits / 8.0
    rec = {"n": n, "d": d, "nbits": nbits, "steps": steps, "warmup": warmup, "flop": flop,
           "encode_ms": e, "encode_tflops": flop / (e["median_ms"] * 1e-3) / 1e12,
           "encode_frac_f64_matrix_peak": flop / (e["median_ms"] * 1e-3) / F64_MATRIX_PEAK,
           "encode_algorithmic_bytes": enc_bytes, "encode_hbm_floor_ms": enc_bytes / HBM_ROOF * 1e3,
           "encode_bound": "f64 matrix pipe" if flop / F64_MATRIX_PEAK > enc_bytes / HBM_ROOF else "HBM",
           "whiten_rows": wrows, "whiten_ms_measured": wh,
           "whiten_ms_at_n": {k: v * scale for k, v in wh.items()},
           "whiten_tflops": 2.0 * wrows * d * nbits / (wh["median_ms"] * 1e-3) / 1e12,
           "whiten_output_bytes_at_n": n * nbits * 8.0,
           "encode_over_whiten": e["median_ms"] / (wh["median_ms"] * scale),
           "rows_compared_with_whiten_route": chk, "code_bytes_differing": differing}
    del Y, codes, R
    torch.cuda.empty_cache()
    return rec


def bench_search(_lib, torch, X, nbits, nq, k, steps, warmup):
    n, d = X.shape
    R = np.random.default_rng(nbits).standard_normal((nbits, d))
    q = np.random.default_rng(nbits + 1).standard_normal((nq, d)).astype(np.float32)
    with _lib.LSHIndex.empty(d, nbits, n, R=R) as idx:
        t0 = time.perf_counter()
        idx.add_device(X.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        secs = []
        for i in range(warmup + steps):
            _, _, sec = idx.search(q, k)
            if i >= warmup:
                secs.append(sec * 1e3)
        st = stats(secs)
        return {"n": n, "d": d, "nbits": nbits, "queries": nq, "k": k, "steps": steps, "warmup": warmup,
                "index_build_from_device_rows_s": build_s, "search_ms": st, "queries_per_s": nq / (st["median_ms"] * 1e-3),
                "hbm_bytes_index": idx.hbm_bytes,
                "note": "LSHIndex.search: host queries in, host answer out (upload, encode, Hamming search, download)"}


def bench_matching(torch, X, nbits, nq, k):
    from isehr_amd.nnsearch import matching_LSH_hip
    train = X.cpu().numpy()
    q = np.random.default_rng(nbits + 1).standard_normal((nq, X.shape[1])).astype(np.float32)
    matching_LSH_hip(1, train[:4096], q[:8], nbits)                   # code objects loaded
    t0 = time.perf_counter()
    _, tpq = matching_LSH_hip(k, train, q, nbits)
    wall = time.perf_counter() - t0
    return {"n": int(X.shape[0]), "d": int(X.shape[1]), "nbits": nbits, "queries": nq, "k": k, "time_per_query_s": tpq,
            "queries_per_s": 1.0 / tpq, "whole_call_s": wall,
            "note": "one matching_LSH_hip call from host arrays; time_per_query spans the search only (fresh index: first-use "
                    "allocation of the search buffers included), whole_call_s adds the rotation (QR) and the index build"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1005994)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--bits", default="2048,1024,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--e2e-bits", type=int, default=256)
    ap.add_argument("--no-matching", action="store_true", help="skip the whole matching_LSH_hip call (an 8 GB host copy)")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    import isehr_amd  # noqa: F401
    from isehr_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this benchmark measures the device and has no other path")
    if args.steps < 10:
        raise SystemExit("--steps: the median of at least 10 launches")
    _lib.load()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    X = torch.empty((args.n, args.d), dtype=torch.float32, device=dev)
    for r in range(0, args.n, 1 << 18):
        m = min(1 << 18, args.n - r)
        X[r:r + m] = torch.randn((m, args.d), dtype=torch.float32, device=dev, generator=gen)
    torch.cuda.synchronize()
    doc = {"device": torch.cuda.get_device_name(0), "f64_matrix_peak_flops": F64_MATRIX_PEAK, "hbm_roof_bytes_per_s": HBM_ROOF,
           "timing": "HIP events around one call, median of --steps after --warmup, encode and whiten alternating", "encode": []}
    for nbits in [int(b) for b in args.bits.split(",")]:
        rec = bench_bits(_lib, torch, X, nbits, args.steps, args.warmup)
        print(json.dumps(rec), flush=True)
        doc["encode"].append(rec)
    doc["search"] = bench_search(_lib, torch, X, args.e2e_bits, args.queries, args.k, args.steps, args.warmup)
    print(json.dumps(doc["search"]), flush=True)
    if not args.no_matching:
        doc["matching_LSH_hip"] = bench_matching(torch, X, args.e2e_bits, args.queries, args.k)
        print(json.dumps(doc["matching_LSH_hip"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
