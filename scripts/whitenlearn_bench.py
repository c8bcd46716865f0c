#!/usr/bin/env python
"""Times the scatter-matrix launch (csrc/scatter.hip) that learning a whitening rests on, next to the whitening GEMM
(whiten_mfma_kernel through mi_whiten_apply_device, dims = d, eps < 0) as the yardstick: same process, alternating, HIP events
around the launches, warm-up first, device-generated rows.

    python scripts/whitenlearn_bench.py [--n 1005994] [--d 2048] [--reps 5] [--pairs 200000] [--out profiles/whitenlearn_bench.json]

Reported per layout (row-major rows; the reference's [D, N] array seen as .T): median scatter time; TFLOP/s on the 2 N d^2 flop
of the full product and on the share actually multiplied (tiles on or above the diagonal); the fraction of the 78.6 TFLOP/s
float64 matrix peak on the latter; the whitening GEMM's median and the ratio scatter / GEMM (the acceptance line is <= 1.0).
Then pairs mode, pcawhitenlearn_hip end to end with the eigh time split out, and a host float64 X.T @ X on a 50 000-row slice
scaled to N (called "scaled": nobody waited for the full product)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MATRIX_PEAK_TFLOPS = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1005994)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--host-rows", type=int, default=50000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import isehr_amd  # noqa: F401
    from isehr_amd import _lib, whiten
    _lib.load()
    n, d = a.n, a.d
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.empty((n, d), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(x.data_ptr(), 77, 0, n, d)
    x.abs_()                                                  # non-negative like GeM descriptors
    torch.cuda.synchronize()
    xt = x.t().contiguous()                                   # the reference's [D, N] memory
    layouts = {"rows": (x, d, 1), "DN": (xt, 1, n)}
    ws_bytes = _lib.scatter_workspace_bytes(d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    C = torch.empty((d, d), dtype=torch.float64, device="cuda")
    centre = torch.empty(d, dtype=torch.float64, device="cuda")
    _lib.column_sum_device(x.data_ptr(), n, d, centre.data_ptr(), stream=stream)
    centre /= n
    P = torch.eye(d, dtype=torch.float64, device="cuda") + 0.001
    y = torch.empty((n, d), dtype=torch.float64, device="cuda")
    nt = (d + 127) // 128
    upper_share = (nt * (nt + 1) / 2) / (nt * nt)
    flop = 2.0 * n * d * d

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    def scatter(t, rs, cs, q=None, p=None):
        _lib.scatter_matrix_device(t.data_ptr(), n, d, C.data_ptr(), ws.data_ptr(), ws_bytes, centre.data_ptr(),
                                   None if q is None else q.data_ptr(), None if p is None else p.data_ptr(),
                                   0 if q is None else q.numel(), False, _lib.MI_F32, rs, cs, stream)

    def gemm(t, rs, cs):
        _lib.whiten_apply_device(t.data_ptr(), n, d, centre.data_ptr(), P.data_ptr(), d, y.data_ptr(), eps=-1.0,
                                 row_stride=rs, col_stride=cs, stream=stream)

    res = {"n": n, "d": d, "reps": a.reps, "dtype": "f32", "workspace_bytes": ws_bytes, "upper_tile_share": upper_share,
           "f64_matrix_peak_tflops": F64_MATRIX_PEAK_TFLOPS, "layouts": {}}
    for name, (t, rs, cs) in layouts.items():
        timed(lambda: scatter(t, rs, cs))                     # warm-up
        timed(lambda: gemm(t, rs, cs))
        ts, tg = [], []
        for _ in range(a.reps):                               # alternating
            ts.append(timed(lambda: scatter(t, rs, cs)))
            tg.append(timed(lambda: gemm(t, rs, cs)))
        s, g = float(np.median(ts)), float(np.median(tg))
        res["layouts"][name] = {
            "scatter_s": ts, "scatter_median_s": s, "whiten_gemm_s": tg, "whiten_gemm_median_s": g,
            "scatter_over_gemm": s / g,
            "scatter_tflops_full_product": flop / s * 1e-12,
            "scatter_tflops_multiplied": flop * upper_share / s * 1e-12,
            "scatter_fraction_of_f64_matrix_peak": flop * upper_share / s * 1e-12 / F64_MATRIX_PEAK_TFLOPS,
            "whiten_gemm_tflops": flop / g * 1e-12,
            "whiten_gemm_fraction_of_f64_matrix_peak": flop / g * 1e-12 / F64_MATRIX_PEAK_TFLOPS,
        }
        print(name, json.dumps(res["layouts"][name]), flush=True)
    del y
    # pairs mode
    gen = torch.Generator(device="cuda").manual_seed(3)
    q = torch.randint(0, n, (a.pairs,), device="cuda", generator=gen)
    p = torch.randint(0, n, (a.pairs,), device="cuda", generator=gen)
    res["pairs"] = {"n_pairs": a.pairs}
    for name, (t, rs, cs) in layouts.items():
        timed(lambda: scatter(t, rs, cs, q, p))
        res["pairs"][name + "_median_s"] = float(np.median([timed(lambda: scatter(t, rs, cs, q, p)) for _ in range(a.reps)]))
    print("pairs", json.dumps(res["pairs"]), flush=True)
    # the learner end to end, eigh split out
    t0 = time.time()
    m, Pl = whiten.pcawhitenlearn_hip(xt)
    total = time.time() - t0
    scatter(x, d, 1)
    torch.cuda.synchronize()
    Ch = C.cpu().numpy()
    t0 = time.time()
    whiten.pca_from_scatter(Ch, n)
    res["pcawhitenlearn_hip"] = {"total_s": total, "factorisation_eigh_s": time.time() - t0}
    print("learner", json.dumps(res["pcawhitenlearn_hip"]), flush=True)
    # host yardstick, scaled
    hr = min(a.host_rows, n)
    xh = x[:hr].cpu().numpy().astype(np.float64)
    t0 = time.time()
    xh.T @ xh
    th = time.time() - t0
    res["host_float64_product"] = {"rows": hr, "seconds": th, "scaled_to_n_s": th * n / hr, "omp_num_threads": os.environ.get("OMP_NUM_THREADS", ""),
                                   "note": "scaled from the slice; promotion and centring of the full array not included"}
    print("host", json.dumps(res["host_float64_product"]), flush=True)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
