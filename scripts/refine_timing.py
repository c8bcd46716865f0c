"""Timing of the shortlist re-ranking (mi_refine_device) on the full-size gallery: 1 005 994 x 2048 rows synthesised on
the device (synth_fill_device) in a squared-L2 gallery, nq in {1024, 1}, kc in {100, 1000, 4096} random ids per query, k = 100.
Per point: the device time of one call (HIP events on the stream, median of 5 after a warm-up call), the byte floor
nq * kc * 8 KiB at 0.85 x 8 TB/s (the HBM rate the single-query search is held against), and for kc <= 2048 the same ids through
the one-workgroup-per-query tail of the flat L2 search (mi_debug_l2_tail_device): what spreading a query's rows over kc / 8
workgroups buys.  One GPU process:

    timeout -k 10 600 python scripts/refine_timing.py [out.json]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import isehr_amd  # noqa: E402,F401
from isehr_amd import _lib  # noqa: E402

N, D, K, REPS = 1005994, 2048, 100, 5
NQS = (1024, 1)
KCS = (100, 1000, 4096)
HBM_BYTES_PER_S = 0.85 * 8e12


def median_ms(fn, reps=REPS):
    fn()                                           # warm-up (grows the handle's buffers)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    s = torch.cuda.current_stream().cuda_stream
    raw = torch.empty((N, D), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(raw.data_ptr(), 1234, 0, N, D, s)
    torch.cuda.synchronize()
    g = _lib.Gallery.l2_from_device_ptr(raw.data_ptr(), N, D)
    del raw
    torch.cuda.empty_cache()
    lib = _lib.load()
    out = {"rows": N, "dim": D, "k": K, "hbm_bytes_per_s": HBM_BYTES_PER_S, "points": []}
    gen = torch.Generator(device="cuda").manual_seed(99)
    for nq in NQS:
        q = torch.empty((nq, D), dtype=torch.float32, device="cuda")
        _lib.synth_fill_device(q.data_ptr(), 4321, 0, nq, D, s)
        for kc in KCS:
            cand = torch.randint(0, N, (nq, kc), dtype=torch.int64, device="cuda", generator=gen)
            idx = torch.empty((nq, kc), dtype=torch.int64, device="cuda")
            v64 = torch.empty((nq, kc), dtype=torch.float64, device="cuda")
            ms = median_ms(lambda: g.refine_device(q.data_ptr(), nq, cand.data_ptr(), kc, K, idx.data_ptr(), val64_ptr=v64.data_ptr(), stream=s))
            floor_ms = nq * kc * D * 4 / HBM_BYTES_PER_S * 1e3
            pt = {"nq": nq, "kc": kc, "refine_ms": ms, "floor_ms": floor_ms, "refine_over_floor": ms / floor_ms,
                  "gather_tb_per_s": nq * kc * D * 4 / (ms * 1e-3) / 1e12}
            if kc <= 2048:
                ref = g.refine(q.cpu().numpy(), cand.cpu().numpy(), kc)[2]       # all kc, to compare the two kernels' values
                tail_ms = median_ms(lambda: _lib.check(lib.mi_debug_l2_tail_device(
                    g._h, C.c_void_p(q.data_ptr()), nq, C.c_void_p(cand.data_ptr()), kc, kc, C.c_void_p(idx.data_ptr()),
                    C.c_void_p(v64.data_ptr()), C.c_void_p(s))))
                torch.cuda.synchronize()
                # the tail keeps repeated ids, refine drops them: compare the distinct values
                same = all(np.array_equal(np.unique(v64[i].cpu().numpy()), np.unique(ref[i][np.isfinite(ref[i])])) for i in range(min(nq, 8)))
                pt.update({"one_workgroup_tail_ms": tail_ms, "tail_over_refine": tail_ms / ms, "same_values": bool(same)})
            out["points"].append(pt)
            print(json.dumps(pt), flush=True)
    g.close()
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
