"""Timing of the exact squared-L2 top-K search on the full-size gallery: 1 005 994 x 2048 rows synthesised on the
device (synth_fill_device) and scaled to unit norm on average ("unit") or to 30 times that ("x30": the bias 1/2 ||g||^2 leaves
fp16's range, the gallery takes the bf16 image), K = 100, nq in {1, 70, 1024}.  Per point: queries/s of Gallery.search_l2 next
to Gallery.search on a MI_NORM_NONE gallery of the SAME rows in the same process (the baseline: the same kernels on 2048
instead of 2112 stored columns, no distance tail), and what the filter let through: survivors and candidates per query and the
batches it had to answer again (overflow_batches).  Every time is the median of 5 wall times of synchronous host calls after a
warm-up call.  One GPU process:

    timeout -k 10 900 python scripts/l2_search_timing.py [out.json]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import isehr_amd  # noqa: E402,F401
from isehr_amd import _lib  # noqa: E402
from isehr_amd.synth import synth_rows  # noqa: E402

N, D, K, REPS = 1005994, 2048, 100, 5
NQS = (1, 70, 1024)
UNIT = 1.0 / (1.1547 * np.sqrt(D))       # synthetic rows have norm ~ 1.1547 sqrt(D)


def median_time(fn, reps=REPS):
    fn()                                           # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def galleries(scale):
    s = torch.cuda.current_stream().cuda_stream
    raw = torch.empty((N, D), dtype=torch.float32, device="cuda")
    _lib.synth_fill_device(raw.data_ptr(), 1234, 0, N, D, s)
    raw *= scale
    torch.cuda.synchronize()
    g_l2 = _lib.Gallery.l2_from_device_ptr(raw.data_ptr(), N, D)
    g_ip = _lib.Gallery.from_device_ptr(raw.data_ptr(), N, D, norm_mode=_lib.NORM_NONE)
    del raw
    torch.cuda.empty_cache()
    return g_l2, g_ip


def per_query(g, fn, nq):
    g.status(reset=True)
    fn()
    st = g.status()
    # one call; a batch that was answered again (overflow_batches, spec_retries) counts its queries once per attempt
    return {"survivors_per_query": st["survivors"] / nq, "candidates_per_query": st["candidates"] / nq,
            "overflow_batches": st["overflow_batches"], "spec_retries": st["spec_retries"], "batches_run": st["searches"]}


def main():
    out = {"rows": N, "dim": D, "k": K, "points": []}
    for name, scale in (("unit", UNIT), ("x30", 30.0 * UNIT)):
        g_l2, g_ip = galleries(float(scale))
        img = {"l2": int(g_l2.get_option("image_dtype")), "ip": int(g_ip.get_option("image_dtype"))}
        for nq in NQS:
            q = synth_rows(4321, 0, nq, D) * np.float32(scale)
            t_l2 = median_time(lambda: g_l2.search_l2(q, K))
            t_ip = median_time(lambda: g_ip.search(q, K))
            pt = {"gallery": name, "nq": nq, "image_f16": img, "l2_ms": t_l2 * 1e3, "ip_ms": t_ip * 1e3,
                  "l2_queries_per_s": nq / t_l2, "ip_queries_per_s": nq / t_ip, "l2_vs_ip_time": t_l2 / t_ip,
                  "l2": per_query(g_l2, lambda: g_l2.search_l2(q, K), nq), "ip": per_query(g_ip, lambda: g_ip.search(q, K), nq)}
            out["points"].append(pt)
            print("%-4s nq %4d: L2 %8.3f ms (%9.0f q/s) | IP %8.3f ms (%9.0f q/s) | x%.2f | L2 surv/q %.0f cand/q %.0f overflow %d | "
                  "IP surv/q %.0f cand/q %.0f overflow %d | image f16 L2 %d IP %d"
                  % (name, nq, pt["l2_ms"], pt["l2_queries_per_s"], pt["ip_ms"], pt["ip_queries_per_s"], pt["l2_vs_ip_time"],
                     pt["l2"]["survivors_per_query"], pt["l2"]["candidates_per_query"], pt["l2"]["overflow_batches"],
                     pt["ip"]["survivors_per_query"], pt["ip"]["candidates_per_query"], pt["ip"]["overflow_batches"],
                     img["l2"], img["ip"]), flush=True)
        g_l2.close()
        g_ip.close()
    print(json.dumps(out))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
