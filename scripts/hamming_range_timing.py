"""Timing of the radius search and the self-join on a binary index (mi_hamming_range_search_device, mi_hamming_self_range;
DESIGN 5.13c) at full size: 1 005 994 random 2048-bit codes made on the device, 10 000 of the rows overwritten with copies of
other rows 0 .. 4 bits away, 1024 queries.  Per point the device time of one call (HIP events on the stream, median of 5 after
a warm-up call):
  - mi_hamming_search_device, k = 100: the yardstick (csrc/hamming.hip, not touched by the radius search);
  - mi_hamming_range_search_device at the radius that gives about 100 hits per query (the median 100th distance of the top-K
    answer) and at radius 0, each with the early exit of the scan on and off;
  - the whole self-join dedup.near_duplicate_pairs_hamming at a small radius, early exit on and off (wall time, host included).
One GPU process:

    timeout -k 10 900 python scripts/hamming_range_timing.py [out.json]
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
from isehr_amd.dedup import near_duplicate_pairs_hamming  # noqa: E402

N, NBITS, NQ, K, REPS = 1005994, 2048, 1024, 100, 5
COPIES, JOIN_RADIUS, JOIN_BATCH = 10000, 8, 4096


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
    nb = NBITS // 8
    gen = torch.Generator(device="cuda").manual_seed(7)
    codes = torch.randint(0, 256, (N, nb), dtype=torch.uint8, device="cuda", generator=gen)
    dst = torch.randperm(N, device="cuda", generator=gen)[:2 * COPIES]
    src, dst = dst[:COPIES], dst[COPIES:]
    flips = torch.zeros((COPIES, nb), dtype=torch.uint8, device="cuda")
    for _ in range(4):                             # up to 4 flipped bits (two draws may hit the same bit)
        col = torch.randint(0, nb, (COPIES,), device="cuda", generator=gen)
        bit = torch.randint(0, 8, (COPIES,), device="cuda", generator=gen)
        on = torch.randint(0, 2, (COPIES,), device="cuda", generator=gen).to(torch.uint8)
        flips[torch.arange(COPIES, device="cuda"), col] ^= (on << bit).to(torch.uint8)
    codes[dst] = codes[src] ^ flips
    q = torch.randint(0, 256, (NQ, nb), dtype=torch.uint8, device="cuda", generator=gen)
    torch.cuda.synchronize()
    g = _lib.BinaryGallery.from_device_ptr(codes.data_ptr(), N, NBITS)
    del codes
    torch.cuda.empty_cache()

    out = {"rows": N, "nbits": NBITS, "queries": NQ, "k": K, "reps": REPS, "points": []}
    idx = torch.empty((NQ, K), dtype=torch.int64, device="cuda")
    dist = torch.empty((NQ, K), dtype=torch.int32, device="cuda")
    ms = median_ms(lambda: g.search_device(q.data_ptr(), NQ, K, idx.data_ptr(), dist_ptr=dist.data_ptr(), stream=s))
    out["points"].append({"what": "mi_hamming_search_device", "k": K, "ms": ms})
    radius = int(dist[:, K - 1].median().item())
    top = (idx.cpu().numpy(), dist.cpu().numpy())

    cap = NQ * 4096
    lims = torch.empty(NQ + 1, dtype=torch.int64, device="cuda")
    ridx = torch.empty(cap, dtype=torch.int64, device="cuda")
    rdist = torch.empty(cap, dtype=torch.int32, device="cuda")
    answers = {}
    for r in (radius, 0):
        for early in (1, 0):
            _lib.set_global_option("hamming_range_early_exit", early)
            ms = median_ms(lambda: g.range_search_device(q.data_ptr(), NQ, r, cap, lims.data_ptr(), ridx.data_ptr(),
                                                         dist_ptr=rdist.data_ptr(), stream=s))
            lh = lims.cpu().numpy()
            total = int(lh[-1])
            assert total <= cap
            ans = (lh, ridx[:total].cpu().numpy(), rdist[:total].cpu().numpy())
            if r in answers:                       # the early exit only changes the work
                assert all(np.array_equal(a, b) for a, b in zip(ans, answers[r]))
            answers[r] = ans
            out["points"].append({"what": "mi_hamming_range_search_device", "radius": r, "early_exit": early, "ms": ms,
                                  "hits_per_query": total / NQ})
    # the radius answer holds the top-K answer of every query whose 100th distance is within the radius
    lh, ri, rd = answers[radius]
    checked = 0
    for i in range(NQ):
        if top[1][i, K - 1] <= radius:
            assert np.array_equal(ri[lh[i]:lh[i] + K], top[0][i]) and np.array_equal(rd[lh[i]:lh[i] + K], top[1][i])
            checked += 1
    out["queries_checked_against_top_k"] = checked

    for early in (1, 0):
        _lib.set_global_option("hamming_range_early_exit", early)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pi, pj, pd = near_duplicate_pairs_hamming(g, JOIN_RADIUS, batch=JOIN_BATCH)
        secs = time.perf_counter() - t0
        out["points"].append({"what": "near_duplicate_pairs_hamming", "radius": JOIN_RADIUS, "batch": JOIN_BATCH,
                              "early_exit": early, "seconds": secs, "pairs": int(pi.size),
                              "pairs_by_distance": np.bincount(pd, minlength=JOIN_RADIUS + 1).tolist()})
    _lib.set_global_option("hamming_range_early_exit", 1)
    g.close()
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
