"""Truth of the graph index over PQ codes (mi_pq_graph_search, mi_pq_graph_build), the case sweep of
tests/test_gpu_pq_graph.py and its seeded inputs.  No arithmetic of its own: the values are tests/_pq_truth.py's (dtable64,
adc_truth: pinned bit-equal to the library's PQ search), the traversal and the table construction tests/_graph_truth.py's
(search_truth, build_truth with l2=True, random_table).  A float32 distance widens exactly to the float64 search_truth takes
and narrows back unchanged."""
import numpy as np

import _graph_truth as G
import _pq_truth as P

NS = [1, 2, 65, 300, 3000]
DMS = [(4, 1), (15, 3), (64, 16), (2048, 16), (128, 64)]
KSS = [2, 7, 256]
RS = [1, 2, 32, 64]
EFS = [1, 2, 8, 64, 65, 2048]
KMODES = ["one", "ef"]
NQS = [1, 5, 130]
NES = [1, 3, 64]
OFFS = [0, 1000003]
CEILING = (3000, 128, 64, 256, 64, 2048, "ef", 1, 3, 0)       # the largest LDS carve the contract admits


def values(q, C, codes):
    """float32 [Q, n]: the ADC distance of every (query, row) pair, the bits of mi_pq_search."""
    return P.adc_truth(P.dtable64(q, C)[1], codes)


def decode(C, codes):
    """float32 [n, M * L]: the rows reconstructed, C[j][code[:, j]] side by side."""
    C = np.asarray(C, np.float32)
    codes = np.asarray(codes).astype(np.int64)
    return np.concatenate([C[j][codes[:, j]] for j in range(C.shape[0])], axis=1)


def search_truth(q, C, codes, table, entries, k, ef, row_offset=0):
    """-> (ids int64 [Q, k], dist float32 [Q, k], visited int32 [Q])."""
    ids, val, vis = G.search_truth(values(q, C, codes).astype(np.float64), table, entries, k, ef, True, row_offset)
    return ids, val.astype(np.float32), vis


def build_truth(C, codes, R, ne):
    """-> (table int32 [n, R], entries int32 [min(ne, n)]): mi_graph_build's definition over the ADC values of the decoded rows."""
    return G.build_truth(values(decode(C, codes), C, codes).astype(np.float64), R, ne, True)


def sweep_cases():
    """41 cases (n, d, M, Ks, R, ef, kmode, nq, ne, row_offset): 40 that touch every value of every axis, the number of queries
    dropping where the host truth would take more than a moment, and the LDS ceiling."""
    cases = []
    for i in range(40):
        n = NS[i % 5]
        d, M = DMS[(i + i // 5) % 5]
        Ks = KSS[(i + i // 7) % 3]
        R = RS[(i + i // 4) % 4]
        ef = EFS[(i + i // 6) % 6]
        nq = NQS[(i + i // 3) % 3]
        ne = NES[(i + i // 9) % 3]
        while nq > 1 and nq * n * min(ef, n) > 3e6:
            nq = NQS[NQS.index(nq) - 1]
        cases.append((n, d, M, Ks, R, ef, KMODES[(i + i // 2) % 2], nq, ne, OFFS[(i // 2) % 2]))
    return cases + [CEILING]


def case_id(c):
    return "n%d-d%d-M%d-Ks%d-R%d-ef%d-%s-q%d-e%d-off%d" % c


def case_inputs(case):
    """-> (C f32 [M, Ks, L], codes uint8 [n, M], q f32 [nq, d], table int32 [n, R], entries int32 [ne]), all seeded."""
    n, d, M, Ks, R, ef, _, nq, ne, _ = case
    rng = np.random.default_rng([n, d, M, Ks, R, ef, nq, ne])
    C = rng.standard_normal((M, Ks, d // M)).astype(np.float32)
    codes = rng.integers(0, Ks, size=(n, M)).astype(np.uint8)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return C, codes, q, G.random_table(rng, n, R), rng.integers(0, n, size=ne).astype(np.int32)
