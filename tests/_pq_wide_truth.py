"""Pure-numpy truth of the wide PQ index (tests only).  Tables, ADC sums and order are _pq_truth's as they stand (they do not depend
on Ks); the encoder and the training are restated here because _pq_truth.encode_truth returns bytes: the same sentences with
uint16 codes, and the rows passing in blocks so that Ks = 8192 stays within a few hundred MiB."""
import numpy as np

from _pq_truth import dtable64
from _pq_train_truth import update_truth


def encode_truth16(x, C, block=1024):
    """-> uint16 [N, M]: np.argmin of the float64 sums of dtable64, ties to the lower codeword (argmin returns the first)."""
    x = np.asarray(x)
    C = np.asarray(C, np.float32)
    out = np.empty((x.shape[0], C.shape[0]), np.uint16)
    for r in range(0, out.shape[0], block):
        out[r:r + block] = np.argmin(dtable64(x[r:r + block], C)[0], axis=-1)
    return out


def train_truth16(x, M, Ks, iters, C0):
    """_pq_train_truth.train_truth with encode_truth16 -> (C float32 [M, Ks, L], moved int64 [iters], emptied): emptied counts
    the (iteration, book, codeword) triples that had no member at an update."""
    x = np.asarray(x)
    C = np.ascontiguousarray(C0, dtype=np.float32).copy()
    assert C.shape == (M, Ks, x.shape[1] // M)
    moved = np.zeros(iters, np.int64)
    prev, emptied = None, 0
    for t in range(iters):
        codes = encode_truth16(x, C)
        moved[t] = codes.size if prev is None else int((codes != prev).sum())
        if t > 0 and moved[t] == 0:
            break
        emptied += sum(int(Ks - np.unique(codes[:, j]).size) for j in range(M))
        C = update_truth(x, codes, C)
        prev = codes
    return C, moved, emptied
