"""CPU: the premises of tests/_margin_truth_sharded.py for every case tests/test_gpu_certificate_margin_sharded.py runs -- the
rows are exact and round to the intended 16-bit values (torch's .half() / .bfloat16()), the 16-bit scores are whole units in any
summation order, the layout is what the module says (a split pattern's imposters and victims on different loud shards, the quiet
shard holds fillers and f' victims only) -- and the proof that the GPU test fails on a subtly wrong protocol: the host model
equals the truth with the agreed maxima and the whole margin, loses a victim for EVERY quiet query when each shard cuts with its
own maxima, loses a victim for EVERY split query at 0.85 of the margin, and counts exactly 2 K candidates per query over the
shards.  The achieved tightness is printed; DESIGN 3 records it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _margin_truth as mt  # noqa: E402
import _margin_truth_sharded as ms  # noqa: E402

FLOOR = 0.85
IDS = ["d%d-%s-n%d" % c[:3] for c in ms.CASES]


@pytest.fixture(params=ms.CASES, ids=IDS)
def prob(request):
    return ms.problem(*request.param)


def _lost(got, want):
    return [len(set(w.tolist()) - set(g.tolist())) for g, w in zip(got, want)]


def test_layout(prob):
    assert prob.bounds == [(0, 6000), (6000, 12000), (12000, 18000)] and prob.quiet.sum() == prob.patterns // 2
    for p in range(prob.patterns):
        si, sv = set(prob.shard_of(prob.imposters[p]).tolist()), set(prob.shard_of(prob.victims[p]).tolist())
        assert len(si) == 1 and len(sv) == 1 and si != sv and si <= {0, 1}
        assert sv == ({ms.QUIET_SHARD} if prob.quiet[p] else {1 - si.pop()})
    # both directions: a split and a quiet pattern with the imposters on shard 0, and on shard 1
    for quiet in (False, True):
        assert set(prob.imposter_shard[prob.quiet == quiet].tolist()) == {0, 1}
    lo, hi = prob.bounds[ms.QUIET_SHARD]
    kinds = prob.kind[lo:hi]
    assert set(kinds.tolist()) == {mt.FILLER, mt.VICTIM} and (prob.fnum[lo:hi][kinds == mt.VICTIM] == ms.QUIET_NUM).all()
    assert (prob.kind == mt.VICTIM).sum() == (prob.kind == mt.IMPOSTER).sum() == prob.patterns * prob.k
    assert (np.abs(prob.fnum[prob.kind != mt.FILLER][prob.shard_of(np.flatnonzero(prob.kind != mt.FILLER)) < 2]) == mt.F_NUM).all()


def test_rows_and_queries_round_to_the_intended_16_bit_values(prob):
    import torch
    cast = (lambda t: t.half()) if prob.image == "f16" else (lambda t: t.bfloat16())
    for a, ah in ((prob.X, prob.Xh), (prob.base_queries(0), prob.base_queries(0))):
        back = cast(torch.from_numpy(a)).float().numpy()
        assert np.array_equal(back.view(np.uint32), ah.view(np.uint32))
    fm = mt.FORMATS[prob.image]
    m = np.abs(prob.Xh.astype(np.float64)) / prob.ulp
    assert (m == np.round(m)).all() and m.min() >= fm["lo"] and m.max() <= fm["hi"]
    assert (prob.X_int.astype(np.float64) * prob.grid == prob.X.astype(np.float64)).all()                # values are exact
    # what the image drops: t f ulp on EVERY column against sigma, f = 31/64 (8/64 for a quiet victim), nothing for a filler
    drop = (prob.Xh.astype(np.float64) - prob.X.astype(np.float64)) / prob.ulp
    sig = np.where(prob.pattern[:, None] >= 0, prob.sigma[prob.pattern], 0)
    assert np.array_equal(drop, -(prob.fnum / mt.F_DEN)[:, None] * sig)
    if prob.image == "f16":
        assert max(prob.shard_norm_bounds(r)[0] for r in range(ms.SHARDS)) <= 4.0
    # the quiet shard's own max |g^ - g| is f' ulp sqrt(d), a loud shard's f ulp sqrt(d); the agreement takes the loud one
    for r in range(ms.SHARDS):
        num = ms.QUIET_NUM if r == ms.QUIET_SHARD else mt.F_NUM
        want = np.float32(num / mt.F_DEN * prob.ulp * np.sqrt(prob.d) * (1.0 + 1e-6))
        assert prob.shard_norm_bounds(r)[2] == want
    assert np.array_equal(np.array(prob.agreed_bounds(), np.float32), np.array(prob.norm_bounds(), np.float32))
    assert prob.agreed_bounds()[2] == prob.shard_norm_bounds(0)[2] == prob.shard_norm_bounds(1)[2]


def test_scores_are_whole_units_in_any_order(prob):
    qh = mt.round16(prob.base_queries(0), prob.image)
    want = prob.approx().astype(np.float32)
    assert np.array_equal(want.astype(np.float64), prob.approx())
    units = prob.approx() / prob.unit
    assert np.array_equal(units, np.round(units))

    def acc(cols):
        s = np.zeros((prob.patterns, prob.n), np.float32)
        for j in cols:
            s += qh[:, j][:, None] * prob.Xh[:, j][None, :]
        return s

    half = prob.d // 2
    for got in (acc(range(prob.d)), acc(range(prob.d - 1, -1, -1)), acc(range(half)) + acc(range(half, prob.d))):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    q, x = prob.base_queries(0).astype(np.float64), prob.X.astype(np.float64)
    assert np.array_equal(q @ x.T, prob.exact()) and np.array_equal(q[:, ::-1] @ x[:, ::-1].T, prob.exact())


def test_truth_is_the_victims_and_the_gathered_kth_the_imposters_level(prob):
    ids, sc = prob.truth()
    A, S = prob.approx(), prob.exact()
    top16 = np.argsort(-A, axis=1, kind="stable")[:, :prob.k]
    assert [set(r.tolist()) for r in ids] == [set(r.tolist()) for r in prob.victims]
    assert [set(r.tolist()) for r in top16] == [set(r.tolist()) for r in prob.imposters]
    L = prob.gathered_kth()
    assert np.array_equal(L, prob.kth_approx()) and (L == prob.T * prob.unit).all()
    for p in range(prob.patterns):
        assert S[p][prob.victims[p]].min() > S[p][prob.imposters[p]].max()
        below = (prob.T * prob.unit - A[p][prob.victims[p]].min()) / prob.unit
        lo = prob.vq_low if prob.quiet[p] else prob.v_low
        assert below == prob.T - lo
        rest = np.ones(prob.n, bool)
        rest[prob.victims[p]] = rest[prob.imposters[p]] = False
        assert A[p][rest].max() < A[p][prob.victims[p]].min() - 8 * prob.shard_margin()[p]                 # far below the band
    # the victims' own shard never sees L among its rows: its K-th 16-bit score is far below the gathered one
    for p in range(prob.patterns):
        lo, hi = prob.bounds[prob.victim_shard[p]]
        assert -np.partition(-A[p, lo:hi], prob.k - 1)[prob.k - 1] < L[p]


def test_tightness_and_what_a_wrong_protocol_loses(prob):
    ids, sc = prob.truth()
    split, quiet = ~prob.quiet, prob.quiet
    agreed = prob.tightness_against()
    own = prob.tightness_against(ms.QUIET_SHARD)
    clear = prob.cut_clearance()
    unit_margin = prob.shard_margin() / prob.unit
    print("\n%s d %d: split patterns need %.4f .. %.4f of the agreed margin (%.2f units); quiet patterns %.4f .. %.4f of the agreed "
          "margin and %.4f .. %.4f of the quiet shard's own (%.2f units); lowest quiet victim %d units below L; nearest score "
          "to a cut %.2f units" % (prob.image, prob.d, agreed[split].min(), agreed[split].max(), unit_margin[0], agreed[quiet].min(),
                                   agreed[quiet].max(), own[quiet].min(), own[quiet].max(),
                                   prob.shard_margin(ms.QUIET_SHARD)[0] / prob.unit, prob.T - prob.vq_low, clear))
    assert agreed[split].min() >= FLOOR and agreed.max() < 1.0
    # the quiet victims: well outside their shard's own margin, inside the agreed one at (f + f') / (2 f) of it, less what the
    # gamma term, the 1.001 and the one unit add
    assert own[quiet].min() > 2.0
    ratio = (mt.F_NUM + ms.QUIET_NUM) / (2.0 * mt.F_NUM)
    assert 0.93 * ratio < agreed[quiet].min() and agreed[quiet].max() < ratio
    # the f32 cut L - margin of the device cannot fall on the other side of a row: L is exact, the one subtraction rounds by at
    # most 2^-24 T units
    assert clear > 0.05 and 2.0 ** -24 * prob.T < 0.01

    got = prob.protocol(1.0)
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], sc)
    assert (got[2].sum(1) == 2 * prob.k).all()                   # exactly 2 K rows within the agreed margin of L, over the shards
    for p in range(prob.patterns):                               # K on the imposters' shard, K on the victims', none elsewhere
        want = np.zeros(ms.SHARDS, np.int64)
        want[prob.imposter_shard[p]] += prob.k
        want[prob.victim_shard[p]] += prob.k
        assert np.array_equal(got[2][p], want)
    # each shard cutting with its OWN maxima: every quiet query loses a victim (the split ones, on loud shards, do not)
    lost = np.array(_lost(prob.protocol(1.0, own=True)[0], ids))
    assert (lost[quiet] > 0).all() and (lost[split] == 0).all()
    # 0.85 of the agreed margin: every split query loses a victim (the quiet ones need 0.62 and keep theirs)
    lost = np.array(_lost(prob.protocol(0.85)[0], ids))
    assert (lost[split] > 0).all() and (lost[quiet] == 0).all()
    # half the margin loses victims of both kinds
    assert (np.array(_lost(prob.protocol(0.5)[0], ids)) > 0).all()


def test_per_shard_lists_and_batches(prob):
    ids, sc, count, sid, ssc = prob.protocol(1.0)
    for p in range(prob.patterns):
        for r in range(ms.SHARDS):
            rows = sid[r, p][sid[r, p] >= 0]
            lo, hi = prob.bounds[r]
            assert len(rows) == min(prob.k, count[p, r]) and ((rows >= lo) & (rows < hi)).all()
        assert set(ids[p].tolist()) <= set(sid[prob.victim_shard[p], p].tolist())
    nq = 2 * prob.patterns + 3
    assert np.array_equal(prob.truth(nq=nq)[0][prob.patterns + 1], ids[1])
    assert np.array_equal(ms.shard_bounds(10, 3, 2), (8, 10)) and ms.shard_bounds(2, 3, 2) == (2, 2)
