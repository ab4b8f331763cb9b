"""Inputs and the fp64 restatement for the tests of ynet_score_rank_samples (tests/test_predict_host.py checks the generator on
the CPU, tests/test_gpu_predict.py runs the kernel against it)."""
import numpy as np

SEED = 20240611
KS, NWPS, BS = (1, 2, 20, 64), (1, 3), (1, 7, 128)
H, W, PRED = 40, 56, 12          # a non-square map


def make_case(K, n_wp, B, seed=SEED, H=H, W=W, pred_len=PRED):
    """Random prob in (0, 1), integer-valued samples (x, y) with duplicates (= exact score ties) planted, random trajectories."""
    rng = np.random.default_rng([seed, K, n_wp, B])
    prob = rng.uniform(1e-6, 1.0 - 1e-6, size=(B, n_wp, H, W)).astype(np.float32)
    prob = np.minimum(prob, np.float32(1.0 - 2.0 ** -24))
    wps = np.stack([rng.integers(0, W, size=(K, B, n_wp)), rng.integers(0, H, size=(K, B, n_wp))], axis=-1).astype(np.float32)
    if K >= 2:
        wps[K - 1] = wps[0]                       # the last sample repeats the first one: an exact tie in every agent
    if K >= 20:
        wps[7, ::2] = wps[3, ::2]                 # more duplicates, in every other agent; one triple
        wps[11, ::2] = wps[3, ::2]
        wps[K - 2, 1::3] = wps[K - 5, 1::3]
    trajs = (rng.standard_normal(size=(K, B, pred_len, 2)) * 20.0 + 30.0).astype(np.float32)
    return prob, wps, trajs


def score_fp64(prob, wps):
    """score[b, k] = sum over w of log(prob[b, w, y, x] + 1e-12) in fp64 -> [B, K]"""
    K, B, n_wp, _ = wps.shape
    x, y = wps[..., 0].astype(np.int64), wps[..., 1].astype(np.int64)
    b = np.arange(B)[None, :, None]
    w = np.arange(n_wp)[None, None, :]
    p = prob.astype(np.float64)[b, w, y, x]                      # [K, B, n_wp]
    return np.log(p + 1e-12).sum(axis=2).T


def rank_fp64(score):
    """descending, equal scores by ascending index -> order [B, K]"""
    return np.argsort(-score, axis=1, kind="stable")


def adjacent_pairs(score, order, n_wp):
    """Of the ranked fp64 scores: (gap to the next one, that gap is inside n_wp * 2^-20 * |score| but not an exact tie) -> two [B, K - 1] arrays"""
    s = np.take_along_axis(score, order, axis=1)
    gap = s[:, :-1] - s[:, 1:]
    tol = n_wp * 2.0 ** -20 * np.maximum(np.abs(s[:, :-1]), np.abs(s[:, 1:]))
    return gap, (gap <= tol) & (gap > 0)


def check_order(order_dev, score, n_wp):
    """The device's order against the fp64 ranking: it is a permutation per agent; every position holds a sample of the run of fp64
    neighbours closer than the gap that the position's fp64 sample belongs to (a run of one: the same sample); samples whose fp64
    scores are EQUAL come in index order.  -> fraction of adjacent pairs inside the gap"""
    B, K = score.shape
    order = rank_fp64(score)
    assert order_dev.shape == (B, K)
    assert (np.sort(order_dev, axis=1) == np.arange(K)[None]).all(), "order is not a permutation"
    gap, close = adjacent_pairs(score, order, n_wp)
    run = np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(~(close | (gap == 0)), axis=1)], axis=1)      # run id per fp64 position
    pos64 = np.empty_like(order)
    np.put_along_axis(pos64, order, np.broadcast_to(np.arange(K), (B, K)).copy(), axis=1)                   # sample -> fp64 position
    run_of_dev = np.take_along_axis(run, np.take_along_axis(pos64, order_dev, axis=1), axis=1)
    assert (run_of_dev == run).all(), "a sample is ranked across a gap that fp32 resolves"
    s_dev = np.take_along_axis(score, order_dev, axis=1)
    same = s_dev[:, :, None] == s_dev[:, None, :]
    later = np.arange(K)[None, :, None] < np.arange(K)[None, None, :]                                      # position i before position j
    wrong = same & later & (order_dev[:, :, None] > order_dev[:, None, :])
    assert not wrong.any(), "an exact tie is not in index order"
    return float(close.mean()) if K > 1 else 0.0
