"""Inputs and fp64 restatements for the tests of the style bank's two kernels (tests/test_style_bank_host.py checks them on the
CPU, tests/test_gpu_style_bank.py runs the kernels against them).  The score inputs are those of tests/_predict_cases.py."""
import numpy as np

import _predict_cases as C

PERMS = ("identity", "reversed", "random")
GATHER_LS = (1, 2, 3, 40, 4096)


def out_rows(kind, B, seed=C.SEED):
    if kind == "identity":
        return np.arange(B)
    if kind == "reversed":
        return np.arange(B)[::-1].copy()
    return np.random.default_rng([seed, B, 17]).permutation(B)


def rank_rows_fp64(prob, wps, trajs, out_row, resize_factor):
    """ynet_score_rank_samples_rows restated: agent b is scored and ranked as ynet_score_rank_samples does (fp64 scores, descending,
    equal scores by ascending index) and its results are stored at row out_row[b].
    -> score [B, K] in SAMPLE order at the output rows, order [B, K], ranked [B, K, pred, 2] (fp32 product with the fp32 reciprocal,
    as the kernel forms it), goals [B, K, n_wp, 2]"""
    score = C.score_fp64(prob, wps)                                   # [B, K] by batch row
    order = C.rank_fp64(score)
    B, K = score.shape
    inv = np.float32(1.0 / float(resize_factor))
    cols = np.arange(B)[:, None]
    ranked = trajs.transpose(1, 0, 2, 3)[cols, order] * inv           # [B, K, pred, 2]
    goals = wps.transpose(1, 0, 2, 3)[cols, order]
    out = [np.empty_like(a) for a in (score, order, ranked, goals)]
    for o, a in zip(out, (score, order, ranked, goals)):
        o[out_row] = a
    return out


def gather_case(L, n_src, n, seed=C.SEED):
    """A source of n_src rows of L floats (every float distinct), n indices with repeats planted."""
    rng = np.random.default_rng([seed, L, n_src, n])
    src = (rng.permutation(n_src * L).astype(np.float32) - np.float32(0.5 * n_src * L)).reshape(n_src, L)      # (n_src * L < 2^24: exact)
    idx = rng.integers(0, n_src, size=n)
    idx[-1] = idx[0]
    if n > 2:
        idx[n // 2] = idx[0]
    return src, idx
