"""numpy reference of the device evaluation metrics (test infrastructure): the packed-key
integer formulation of ROC-AUC and average precision, and the shared AUC/AP test inputs.

key = (float32_bits(prob) << 1) | label; sorted keys = ascending scores, negatives first
inside a tie group (a run of equal key >> 1).  For group g with pos_g / neg_g members and
neg_below_g negatives in lower-scored groups:
    A2      = sum_g pos_g * (2 * neg_below_g + neg_g)          (exact integer)
    roc_auc = A2 / (2 * P * N)
    ap      = sum_g (pos_g / P) * (TP_g / ALL_g), TP_g / ALL_g: positives / samples with a
              score >= group g's
"""
import math

import numpy as np


def pack_keys(prob, label):
    prob = np.ascontiguousarray(prob, dtype=np.float32).ravel()
    lab = np.asarray(label).ravel().astype(np.uint64)
    return ((prob.view(np.uint32).astype(np.uint64) << np.uint64(1)) | lab).astype(np.uint32)


def confusion(prob, label):
    """(tp, fp, tn, fn) at the threshold prob > 0.5f."""
    prob = np.asarray(prob, dtype=np.float32).ravel()
    lab = np.asarray(label).ravel() == 1
    pred = prob > np.float32(0.5)
    return (int(np.sum(pred & lab)), int(np.sum(pred & ~lab)), int(np.sum(~pred & ~lab)),
            int(np.sum(~pred & lab)))


def _a2_slow(pos_g, neg_below, neg_g):
    """A2 in python integers, one group at a time: what metrics_from_keys' vectorised int64
    sum must return (tests/test_eval_cpu.py)."""
    return sum(int(p) * (2 * int(b) + int(q)) for p, b, q in zip(pos_g, neg_below, neg_g))


def metrics_from_keys(keys, slow=False):
    """dict(sorted, a2, n_pos, n_neg, groups, ap, ap_fsum) of the packed keys (python
    integers).  ``ap`` is numpy's float64 sum of the groups' terms from the highest score
    down, ``ap_fsum`` the exactly rounded sum (math.fsum) of the same terms.  Vectorised, so
    millions of groups cost a sort and a few passes (``slow``: A2 by _a2_slow)."""
    srt = np.sort(np.asarray(keys, dtype=np.uint32), kind="stable")
    n = srt.size
    lab = (srt & np.uint32(1)).astype(np.int64)
    score = srt >> np.uint32(1)
    start = np.flatnonzero(np.r_[True, score[1:] != score[:-1]]) if n else np.zeros(0, np.int64)
    end = np.r_[start[1:], n]
    cpos = np.r_[0, np.cumsum(lab)]           # positives before index i
    pos_g = cpos[end] - cpos[start]
    neg_g = (end - start) - pos_g
    neg_below = start - cpos[start]
    P = int(cpos[-1])
    N = n - P
    # every term pos_g * (2 neg_below + neg_g) and every partial sum is at most 2 P N
    assert 2 * P * N < 2 ** 62, "A2 would not fit the int64 sum"
    if slow:
        a2 = _a2_slow(pos_g, neg_below, neg_g)
    else:
        assert pos_g.dtype == neg_below.dtype == neg_g.dtype == np.int64
        a2 = int(np.sum(pos_g * (2 * neg_below + neg_g), dtype=np.int64))
    ap = ap_fsum = 0.0
    if P:
        tp = P - cpos[start]                  # positives scored >= group g
        terms = (pos_g.astype(np.float64) / P) * (tp.astype(np.float64) /
                                                  (n - start).astype(np.float64))
        ap = float(np.sum(terms[::-1]))       # from the highest score down
        ap_fsum = math.fsum(terms)
    return dict(sorted=srt, a2=int(a2), n_pos=P, n_neg=N, groups=int(start.size), ap=ap,
                ap_fsum=ap_fsum)


def full(prob, label):
    """Every number the device path reports, from probabilities and labels."""
    out = metrics_from_keys(pack_keys(prob, label))
    tp, fp, tn, fn = confusion(prob, label)
    out.update(tp=tp, fp=fp, tn=tn, fn=fn)
    if out["n_pos"] and out["n_neg"]:
        out["roc_auc"] = out["a2"] / (2 * out["n_pos"] * out["n_neg"])
    out["recall"] = tp / (tp + fn) if tp + fn else 0.0
    out["precision"] = tp / (tp + fp) if tp + fp else 0.0
    out["f1"] = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else 0.0
    out["accuracy"] = (tp + tn) / max(tp + fp + tn + fn, 1)
    return out


def auc_ap_inputs(tile):
    """The shared AUC/AP inputs: [(name, prob float32 [n], label float32 [n])].  Labels are
    Bernoulli(0.3) with a fixed seed (both classes present for every n >= 2 listed)."""
    cases = []
    big = 70001

    def labels(n, seed):
        return (np.random.RandomState(seed).rand(n) < 0.3).astype(np.float32)

    for n in (1, 2, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1):
        rng = np.random.RandomState(1000 + n)
        cases.append((f"n{n}", rng.rand(n).astype(np.float32), labels(n, 3 + n)))
    rng = np.random.RandomState(11)
    distinct = rng.permutation(big).astype(np.float32) / np.float32(big)  # all different
    cases.append(("distinct", distinct, labels(big, 12)))
    q = (np.random.RandomState(13).randint(0, 8, big).astype(np.float32) + 0.5) / np.float32(8)
    cases.append(("quant8", q, labels(big, 14)))
    cases.append(("equal", np.full(big, 0.375, np.float32), labels(big, 15)))
    half = np.random.RandomState(16).rand(big).astype(np.float32)
    half[:big // 7] = 0.5
    half[big // 7] = 0.0
    half[big // 7 + 1] = 1.0
    half[big // 7 + 2] = 0.0
    half[big // 7 + 3] = 1.0
    cases.append(("half", half, labels(big, 17)))
    return cases


MAX_SORT_WGS = 1024  # metrics.hip kMaxSortWgs: workgroups of a sort pass


def sort_plan(n, tile):
    """(ntiles, tiles_per_wg, wgs) of metrics.hip's sort_plan for n keys."""
    ntiles = -(-max(n, 1) // tile)
    per_wg = -(-ntiles // MAX_SORT_WGS)
    return ntiles, per_wg, -(-ntiles // per_wg)


BIG_NAMES = ("big_distinct", "big_ties", "big_three")


def big_input(name, tile):
    """(prob float32 [n], label float32 [n]) of an input above MAX_SORT_WGS * tile keys, where
    every sort workgroup owns a run of tiles.  Kept out of auc_ap_inputs, whose callers run
    every case several times.
      big_distinct  1024 tiles + 1 key: 2 tiles per workgroup, the last workgroup one tile of
                    one key; the scores a permutation of i / n, all different (n < 2^24)
      big_ties      the same plan; 1000 score levels, so the tie groups cross every tile and
                    workgroup boundary
      big_three     2 * 1024 + 3 tiles + 7 keys: 3 tiles per workgroup; random scores, one
                    seventh of them 0.5"""
    seed = 100 + BIG_NAMES.index(name)
    rng = np.random.RandomState(seed)
    n = MAX_SORT_WGS * tile + 1 if name != "big_three" else (2 * MAX_SORT_WGS + 3) * tile + 7
    lab = (np.random.RandomState(seed + 10).rand(n) < 0.3).astype(np.float32)
    if name == "big_distinct":
        assert n < 2 ** 24
        prob = rng.permutation(n).astype(np.float32) / np.float32(n)
    elif name == "big_ties":
        prob = (rng.randint(0, 1000, n).astype(np.float32) + np.float32(0.5)) / np.float32(1000)
    else:
        prob = rng.rand(n).astype(np.float32)
        prob[rng.permutation(n)[:n // 7]] = 0.5
    return prob, lab
