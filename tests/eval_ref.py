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


def metrics_from_keys(keys):
    """dict(sorted, a2, n_pos, n_neg, groups, ap) of the packed keys (python integers)."""
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
    a2 = sum(int(p) * (2 * int(b) + int(q)) for p, b, q in zip(pos_g, neg_below, neg_g))
    ap = 0.0
    if P:
        tp = P - cpos[start]                  # positives scored >= group g
        terms = (pos_g.astype(np.float64) / P) * (tp.astype(np.float64) /
                                                  (n - start).astype(np.float64))
        ap = float(np.sum(terms[::-1]))       # from the highest score down
    return dict(sorted=srt, a2=int(a2), n_pos=P, n_neg=N, groups=int(start.size), ap=ap)


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
