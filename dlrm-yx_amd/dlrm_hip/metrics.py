"""Evaluation metrics on the device: a log of scored samples and the reference's
validation results from it (dlrm_s_pytorch.py:1093-1108: recall, precision, f1, ap, roc_auc,
accuracy - there via sklearn on every probability copied to the host).

Each scored sample is one uint32 key, (float_bits(prob) << 1) | label, appended by the
forward-only head (ops.head_predict) or by ``EvalState.update``; the confusion counts are
kept beside the log.  ``compute()`` sorts the keys (dlrm_eval_metrics) and reads back a few
integers; ``finalize`` turns them into the ratios on the host.
"""
from __future__ import annotations

import struct
from typing import Optional

import torch

from . import _lib, ops

ERR_OVERFLOW, ERR_SCORE, ERR_LABEL = 1, 2, 4  # dlrm_eval_error bits
_CURSOR, _TP, _FP, _TN, _FN, _ERR = range(6)  # slots of the int64 control block


def _ratio(num: int, den: int) -> float:
    return num / den if den else 0.0  # sklearn's zero_division value (it also warns)


def finalize(tp: int, fp: int, tn: int, fn: int, auc_num2: int, n_pos: int, n_neg: int,
             ap: float) -> dict:
    """The reference's validation results from the raw integers: tp/fp/tn/fn at the
    threshold prob > 0.5 (= np.round(prob) == 1), auc_num2 = sum over tie groups of
    pos_g (2 neg_below_g + neg_g), n_pos / n_neg the class sizes, ap the average-precision
    sum.  Raises ValueError when only one class was logged (roc_auc is undefined: sklearn
    raises there too); precision / recall / f1 with a zero denominator are 0.0."""
    tp, fp, tn, fn = int(tp), int(fp), int(tn), int(fn)
    auc_num2, n_pos, n_neg = int(auc_num2), int(n_pos), int(n_neg)
    if n_pos == 0 or n_neg == 0:
        raise ValueError("only one class present in the logged labels: roc_auc is not defined")
    return {
        "recall": _ratio(tp, tp + fn),
        "precision": _ratio(tp, tp + fp),
        "f1": _ratio(2 * tp, 2 * tp + fp + fn),
        "ap": float(ap),
        "roc_auc": auc_num2 / (2 * n_pos * n_neg),
        "accuracy": _ratio(tp + tn, tp + fp + tn + fn),
        "tp": tp, "fp": fp, "tn": tn, "fn": fn,
        "auc_num2": auc_num2, "n_pos": n_pos, "n_neg": n_neg,
    }


def _raise_error_bits(err: int) -> None:
    if err & ERR_OVERFLOW:
        raise OverflowError("evaluation log overflow: an update did not fit the capacity "
                            "(it logged nothing)")
    if err & ERR_SCORE:
        raise ValueError("evaluation log: a probability outside [0, 1] or NaN (row skipped)")
    if err & ERR_LABEL:
        raise ValueError("evaluation log: a label that is not exactly 0 or 1 (row skipped)")


class EvalState:
    """Device log of up to ``capacity`` scored samples.  ``keys``: an int32 device tensor
    of ``capacity`` elements to use as the log (default: a new one)."""

    def __init__(self, capacity: int, device="cuda:0", keys: Optional[torch.Tensor] = None):
        self.capacity = int(capacity)
        if self.capacity <= 0:
            raise ValueError("EvalState: capacity must be positive")
        self.dev = torch.device(device)
        if keys is None:
            keys = torch.empty(self.capacity, dtype=torch.int32, device=self.dev)
        elif (keys.dtype != torch.int32 or keys.numel() != self.capacity
              or not keys.is_contiguous() or not keys.is_cuda):
            raise ValueError("EvalState: keys must be a contiguous int32 device tensor of "
                             "capacity elements")
        self.keys = keys
        # cursor, TP, FP, TN, FN, error word (its low 32 bits), 2 spare
        self.ctrl = torch.zeros(8, dtype=torch.int64, device=self.dev)
        self._c = _lib.EvalStateC(self.keys.data_ptr(), self.capacity, self.ctrl.data_ptr(),
                                  self.ctrl.data_ptr() + 8 * _TP, self.ctrl.data_ptr() + 8 * _ERR)
        self.last_out: Optional[torch.Tensor] = None  # dlrm_eval_metrics' integers

    def c_struct(self):
        return self._c

    def reset(self) -> None:
        """Empty the log and clear the counts and error bits (enqueues only)."""
        self.ctrl.zero_()

    def update(self, prob: torch.Tensor, target: torch.Tensor) -> None:
        """Log probabilities that already exist (e.g. the reference driver's Z_test, T_test)."""
        ops.eval_update(prob.to(self.dev, torch.float32), target.to(self.dev, torch.float32),
                        self)

    @property
    def count(self) -> int:
        """Samples logged so far (synchronises)."""
        return int(self.ctrl[_CURSOR].item())

    def compute(self, group=None) -> dict:
        """The reference's validation results over everything logged (synchronises; sorts the
        log in place - later updates still append after it).  ``group``: a process group
        whose ranks each logged their own samples; the counts and logs of all ranks are
        gathered and every rank returns the same dict."""
        ctrl = self.ctrl.cpu().tolist()
        if group is None:
            err = ctrl[_ERR] & 0xFFFFFFFF
            _raise_error_bits(err)
            n, keys = ctrl[_CURSOR], self.keys
            counts = ctrl[_TP:_FN + 1]
        else:
            n, keys, counts, err = self._gather(group, ctrl)
            _raise_error_bits(err)
        if n == 0:
            raise ValueError("no samples logged")
        need = _lib.query("dlrm_eval_metrics_workspace_size", n)
        ws = torch.empty(need, dtype=torch.uint8, device=self.dev)  # freed after this call
        self.last_out = ops.eval_metrics(keys, n, workspace=ws)
        a2, n_pos, n_neg, _groups, ap_bits = self.last_out.cpu().tolist()
        ap = struct.unpack("<d", struct.pack("<q", ap_bits))[0]
        return finalize(*counts, a2, n_pos, n_neg, ap)

    def _gather(self, group, ctrl):
        """All ranks' control blocks, then their logs padded to the longest (staged through
        the host on gloo, which has no device collectives)."""
        import torch.distributed as dist
        W = dist.get_world_size(group)
        host = dist.get_backend(group) == "gloo"
        cdev = torch.device("cpu") if host else self.dev
        mine = torch.tensor(ctrl, dtype=torch.int64, device=cdev)
        allc = [torch.empty_like(mine) for _ in range(W)]
        dist.all_gather(allc, mine, group=group)
        allc = [c.cpu().tolist() for c in allc]
        err = 0
        for c in allc:
            err |= c[_ERR] & 0xFFFFFFFF
        counts = [sum(c[k] for c in allc) for k in (_TP, _FP, _TN, _FN)]
        lens = [c[_CURSOR] for c in allc]
        longest = max(max(lens), 1)
        pad = torch.zeros(longest, dtype=torch.int32, device=cdev)
        pad[:lens[dist.get_rank(group)]] = self.keys[:lens[dist.get_rank(group)]].to(cdev)
        parts = [torch.empty_like(pad) for _ in range(W)]
        dist.all_gather(parts, pad, group=group)
        union = torch.cat([p[:m] for p, m in zip(parts, lens)]).to(self.dev)
        return sum(lens), union.contiguous(), counts, err
