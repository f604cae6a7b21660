"""Generate tests/golden/lr_schedule.json from the reference's own LRPolicyScheduler
(dlrm_s_pytorch.py:188-222).

Runs only where the reference sources are available (it imports them through
make_golden.import_reference).  For every configuration (base, W, S, D) - base learning
rate, --lr-num-warmup-steps, --lr-decay-start-step, --lr-num-decay-steps - the reference
class drives a dummy torch.optim.SGD exactly as the training loop does (the rate in effect
for iteration i is param_groups[0]["lr"] before the i-th lr_scheduler.step(); the scheduler's
_step_count is then i + 1, because the torch base class steps once in its constructor).
The file records those rates as exact doubles (float.hex()).

Usage:  python tests/golden/make_golden_lr.py [--ref /root/reference]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# every iteration recorded, to at least three past S + D
SMALL = [(0.1, 4, 6, 5), (24.0, 5, 5, 3), (1.0, 0, 0, 0), (1.0, 3, 3, 0), (0.3, 7, 9, 11),
         (1.0, 0, 0, 4), (1e-6, 2, 2, 50)]
# the MLPerf Terabyte shape: one scheduler stepped through, only these step counts kept
MLPERF = (24.0, 2750, 49315, 27772)
MLPERF_SC = [1, 2, 2749, 2750, 2751, 49314, 49315, 49316, 77086, 77087, 77088, 100000]


def run(R, base, W, S, D, n_iter):
    """[(step_count, lr)] for iterations 1..n_iter of the reference scheduler."""
    import torch
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=base)
    sched = R.ref.LRPolicyScheduler(opt, W, S, D)
    out = []
    for _ in range(n_iter):
        out.append((int(sched._step_count), float(opt.param_groups[0]["lr"])))
        opt.step()
        sched.step()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    from make_golden import import_reference
    R = import_reference(args.ref)
    import warnings
    warnings.simplefilter("ignore")
    configs = []
    for base, W, S, D in SMALL:
        rec = run(R, base, W, S, D, S + D + 4)
        assert [sc for sc, _ in rec] == list(range(1, len(rec) + 1))
        configs.append(dict(base=float(base).hex(), W=W, S=S, D=D,
                            step_counts=[sc for sc, _ in rec],
                            lr=[v.hex() for _, v in rec]))
    base, W, S, D = MLPERF
    rec = dict(run(R, base, W, S, D, max(MLPERF_SC)))
    configs.append(dict(base=float(base).hex(), W=W, S=S, D=D, step_counts=MLPERF_SC,
                        lr=[rec[sc].hex() for sc in MLPERF_SC]))
    path = os.path.join(HERE, "lr_schedule.json")
    with open(path, "w") as f:
        json.dump(dict(source="LRPolicyScheduler, dlrm_s_pytorch.py:188-222",
                       note="lr[i] is param_groups[0]['lr'] while _step_count == "
                            "step_counts[i]; doubles as float.hex()",
                       configs=configs), f, indent=1)
        f.write("\n")
    print("wrote", path, len(configs), "configurations")


if __name__ == "__main__":
    main()
