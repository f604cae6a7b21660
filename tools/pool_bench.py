#!/usr/bin/env python3
"""The multi-hot lookup fused into the dot interaction (DLRMTrainer.fuse_pool)
timed on one MI355X against the two-launch path, in one process on the same batches
(bench.py measures the one-hot default and is not touched).

One trainer at a bench.py config (default terabyte = C3: B = 2048, D = 128, 26 tables) and two
families of multi-hot batches: 10 indices per bag, and bag lengths uniform in 1..10 (the
first ones of the same indices).  For each family: capture_predict() with fuse_pool off and on
for the fp32 tables, emb_bits=8 and emb_bits=4, and capture() of the training step off and on;
ms per replay over --nb batches in alternating windows (off, on, off, ..., --rounds of each)
after a clock preheat.  The spread between a mode's own windows is the yardstick for the
difference between the modes.  Before timing, the fused predict's probabilities are compared
with the unfused ones (max |difference|; at D = 128 and B > 1024 both run the same Gram
arithmetic on the same pooled values).

Writes one JSON document to --out and prints it.
python tools/pool_bench.py [--config terabyte] [--steps 200] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from embq_bench import _cycle, _trainer  # noqa: E402
from lr_sched_bench import _stats, _time_ms  # noqa: E402

LMAX = 10


def _ragged(tr, full, seed):
    """``full`` (LMAX indices per bag) cut to bag lengths uniform in 1..LMAX."""
    import torch
    from dlrm_hip.trainer import Batch
    g = torch.Generator(device=tr.dev).manual_seed(seed)
    nbags = full.offsets.numel() - 1
    lens = torch.randint(1, LMAX + 1, (nbags,), generator=g, device=tr.dev)
    keep = torch.arange(LMAX, device=tr.dev)[None, :] < lens[:, None]
    off = torch.zeros(nbags + 1, dtype=torch.int32, device=tr.dev)
    off[1:] = torch.cumsum(lens, 0)
    per_table = int(lens.view(tr.T_local, -1).sum(1).max())
    return Batch(full.X, off, full.indices.view(nbags, LMAX)[keep].contiguous(), full.target,
                 per_table, False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="terabyte")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nb", type=int, default=4, help="batches a window cycles through")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gpool = torch.cuda.graph_pool_handle()
    c = bench.CONFIGS[args.config]
    tr = _trainer(c, dev)
    for bits in (8, 4):
        tr.quantize_embedding(bits)
    fixed = [tr.synthetic_batch(c["B"], LMAX, seed=100 + i) for i in range(args.nb)]
    families = {"L10": fixed, "L1to10": [_ragged(tr, b, 7 + i) for i, b in enumerate(fixed)]}
    res = {"device": torch.cuda.get_device_name(dev), "config": args.config, "batch": c["B"],
           "steps_per_window": args.steps, "rounds": args.rounds, "batches": args.nb}
    for fam, batches in families.items():
        graphs, shift = {}, {}
        for what in ("predict32", "predict8", "predict4", "train"):
            for on in (False, True):
                tr.fuse_pool = on
                if what == "train":
                    for b in batches:  # eager: allocations
                        tr.step(b)
                    assert tr.pool_fused == on
                    torch.cuda.synchronize()
                    graphs[what, on] = [tr.capture(b, pool=gpool) for b in batches]
                else:
                    bits = int(what[7:])
                    p = tr.predict(batches[0], emb_bits=bits).clone()
                    if on:
                        shift[what] = float((p - ref).abs().max())
                    ref = p
                    torch.cuda.synchronize()
                    graphs[what, on] = [tr.capture_predict(b, pool=gpool, emb_bits=bits)
                                        for b in batches]
        tr.check_errors()
        bench.preheat_device(dev, 300.0)
        row = {}
        for what in ("predict32", "predict8", "predict4", "train"):
            win = {False: [], True: []}
            for _ in range(args.rounds):
                for on in (False, True):
                    win[on].append(_time_ms(_cycle(graphs[what, on]), args.steps, args.warmup))
            a, h = _stats(win[False]), _stats(win[True])
            row[what] = {"two_launches_ms": a, "fuse_pool_ms": h,
                         "fused_minus_unfused_us": round((h["median"] - a["median"]) * 1e3, 2),
                         "fused_over_unfused": round(h["median"] / a["median"], 4),
                         "outside_spread": bool(abs(h["median"] - a["median"])
                                                > max(a["spread"], h["spread"]))}
        res[fam] = {"lookups_per_batch": int(batches[0].indices.numel()), "ms_per_replay": row,
                    "max_prob_shift_fused_vs_unfused": shift}
        del graphs
    tr.check_errors()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
