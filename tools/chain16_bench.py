#!/usr/bin/env python3
"""The 16-bit bottom-MLP chain (DLRMTrainer.fuse_bottom16) timed on one MI355X
against the per-layer dlrm_linear16_forward launches, in one process on the same batches
(bench.py measures the fp32 default and is not touched).

One trainer at a bench.py config (default terabyte = C3 at true rows: B = 2048, bottom MLP
13 -> 512 -> 256 -> 128) with mlp_precision="bf16".  With fuse_bottom16 off and on:
capture_predict() in bf16 and in fp16 and capture() of the bf16 training step, ms per replay
over --nb batches in alternating windows (off, on, off, ..., --rounds of each) after a clock
preheat; and the bottom MLP alone on the trainer's own views, as a graph of the per-layer
launches against a graph of the one chain launch.  The spread between a mode's own windows is
the yardstick for the difference between the modes.  Before timing, the fused predict's
probabilities are compared with the unfused ones (the contract is bit equality).

Writes one JSON document to --out and prints it.
python tools/chain16_bench.py [--config terabyte] [--steps 200] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from embq_bench import _cycle  # noqa: E402
from lr_sched_bench import _stats, _time_ms  # noqa: E402

KINDS = ("predict_bf16", "predict_fp16", "train_bf16", "bottom_bf16", "bottom_fp16")


def _bottom_graph(tr, batch, dtype, fused):
    """The bottom MLP alone, captured: the trainer's weights, one output buffer per layer."""
    import torch
    from dlrm_hip import ops
    outs = [torch.empty(batch.X.shape[0], L.N, device=tr.dev) for L in tr.bot]
    chain = ops.mlp_chain16(batch.X[:, :tr.bot[0].K],
                            [(L.W[:, :L.K], L.b, y) for L, y in zip(tr.bot, outs)], dtype=dtype)

    def run():
        if fused:
            return ops.mlp_chain16_forward(chain, tr.dev)
        h = batch.X
        for L, y in zip(tr.bot, outs):
            h = ops.linear16_forward(h[:, :L.K], L.W[:, :L.K], L.b, relu=True, out=y, dtype=dtype)

    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.keep = (outs, chain)
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="terabyte")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nb", type=int, default=4, help="batches a window cycles through")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain16_bench.json"))
    args = ap.parse_args()
    import torch
    import bench
    from train16_bench import _trainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gpool = torch.cuda.graph_pool_handle()
    c, tr = _trainer(args.config, dev, "bf16")
    batches = [tr.synthetic_batch(c["B"], c["L"], seed=100 + i) for i in range(args.nb)]
    res = {"device": torch.cuda.get_device_name(dev), "config": args.config, "batch": c["B"],
           "bottom": c["bot"], "steps_per_window": args.steps, "rounds": args.rounds,
           "batches": args.nb}
    graphs, equal = {}, {}
    for what in KINDS:
        kind, dtype = what.split("_")
        for on in (False, True):
            tr.fuse_bottom16 = on
            if kind == "train":
                for b in batches:  # eager: allocations
                    tr.step(b)
                assert tr.bottom16_fused == on
                torch.cuda.synchronize()
                graphs[what, on] = [tr.capture(b, pool=gpool) for b in batches]
            elif kind == "predict":
                p = tr.predict(batches[0], precision=dtype).clone()
                assert tr.bottom16_fused == on
                if on:
                    equal[what] = bool(torch.equal(p, ref))
                ref = p
                torch.cuda.synchronize()
                graphs[what, on] = [tr.capture_predict(b, pool=gpool, precision=dtype)
                                    for b in batches]
            else:
                graphs[what, on] = [_bottom_graph(tr, b, dtype, on) for b in batches]
    tr.check_errors()
    bench.preheat_device(dev, 300.0)
    row = {}
    for what in KINDS:
        win = {False: [], True: []}
        for _ in range(args.rounds):
            for on in (False, True):
                win[on].append(_time_ms(_cycle(graphs[what, on]), args.steps, args.warmup))
        a, h = _stats(win[False]), _stats(win[True])
        row[what] = {"per_layer_ms": a, "chain16_ms": h,
                     "chain_minus_per_layer_us": round((h["median"] - a["median"]) * 1e3, 2),
                     "chain_over_per_layer": round(h["median"] / a["median"], 4),
                     "outside_spread": bool(abs(h["median"] - a["median"])
                                            > max(a["spread"], h["spread"]))}
    res["ms_per_replay"] = row
    res["predict_probabilities_bit_equal"] = equal
    tr.check_errors()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
