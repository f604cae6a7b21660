#!/usr/bin/env python3
"""int8 dynamic-quantized MLP layers for inference (DLRMTrainer.quantize_mlp(8),
predict(mlp_bits=8)) timed on one MI355X (bench.py measures the fp32 training
default and is not touched):

  step  : one trainer at a bench.py config (default terabyte = C3: B = 2048, true rows),
          capture_predict() of the forward-only pass over 10 batches for fp32, bf16 and
          mlp_bits=8, ms per replay in alternating windows (fp32, bf16, int8, fp32, ...,
          --rounds of each) after a clock preheat: the spread between a mode's own windows is
          the yardstick for the difference between the modes.  Also the one-off time of
          quantize_mlp(8) (the re-pack) and the largest difference of a probability from the
          fp32 path's at random init.
  ab    : the fp32 default of this tree against a built checkout of the parent commit
          (tools/lr_sched_bench.py ab): `bench.py --gpus 1` from each tree in alternating
          fresh processes; the parent's numbers and every loss_last are written down.

Writes one JSON document to --out and prints it.
python tools/mlp8_bench.py step [--config terabyte] [--steps 200] [--rounds 3]
python tools/mlp8_bench.py ab --parent DIR [--steps 300] [--warmup 50] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from embq_bench import NB, _cycle, _trainer  # noqa: E402
from lr_sched_bench import _stats, _time_ms, ab  # noqa: E402

MODES = {"fp32": dict(), "bf16": dict(precision="bf16"), "int8": dict(mlp_bits=8)}


def _quantize_ms(tr, reps):
    """ms of one quantize_mlp(8) (the re-pack: the buffers exist), median of ``reps``."""
    import torch
    times = []
    for _ in range(reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        evs[0].record()
        tr.quantize_mlp(8)
        evs[1].record()
        torch.cuda.synchronize()
        times.append(evs[0].elapsed_time(evs[1]))
    return sorted(times)[len(times) // 2], times


def step(args):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pool = torch.cuda.graph_pool_handle()
    c = bench.CONFIGS[args.config]
    tr = _trainer(c, dev)
    batches = [tr.synthetic_batch(c["B"], c["L"], seed=100 + i) for i in range(NB)]
    tr.quantize_mlp(8)  # allocates the buffers
    torch.cuda.synchronize()
    graphs = {}
    for name, kw in MODES.items():
        tr.predict(batches[0], **kw)
        torch.cuda.synchronize()
        graphs[name] = [tr.capture_predict(b, pool=pool, **kw) for b in batches]
        for g in graphs[name]:
            g()
    torch.cuda.synchronize()
    bench.preheat_device(dev, 300.0)
    win = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for m in MODES:
            win[m].append(_time_ms(_cycle(graphs[m]), args.steps, args.warmup))
    tr.check_errors()
    res = {"device": torch.cuda.get_device_name(dev), "config": args.config, "batch": c["B"],
           "steps_per_window": args.steps, "rounds": args.rounds,
           "gather_fused": bool(tr._gather_applies(batches[0])),
           "layers": [[L.N, L.K] for L in tr.layers],
           "launches_per_layer": {"fp32": 1, "bf16": 1, "int8": 2},
           "range_from_epilogue": False}
    row = {m: _stats(w) for m, w in win.items()}
    a = row["fp32"]
    for m in ("bf16", "int8"):
        h = row[m]
        row[f"{m}_over_fp32"] = round(h["median"] / a["median"], 4)
        row[f"{m}_minus_fp32_us"] = round((h["median"] - a["median"]) * 1000.0, 2)
        row[f"{m}_outside_spread"] = bool(abs(h["median"] - a["median"])
                                          > max(a["spread"], h["spread"]))
    row["int8_minus_bf16_us"] = round((row["int8"]["median"] - row["bf16"]["median"]) * 1000.0, 2)
    res["ms_per_predict"] = row
    ms, times = _quantize_ms(tr, 5)
    res["quantize_mlp"] = {"ms": round(ms, 3), "all_ms": [round(t, 3) for t in times],
                           "launches": 2 * len(tr.layers)}
    shift = {}
    for m in ("bf16", "int8"):
        worst = 0.0
        for b in batches:
            ref = tr.predict(b).clone()
            worst = max(worst, float((tr.predict(b, **MODES[m]) - ref).abs().max()))
        shift[m] = worst
    res["max_prob_shift_vs_fp32"] = shift
    return res


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("step")
    s.add_argument("--config", default="terabyte")
    s.add_argument("--steps", type=int, default=200)
    s.add_argument("--warmup", type=int, default=30)
    s.add_argument("--rounds", type=int, default=3)
    s.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp8_bench.json"))
    a = sub.add_parser("ab")
    a.add_argument("--parent", required=True, help="a built checkout of the commit to compare")
    a.add_argument("--steps", type=int, default=300)
    a.add_argument("--warmup", type=int, default=50)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp8_default_ab.json"))
    args = ap.parse_args()
    res = {"step": step, "ab": ab}[args.cmd](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
