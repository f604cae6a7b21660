#!/usr/bin/env python3
"""fp16 embedding tables (TrainerConfig.emb_precision = "fp16") timed on one MI355X (bench.py
measures the fp32 default and is not touched):

  step  : two trainers in one process at a bench.py config (default terabyte = C3: B = 2048,
          true rows; 27.7 GB of fp32 tables + 13.9 GB of fp16 tables), DLRMTrainer.capture()
          of the training step and capture_predict() of the forward-only pass, ms per replay
          over 10 batches in alternating windows (fp32, fp16, fp32, ..., --rounds of each)
          after a clock preheat: the spread between a mode's own windows is the yardstick for
          the difference between the modes.
          --rounding: the same protocol over two fp16-table trainers instead, the update
          stored rounded to "nearest" (the mode as it was) against "stochastic"
          (TrainerConfig.emb_rounding: the hash and one more one-thread launch per step);
          training step only, written to profiles/sr16_bench.json.
  trace : --steps replays of the fp16-table step and nothing else, to run under
          `rocprofv3 --kernel-trace` (tools/step_timeline.py prints one step of the trace).
  ab    : the fp32 default of this tree against a built checkout of the parent commit
          (tools/lr_sched_bench.py ab): `bench.py --gpus 1` from each tree in alternating
          fresh processes; the parent's numbers and every loss_last are written down.

Writes one JSON document to --out and prints it.
python tools/emb16_bench.py step [--config terabyte] [--steps 200] [--rounds 3] [--rounding]
python tools/emb16_bench.py trace [--config terabyte] [--steps 30]
python tools/emb16_bench.py ab --parent DIR [--steps 300] [--warmup 50] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from lr_sched_bench import _stats, _time_ms, ab  # noqa: E402

MODES = ("fp32", "fp16")
ROUNDINGS = ("nearest", "stochastic")  # step --rounding: both on fp16 tables
NB = 10  # batches a window cycles through


def _trainer(config, dev, mode):
    kw = dict(emb_precision=mode)
    if mode in ROUNDINGS:
        kw = dict(emb_precision="fp16", emb_rounding=mode)
    import bench
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = bench.CONFIGS[config]
    if c.get("qr") is not None or c["optimizer"] != "sgd":
        raise SystemExit(f"config {config}: fp16 tables run plain tables with SGD only")
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[bench.num_int(len(c["rows"]), c["D"])] + c["top"],
                        loss_function=c["loss"], learning_rate=c["lr"], optimizer=c["optimizer"],
                        **kw)
    return c, DLRMTrainer(cfg, device=dev, seed=1)


def _captured(config, dev, mode, pool, predict):
    """(trainer, train graphs, predict graphs, batches): the graphs read the batches' tensors
    by address, so the batches live as long as the graphs."""
    import torch
    c, tr = _trainer(config, dev, mode)
    batches = [tr.synthetic_batch(c["B"], c["L"], seed=100 + i) for i in range(NB)]
    for b in batches[:3]:
        tr.step(b)
    torch.cuda.synchronize()
    train = [tr.capture(b, pool=pool) for b in batches]
    pred = []
    if predict:
        tr.predict(batches[0])
        torch.cuda.synchronize()
        pred = [tr.capture_predict(b, pool=pool) for b in batches]
    for g in train + pred:
        g()
    torch.cuda.synchronize()
    return c, tr, train, pred, batches


def _cycle(graphs):
    k = [0]

    def run():
        graphs[k[0] % len(graphs)]()
        k[0] += 1
    return run


def step(args):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pool = torch.cuda.graph_pool_handle()
    MODES = ROUNDINGS if args.rounding else globals()["MODES"]
    base, other = MODES
    kinds = (("train", 2),) if args.rounding else (("train", 2), ("predict", 3))
    runs = {m: _captured(args.config, dev, m, pool, not args.rounding) for m in MODES}
    c = runs[base][0]
    bench.preheat_device(dev, 300.0)
    win = {kind: {m: [] for m in MODES} for kind, _ in kinds}
    for _ in range(args.rounds):
        for kind, at in kinds:
            for m in MODES:
                win[kind][m].append(_time_ms(_cycle(runs[m][at]), args.steps, args.warmup))
    for m in MODES:
        runs[m][1].check_errors()
    res = {"device": torch.cuda.get_device_name(dev), "config": args.config, "batch": c["B"],
           "steps_per_window": args.steps, "rounds": args.rounds,
           "table_bytes": {m: runs[m][1].weights.numel() * runs[m][1].weights.element_size()
                           for m in MODES},
           "gather_fused": {m: bool(runs[m][1].gather_fused) for m in MODES}}
    for kind in win:
        row = {m: _stats(w) for m, w in win[kind].items()}
        a, h = row[base], row[other]
        row[f"{other}_over_{base}"] = round(h["median"] / a["median"], 4)
        row[f"{other}_minus_{base}_us"] = round((h["median"] - a["median"]) * 1000.0, 2)
        row["outside_spread"] = bool(abs(h["median"] - a["median"]) > max(a["spread"], h["spread"]))
        res["ms_per_" + kind] = row
    if args.rounding:
        res["rounding_state"] = list(runs["stochastic"][1].rounding_state())
    return res


def trace(args):
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _c, tr, train, _pred, _batches = _captured(args.config, dev, "fp16", None, False)
    run = _cycle(train)
    for _ in range(args.steps):
        run()
    torch.cuda.synchronize()
    tr.check_errors()
    return {"config": args.config, "replays": args.steps, "gather_fused": bool(tr.gather_fused)}


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("step")
    s.add_argument("--config", default="terabyte")
    s.add_argument("--steps", type=int, default=200)
    s.add_argument("--warmup", type=int, default=30)
    s.add_argument("--rounds", type=int, default=3)
    s.add_argument("--rounding", action="store_true",
                   help="fp16 tables: emb_rounding nearest against stochastic")
    s.add_argument("--out", default=None)
    t = sub.add_parser("trace")
    t.add_argument("--config", default="terabyte")
    t.add_argument("--steps", type=int, default=30)
    t.add_argument("--out", default=None)
    a = sub.add_parser("ab")
    a.add_argument("--parent", required=True, help="a built checkout of the commit to compare")
    a.add_argument("--steps", type=int, default=300)
    a.add_argument("--warmup", type=int, default=50)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--out", default=os.path.join(ROOT, "profiles", "emb16_default_ab.json"))
    args = ap.parse_args()
    if args.cmd == "step" and args.out is None:
        args.out = os.path.join(ROOT, "profiles",
                                "sr16_bench.json" if args.rounding else "emb16_bench.json")
    res = {"step": step, "trace": trace, "ab": ab}[args.cmd](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
