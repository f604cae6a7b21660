#!/usr/bin/env python3
"""Element-wise Adagrad (TrainerConfig.optimizer = "adagrad") timed on one MI355X against
row-wise Adagrad (bench.py measures the SGD default and is not touched):

  step  : two trainers in one process at a bench.py config (default terabyte = C3: B = 2048,
          true rows; 2 x 27.7 GB of fp32 tables + 27.7 GB of element-wise state, about 83 GB),
          optimizer "rwsadagrad" and "adagrad" at the same rate, DLRMTrainer.capture() of the
          training step, ms per replay over 10 batches in alternating windows (rwsadagrad,
          adagrad, rwsadagrad, ..., --rounds of each) after a clock preheat: the spread between
          a mode's own windows is the yardstick for the difference between the modes.  The
          row-wise update rides on the bottom-MLP backward's GEMM launches (launch roles); the
          element-wise one runs as launches of its own and reads and writes a second row per
          unique row.
  trace : --steps replays of the adagrad step and nothing else, to run under
          `rocprofv3 --kernel-trace` (tools/step_timeline.py prints one step of the trace).
  ab    : the SGD default of this tree against a built checkout of the parent commit
          (tools/lr_sched_bench.py ab): `bench.py --gpus 1` from each tree in alternating
          fresh processes; the parent's numbers and every loss_last are written down.

Writes one JSON document to --out and prints it.
python tools/adagrad_bench.py step [--config terabyte] [--steps 200] [--rounds 3]
python tools/adagrad_bench.py trace [--config terabyte] [--steps 30]
python tools/adagrad_bench.py ab --parent DIR [--steps 300] [--warmup 50] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from lr_sched_bench import _stats, _time_ms, ab  # noqa: E402

MODES = ("rwsadagrad", "adagrad")
NB = 10  # batches a window cycles through
LR = 0.01  # both modes (the config's SGD rate is not an Adagrad rate)


def _trainer(config, dev, mode):
    import bench
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = bench.CONFIGS[config]
    if c.get("qr") is not None:
        raise SystemExit(f"config {config}: this bench runs plain tables")
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[bench.num_int(len(c["rows"]), c["D"])] + c["top"],
                        loss_function=c["loss"], learning_rate=LR, optimizer=mode)
    return c, DLRMTrainer(cfg, device=dev, seed=1)


def _captured(config, dev, mode, pool):
    """(config, trainer, train graphs, batches): the graphs read the batches' tensors by
    address, so the batches live as long as the graphs."""
    import torch
    c, tr = _trainer(config, dev, mode)
    batches = [tr.synthetic_batch(c["B"], c["L"], seed=100 + i) for i in range(NB)]
    for b in batches[:3]:
        tr.step(b)
    torch.cuda.synchronize()
    train = [tr.capture(b, pool=pool) for b in batches]
    for g in train:
        g()
    torch.cuda.synchronize()
    return c, tr, train, batches


def _cycle(graphs):
    k = [0]

    def run():
        graphs[k[0] % len(graphs)]()
        k[0] += 1
    return run


def _state_bytes(tr):
    return sum(t.numel() * t.element_size() for t in (tr.momentum, tr.emb_sum) if t is not None)


def step(args):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pool = torch.cuda.graph_pool_handle()
    base, other = MODES
    runs = {m: _captured(args.config, dev, m, pool) for m in MODES}
    c = runs[base][0]
    bench.preheat_device(dev, 300.0)
    win = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for m in MODES:
            win[m].append(_time_ms(_cycle(runs[m][2]), args.steps, args.warmup))
    for m in MODES:
        runs[m][1].check_errors()
    row = {m: _stats(w) for m, w in win.items()}
    a, h = row[base], row[other]
    row[f"{other}_over_{base}"] = round(h["median"] / a["median"], 4)
    row[f"{other}_minus_{base}_us"] = round((h["median"] - a["median"]) * 1000.0, 2)
    row["outside_spread"] = bool(abs(h["median"] - a["median"]) > max(a["spread"], h["spread"]))
    return {"device": torch.cuda.get_device_name(dev), "config": args.config, "batch": c["B"],
            "learning_rate": LR, "steps_per_window": args.steps, "rounds": args.rounds,
            "table_bytes": {m: runs[m][1].weights.numel() * 4 for m in MODES},
            "embedding_state_bytes": {m: _state_bytes(runs[m][1]) for m in MODES},
            "gather_fused": {m: bool(runs[m][1].gather_fused) for m in MODES},
            "ms_per_train": row}


def trace(args):
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _c, tr, train, _batches = _captured(args.config, dev, "adagrad", None)
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
    s.add_argument("--out", default=os.path.join(ROOT, "profiles", "adagrad_bench.json"))
    t = sub.add_parser("trace")
    t.add_argument("--config", default="terabyte")
    t.add_argument("--steps", type=int, default=30)
    t.add_argument("--out", default=None)
    a = sub.add_parser("ab")
    a.add_argument("--parent", required=True, help="a built checkout of the commit to compare")
    a.add_argument("--steps", type=int, default=300)
    a.add_argument("--warmup", type=int, default=50)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--out", default=os.path.join(ROOT, "profiles", "adagrad_default_ab.json"))
    args = ap.parse_args()
    res = {"step": step, "trace": trace, "ab": ab}[args.cmd](args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
