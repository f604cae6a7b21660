#!/usr/bin/env python3
"""int8 / int4 embedding tables for inference (DLRMTrainer.quantize_embedding,
predict(emb_bits=)) timed on one MI355X (bench.py measures the fp32 default and
is not touched):

  step  : one trainer at a bench.py config (default terabyte = C3: B = 2048, true rows; 27.7 GB
          of fp32 tables + 7.4 GB of Q8 rows + 3.7 GB of Q4 rows), capture_predict() of the
          forward-only pass over 10 batches for the fp32 tables, emb_bits=8 and emb_bits=4,
          ms per replay in alternating windows (fp32, q8, q4, fp32, ..., --rounds of each)
          after a clock preheat: the spread between a mode's own windows is the yardstick for
          the difference between the modes.  Also the one-off time of quantize_embedding
          against its byte floor (bytes read + written over the HBM peak rate), and the
          largest difference of a probability from the fp32 tables' for each width, at the
          config (random init) and on two small models.
  ab    : the fp32 default of this tree against a built checkout of the parent commit
          (tools/lr_sched_bench.py ab): `bench.py --gpus 1` from each tree in alternating
          fresh processes; the parent's numbers and every loss_last are written down.

Writes one JSON document to --out and prints it.
python tools/embq_bench.py step [--config terabyte] [--steps 200] [--rounds 3]
python tools/embq_bench.py ab --parent DIR [--steps 300] [--warmup 50] [--rounds 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from lr_sched_bench import _stats, _time_ms, ab  # noqa: E402

MODES = {"fp32": 32, "q8": 8, "q4": 4}
NB = 10  # batches a window cycles through
SMALL = {  # the models of tests/test_gpu_rowsq.py
    "d16": dict(D=16, rows=[30, 200, 1, 64, 17], bot=[13, 32, 16], top=[32, 1], B=5),
    "d64": dict(D=64, rows=[200, 30, 150], bot=[13, 64, 32, 64], top=[48, 1], B=70),
}


def _trainer(c, dev):
    import bench
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[bench.num_int(len(c["rows"]), c["D"])] + c["top"],
                        loss_function=c.get("loss", "bce"), learning_rate=c.get("lr", 0.1),
                        optimizer=c.get("optimizer", "sgd"))
    return DLRMTrainer(cfg, device=dev, seed=1)


def _cycle(graphs):
    k = [0]

    def run():
        graphs[k[0] % len(graphs)]()
        k[0] += 1
    return run


def _score_shift(tr, batches):
    """Largest |prob(emb_bits) - prob(fp32 tables)| over the batches, per width."""
    out = {}
    for name, bits in MODES.items():
        if bits == 32:
            continue
        worst = 0.0
        for b in batches:
            ref = tr.predict(b).clone()
            worst = max(worst, float((tr.predict(b, emb_bits=bits) - ref).abs().max()))
        out[name] = worst
    return out


def _quantize_ms(tr, bits, reps):
    """ms of one quantize_embedding (the re-pack: the buffer exists), median of ``reps``."""
    import torch
    times = []
    for _ in range(reps):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        evs[0].record()
        tr.quantize_embedding(bits)
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
    if c.get("qr") is not None:
        raise SystemExit(f"config {args.config}: quantized tables run plain tables only")
    tr = _trainer(c, dev)
    batches = [tr.synthetic_batch(c["B"], c["L"], seed=100 + i) for i in range(NB)]
    for bits in (8, 4):
        tr.quantize_embedding(bits)  # allocates the buffer
    torch.cuda.synchronize()
    graphs = {}
    for name, bits in MODES.items():
        tr.predict(batches[0], emb_bits=bits)
        torch.cuda.synchronize()
        graphs[name] = [tr.capture_predict(b, pool=pool, emb_bits=bits) for b in batches]
        for g in graphs[name]:
            g()
    torch.cuda.synchronize()
    bench.preheat_device(dev, 300.0)
    win = {m: [] for m in MODES}
    for _ in range(args.rounds):
        for m in MODES:
            win[m].append(_time_ms(_cycle(graphs[m]), args.steps, args.warmup))
    tr.check_errors()
    wbytes = tr.weights.numel() * tr.weights.element_size()
    res = {"device": torch.cuda.get_device_name(dev), "config": args.config, "batch": c["B"],
           "steps_per_window": args.steps, "rounds": args.rounds,
           "gather_fused": bool(tr._gather_applies(batches[0])),
           "table_bytes": {"fp32": wbytes,
                           "q8": tr.quantized_rows(8).numel(), "q4": tr.quantized_rows(4).numel()}}
    row = {m: _stats(w) for m, w in win.items()}
    a = row["fp32"]
    for m in ("q8", "q4"):
        h = row[m]
        row[f"{m}_over_fp32"] = round(h["median"] / a["median"], 4)
        row[f"{m}_minus_fp32_us"] = round((h["median"] - a["median"]) * 1000.0, 2)
        row[f"{m}_outside_spread"] = bool(abs(h["median"] - a["median"])
                                          > max(a["spread"], h["spread"]))
    res["ms_per_predict"] = row
    quant = {}
    for m in ("q8", "q4"):
        ms, times = _quantize_ms(tr, MODES[m], 5)
        moved = wbytes + res["table_bytes"][m]
        floor_ms = moved / (bench.HBM_PEAK_GBS * 1e9) * 1e3
        quant[m] = {"ms": round(ms, 3), "all_ms": [round(t, 3) for t in times],
                    "bytes_moved": moved, "floor_ms_at_hbm_peak": round(floor_ms, 3),
                    "achieved_gbs": round(moved / (ms * 1e-3) / 1e9, 1),
                    "frac_of_hbm_peak": round(floor_ms / ms, 4)}
    res["quantize_embedding"] = quant
    res["max_prob_shift_vs_fp32_tables"] = {args.config: _score_shift(tr, batches)}
    del graphs, tr
    for name, m in SMALL.items():
        small = _trainer(m, dev)
        for bits in (8, 4):
            small.quantize_embedding(bits)
        sb = [small.synthetic_batch(m["B"], 1, seed=s) for s in (21, 22)]
        res["max_prob_shift_vs_fp32_tables"][name] = _score_shift(small, sb)
    return res


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("step")
    s.add_argument("--config", default="terabyte")
    s.add_argument("--steps", type=int, default=200)
    s.add_argument("--warmup", type=int, default=30)
    s.add_argument("--rounds", type=int, default=3)
    s.add_argument("--out", default=os.path.join(ROOT, "profiles", "embq_bench.json"))
    s.add_argument("--scores-out", default=os.path.join(ROOT, "profiles", "embq_scores.json"))
    a = sub.add_parser("ab")
    a.add_argument("--parent", required=True, help="a built checkout of the commit to compare")
    a.add_argument("--steps", type=int, default=300)
    a.add_argument("--warmup", type=int, default=50)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--out", default=os.path.join(ROOT, "profiles", "embq_default_ab.json"))
    args = ap.parse_args()
    res = {"step": step, "ab": ab}[args.cmd](args)
    if args.cmd == "step" and args.scores_out:  # the score shifts again, as a file of their own
        with open(args.scores_out, "w") as f:
            f.write(json.dumps({"device": res["device"], "what": "max |prob(emb_bits) - "
                                "prob(fp32 tables)|, random init, measured not asserted",
                                "models": res["max_prob_shift_vs_fp32_tables"]}, indent=1) + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
