#!/usr/bin/env python3
"""What the device-resident learning rates cost on one MI355X (bench.py measures the default
step and is not touched):

  sched : DLRMTrainer.capture() of the default step (host rates) and of the scheduled step
          (TrainerConfig.lr_num_warmup_steps / lr_decay_start_step / lr_num_decay_steps, the
          MLPerf Terabyte policy by default) at a bench.py config (default terabyte = C3:
          B = 2048, true rows), two trainers in one process, ms per replay over 10 batches
          in alternating windows (host, device, host, ..., --rounds of each): the spread
          between a mode's own windows is the yardstick for the difference between the modes.
          Also the tick alone: --reps dlrm_lr_schedule_tick launches per hipGraph replay,
          us per (dependent, one-thread) launch.
  ab    : the default path of this tree against a built checkout of another commit
          (--parent DIR): `bench.py --gpus 1` from each tree as a fresh child process, in
          alternating runs (parent, this, parent, ...).  The spread of the parent's own runs
          is the yardstick; loss_last of every run is recorded (it must not move).

Writes one JSON document to --out and prints it.
python tools/lr_sched_bench.py sched [--config terabyte] [--steps 200] [--rounds 4]
python tools/lr_sched_bench.py ab --parent DIR [--steps 300] [--warmup 50] [--rounds 3]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _paths():
    for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)


def _stats(w):
    return dict(windows=[round(v, 4) for v in w], median=round(sorted(w)[len(w) // 2], 4),
                spread=round(max(w) - min(w), 4))


def _time_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    evs[0].record()
    for _ in range(steps):
        fn()
    evs[1].record()
    torch.cuda.synchronize()
    return evs[0].elapsed_time(evs[1]) / steps


def _trainer(config, dev, policy):
    import bench
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = bench.CONFIGS[config]
    qr = c.get("qr")
    kw = {}
    if policy is not None:
        kw = dict(lr_num_warmup_steps=policy[0], lr_decay_start_step=policy[1],
                  lr_num_decay_steps=policy[2])
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[bench.num_int(len(c["rows"]), c["D"])] + c["top"],
                        loss_function=c["loss"], learning_rate=c["lr"], optimizer=c["optimizer"],
                        qr_flag=qr is not None, qr_collisions=qr["collisions"] if qr else 4,
                        qr_operation=qr["operation"] if qr else "mult",
                        qr_threshold=qr["threshold"] if qr else 200, **kw)
    return c, DLRMTrainer(cfg, device=dev, seed=1)


def sched(args):
    _paths()
    import torch
    import bench
    from dlrm_hip import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    policy = tuple(int(v) for v in args.policy.split(","))
    modes = {"host": None, "device": policy}
    runs = {}
    nb = 10
    pool = torch.cuda.graph_pool_handle()
    for mode, pol in modes.items():
        c, tr = _trainer(args.config, dev, pol)
        batches = [tr.synthetic_batch(c["B"], c["L"], seed=100 + i) for i in range(nb)]
        for b in batches[:3]:
            tr.step(b)
        torch.cuda.synchronize()
        graphs = [tr.capture(b, pool=pool) for b in batches]
        for g in graphs:
            g()
        torch.cuda.synchronize()
        runs[mode] = (tr, graphs, batches)  # the graphs read the batches by address
    k = [0]

    def cycle(graphs):
        def run():
            graphs[k[0] % nb]()
            k[0] += 1
        return run

    bench.preheat_device(dev, 300.0)
    windows = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            windows[m].append(_time_ms(cycle(runs[m][1]), args.steps, args.warmup))
    for m in modes:
        runs[m][0].check_errors()
    step = dict(config=args.config, batch=c["B"], policy=list(policy),
                ms_per_step={m: _stats(w) for m, w in windows.items()},
                lr_step_after=runs["device"][0].lr_step,
                current_lr=runs["device"][0].current_lr())
    h, d = step["ms_per_step"]["host"], step["ms_per_step"]["device"]
    step["device_minus_host_us"] = round((d["median"] - h["median"]) * 1000.0, 2)
    step["inside_spread"] = bool(abs(d["median"] - h["median"]) <= max(h["spread"], d["spread"]))
    # the tick alone: dependent one-thread launches inside one graph
    st = ops.lr_state([0.1, 0.1, 0.1], [1.0, 1.0, 0.125], *policy, device=dev)
    ops.lr_schedule_tick(st)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(args.reps):
            ops.lr_schedule_tick(st)
    g.replay()
    torch.cuda.synchronize()
    tick = [_time_ms(g.replay, 5, 2) * 1000.0 / args.reps for _ in range(args.rounds)]
    return {"device": torch.cuda.get_device_name(dev), "step": step,
            "tick_us_per_launch": _stats(tick), "tick_launches_per_graph": args.reps}


def _bench_child(tree, steps, warmup):
    """One `bench.py --gpus 1` of a tree in a fresh process; its JSON result line."""
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1",
                          "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(f"bench.py in {tree} failed ({out.returncode}): {out.stderr[-2000:]}")
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{") and '"metric"' in line:
            return json.loads(line)
    raise RuntimeError(f"bench.py in {tree} printed no result line")


def ab(args):
    trees = {"parent": os.path.abspath(args.parent), "this": ROOT}
    runs = {k: [] for k in trees}
    for _ in range(args.rounds):
        for name, tree in trees.items():
            r = _bench_child(tree, args.steps, args.warmup)
            runs[name].append(dict(ms_per_step=r["ms_per_step"], value=r["value"],
                                   loss_last=r["loss_last"],
                                   p10_p50_p90=r["ms_per_step_p10_p50_p90"]))
    res = {"steps": args.steps, "warmup": args.warmup, "runs": runs,
           "ms_per_step": {k: _stats([x["ms_per_step"] for x in v]) for k, v in runs.items()}}
    p, t = res["ms_per_step"]["parent"], res["ms_per_step"]["this"]
    res["this_minus_parent_us"] = round((t["median"] - p["median"]) * 1000.0, 2)
    res["parent_spread_us"] = round(p["spread"] * 1000.0, 2)
    res["inside_parent_spread"] = bool(abs(t["median"] - p["median"]) <= p["spread"])
    res["loss_last_equal"] = len({x["loss_last"] for v in runs.values() for x in v}) == 1
    return res


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("sched")
    s.add_argument("--config", default="terabyte")
    s.add_argument("--policy", default="2750,49315,27772", help="W,S,D (MLPerf Terabyte)")
    s.add_argument("--steps", type=int, default=200)
    s.add_argument("--warmup", type=int, default=30)
    s.add_argument("--rounds", type=int, default=4)
    s.add_argument("--reps", type=int, default=200)
    s.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_sched_cost.json"))
    a = sub.add_parser("ab")
    a.add_argument("--parent", required=True, help="a built checkout of the commit to compare")
    a.add_argument("--steps", type=int, default=300)
    a.add_argument("--warmup", type=int, default=50)
    a.add_argument("--rounds", type=int, default=3)
    a.add_argument("--out", default=os.path.join(ROOT, "profiles", "lr_sched_default_ab.json"))
    args = ap.parse_args()
    res = sched(args) if args.cmd == "sched" else ab(args)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
