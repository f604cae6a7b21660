#!/usr/bin/env python3
"""Evaluation-path timings on one MI355X (bench.py measures training and is not touched):

  * predict: DLRMTrainer.capture_predict at a bench.py config (default terabyte = C3:
    B = 2048, true rows) with an EvalState attached, ms per replay over 10 batches, beside
    the training step's capture() on the same process (bench.py's own figure on the parent
    commit is the yardstick; this one is for the ratio); with --precision fp32,bf16,fp16 one
    graph set per precision, timed in alternating windows (fp32, bf16, fp16, fp32, ...,
    --rounds of them) so the spread between the repeated fp32 windows - the unchanged
    path - is the yardstick for the 16-bit ones;
  * metrics: dlrm_eval_metrics (sort + tie-group pass) on n random keys beside torch.sort of
    the same keys as int32.

Prints one JSON line.  python tools/eval_bench.py [--config terabyte] [--steps 300]
[--log2n 24,26] [--skip-predict] [--skip-metrics] [--precision fp32,bf16,fp16] [--rounds 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _time_ms(fn, steps, warmup):
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


def predict_timing(config, steps, warmup, dev, precisions=("fp32",), rounds=1):
    import bench
    from dlrm_hip import metrics
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = bench.CONFIGS[config]
    B, T = c["B"], len(c["rows"])
    qr = c.get("qr")
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[bench.num_int(T, c["D"])] + c["top"], loss_function=c["loss"],
                        learning_rate=c["lr"], optimizer=c["optimizer"], qr_flag=qr is not None,
                        qr_collisions=qr["collisions"] if qr else 4,
                        qr_operation=qr["operation"] if qr else "mult",
                        qr_threshold=qr["threshold"] if qr else 200)
    tr = DLRMTrainer(cfg, device=dev, seed=1)
    nb = 10
    batches = [tr.synthetic_batch(B, c["L"], seed=100 + i) for i in range(nb)]
    for b in batches[:3]:
        tr.step(b)
        for p in precisions:
            tr.predict(b, precision=p)
    torch.cuda.synchronize()
    st = metrics.EvalState((steps + warmup + 2 * nb) * B, dev)
    pool = torch.cuda.graph_pool_handle()
    train = [tr.capture(b, pool=pool) for b in batches]
    preds = {p: [tr.capture_predict(b, metrics=st, pool=pool, precision=p) for b in batches]
             for p in precisions}
    torch.cuda.synchronize()
    for g in train + [g for p in precisions for g in preds[p]]:  # first (upload) replays
        g()
    torch.cuda.synchronize()
    k = [0]

    def cycle(graphs):
        def run():
            graphs[k[0] % nb]()
            k[0] += 1
        return run

    bench.preheat_device(dev, 300.0)
    train_ms = _time_ms(cycle(train), steps, warmup)
    windows = {p: [] for p in precisions}
    logged = 0
    for _ in range(rounds):
        for p in precisions:
            st.reset()
            windows[p].append(round(_time_ms(cycle(preds[p]), steps, warmup), 4))
            logged = st.count
    tr.check_errors()
    pred_ms = windows[precisions[0]][0]
    res = dict(config=config, batch=B, train_ms_per_step=round(train_ms, 4),
               predict_ms_per_step=pred_ms,
               predict_over_train=round(pred_ms / train_ms, 3), keys_logged=logged,
               gather_fused=bool(tr._gather_applies(batches[0])))
    if len(precisions) > 1 or rounds > 1:
        res["predict_windows_ms"] = windows
        res["predict_median_ms"] = {p: sorted(w)[len(w) // 2] for p, w in windows.items()}
        res["predict_spread_ms"] = {p: round(max(w) - min(w), 4) for p, w in windows.items()}
    return res


def metrics_timing(log2n, dev, reps=5):
    from dlrm_hip import _lib, ops
    n = 1 << log2n
    g = torch.Generator(device=dev)
    g.manual_seed(log2n)
    prob = torch.rand(n, generator=g, device=dev)
    lab = (torch.rand(n, generator=g, device=dev) < 0.3).to(torch.int32)
    keys0 = (prob.view(torch.int32) << 1) | lab
    del prob, lab
    ws = torch.empty(_lib.query("dlrm_eval_metrics_workspace_size", n), dtype=torch.uint8,
                     device=dev)
    out = torch.empty(5, dtype=torch.int64, device=dev)
    keys = torch.empty_like(keys0)

    def ours():
        keys.copy_(keys0)
        ops.eval_metrics(keys, n, workspace=ws, out=out)

    def copy_only():
        keys.copy_(keys0)

    def ref():
        torch.sort(keys0)

    t_copy = _time_ms(copy_only, reps, 2)
    t_ours = _time_ms(ours, reps, 2) - t_copy
    ok = bool((keys[1:] >= keys[:-1]).all().item())  # (keys < 2^31: int32 order = key order)
    t_ref = _time_ms(ref, reps, 2)
    return dict(log2n=log2n, eval_metrics_ms=round(t_ours, 3), torch_sort_ms=round(t_ref, 3),
                ratio=round(t_ours / t_ref, 3), sorted=ok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="terabyte")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--log2n", default="24,26")
    ap.add_argument("--skip-predict", action="store_true")
    ap.add_argument("--skip-metrics", action="store_true")
    ap.add_argument("--precision", default="fp32",
                    help="comma list of fp32,bf16,fp16: one predict graph set each, timed in "
                         "alternating windows")
    ap.add_argument("--rounds", type=int, default=0,
                    help="windows per precision (default: 3 with several precisions, else 1)")
    args = ap.parse_args()
    precisions = tuple(p for p in args.precision.split(",") if p)
    rounds = args.rounds or (3 if len(precisions) > 1 else 1)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev)}
    if not args.skip_metrics:
        res["metrics"] = [metrics_timing(int(v), dev) for v in args.log2n.split(",") if v]
        torch.cuda.empty_cache()
    if not args.skip_predict:
        res["predict"] = predict_timing(args.config, args.steps, args.warmup, dev, precisions,
                                        rounds)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
