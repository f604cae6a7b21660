#!/usr/bin/env python3
"""Mixed-precision training timings on one MI355X (bench.py measures the fp32 step and is not
touched):

  * step: DLRMTrainer.capture() of the fp32 step and of the mlp_precision="bf16" step at a
    bench.py config (default terabyte = C3: B = 2048, true rows), two trainers in one
    process, ms per replay over 10 batches in alternating windows (fp32, bf16, fp32, ...,
    --rounds of each): the spread between a mode's own windows is the yardstick for the
    difference between the modes;
  * layers: for every MLP layer below the head, dlrm_linear16_dgrad and dlrm_linear16_wgrad
    (SGD-fused, K + 1 columns, as the step issues them) beside dlrm_gemm_f32 on the same
    problem (the fp32 step's _dgrad / _wgrad problems, each as a launch of its own), --reps
    launches per hipGraph replay, alternating windows again.  The byte bound is the fp32
    traffic of the operands and the output at 8 TB/s.

Writes one JSON document to --out (default profiles/train16_bench.json) and prints it.
python tools/train16_bench.py [--config terabyte] [--steps 200] [--rounds 3] [--skip-step]
[--skip-layers]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_BYTES_PER_US = 8.0e6  # 8 TB/s


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


def _stats(w):
    return dict(windows=[round(v, 4) for v in w], median=round(sorted(w)[len(w) // 2], 4),
                spread=round(max(w) - min(w), 4))


def _trainer(config, dev, precision):
    import bench
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = bench.CONFIGS[config]
    qr = c.get("qr")
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
                        ln_top=[bench.num_int(len(c["rows"]), c["D"])] + c["top"],
                        loss_function=c["loss"], learning_rate=c["lr"], optimizer=c["optimizer"],
                        qr_flag=qr is not None, qr_collisions=qr["collisions"] if qr else 4,
                        qr_operation=qr["operation"] if qr else "mult",
                        qr_threshold=qr["threshold"] if qr else 200, mlp_precision=precision)
    return c, DLRMTrainer(cfg, device=dev, seed=1)


def step_timing(config, steps, warmup, rounds, dev):
    import bench
    modes = ("fp32", "bf16")
    runs = {}
    nb = 10
    pool = torch.cuda.graph_pool_handle()
    for mode in modes:
        c, tr = _trainer(config, dev, mode)
        batches = [tr.synthetic_batch(c["B"], c["L"], seed=100 + i) for i in range(nb)]
        for b in batches[:3]:
            tr.step(b)
        torch.cuda.synchronize()
        graphs = [tr.capture(b, pool=pool) for b in batches]
        for g in graphs:
            g()
        torch.cuda.synchronize()
        # the graphs read the batches' tensors by address: they live as long as the graphs
        runs[mode] = (tr, graphs, batches)
    k = [0]

    def cycle(graphs):
        def run():
            graphs[k[0] % nb]()
            k[0] += 1
        return run

    bench.preheat_device(dev, 300.0)
    windows = {m: [] for m in modes}
    for _ in range(rounds):
        for m in modes:
            windows[m].append(_time_ms(cycle(runs[m][1]), steps, warmup))
    for m in modes:
        runs[m][0].check_errors()
    res = dict(config=config, batch=c["B"], ms_per_step={m: _stats(w) for m, w in windows.items()})
    res["bf16_over_fp32"] = round(res["ms_per_step"]["bf16"]["median"] /
                                  res["ms_per_step"]["fp32"]["median"], 4)
    return res


def _graph_of(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def layer_timing(config, reps, rounds, dev):
    import bench
    from dlrm_hip import ops
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = bench.CONFIGS[config]
    B = c["B"]
    # the MLPs alone (one tiny table): the layers' shapes do not depend on the tables
    ln_top = [bench.num_int(len(c["rows"]), c["D"])] + c["top"]
    cfg = TrainerConfig(m_spa=c["D"], ln_emb=[8] * len(c["rows"]), ln_bot=c["bot"], ln_top=ln_top,
                        loss_function=c["loss"], learning_rate=c["lr"])
    tr = DLRMTrainer(cfg, device=dev, seed=1)
    gen = torch.Generator(device=dev).manual_seed(2)
    out = []
    lr = 1e-30  # the SGD epilogues run, the weights stay put over thousands of launches
    for li, L in enumerate(tr.layers[:-1]):
        name = f"{'bot' if li < tr.n_bot else 'top'} {L.K}->{L.N}"
        g = torch.randn(B, L.Np, generator=gen, device=dev) * 0.01
        inp = torch.rand(B, L.Kp, generator=gen, device=dev) - 0.3
        inp[:, L.K] = 1.0
        inp[:, L.K + 1:] = 0.0
        dx = torch.zeros(B, L.Kp, device=dev)
        ws16 = torch.empty(max(ops.linear16_wgrad_workspace_size(B, L.N, L.K + 1), 4),
                           dtype=torch.uint8, device=dev)
        cand = {}
        if li != 0:  # the bottom MLP's first layer has no data gradient
            pd = [DLRMTrainer._dgrad(L, g, inp, dx)]
            wsd = torch.zeros(max(ops.gemm_group_workspace_size(pd), 4), dtype=torch.uint8,
                              device=dev)
            cand["dgrad"] = (
                lambda pd=pd, wsd=wsd: ops.gemm_group(pd, wsd, dev),
                lambda L=L, g=g, inp=inp, dx=dx: ops.linear16_dgrad(
                    g[:, :L.N], L.W[:, :L.K], inp[:, :L.K], out=dx[:, :L.K]),
                4 * (B * L.N + L.N * L.K + 2 * B * L.K))
        pw = [DLRMTrainer._wgrad(L, g, inp, True, lr)]
        wsw = torch.zeros(max(ops.gemm_group_workspace_size(pw), 4), dtype=torch.uint8, device=dev)
        cand["wgrad"] = (
            lambda pw=pw, wsw=wsw: ops.gemm_group(pw, wsw, dev),
            lambda L=L, g=g, inp=inp, ws16=ws16: ops.linear16_wgrad(
                g[:, :L.N], inp[:, :L.K + 1], L.W[:, :L.K + 1], lr=lr, workspace=ws16),
            4 * (B * L.N + B * (L.K + 1) + 2 * L.N * (L.K + 1)))
        for kind, (f32, b16, nbytes) in cand.items():
            graphs = {"fp32": _graph_of(f32, reps), "bf16": _graph_of(b16, reps)}
            windows = {m: [] for m in graphs}
            for _ in range(rounds):
                for m, gr in graphs.items():
                    windows[m].append(_time_ms(gr.replay, 5, 2) * 1000.0 / reps)
            row = dict(layer=name, kind=kind, M=B, N=L.N, K=L.K,
                       us={m: _stats(w) for m, w in windows.items()},
                       byte_bound_us=round(nbytes / HBM_BYTES_PER_US, 2))
            f, h = row["us"]["fp32"], row["us"]["bf16"]
            row["bf16_over_fp32"] = round(h["median"] / f["median"], 3)
            row["faster"] = bool(f["median"] - h["median"] > max(f["spread"], h["spread"]))
            out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="terabyte")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-layers", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train16_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(dev)}
    if not args.skip_layers:
        res["layers"] = layer_timing(args.config, args.reps, args.rounds, dev)
        torch.cuda.empty_cache()
    if not args.skip_step:
        res["step"] = step_timing(args.config, args.steps, args.warmup, args.rounds, dev)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
