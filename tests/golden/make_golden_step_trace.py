"""Generate tests/golden/step_trace.json: what DLRMTrainer's step launches, and the bits it
leaves, case by case (tests/test_gpu_step_trace.py replays the cases and demands equality).

It uses the trainer's public API plus a recorder put around dlrm_hip._lib.call, the one door
every launch of ops.py goes through, so it runs unchanged on any commit whose trainer has that
API: the committed file was written on an MI355X from the commit BEFORE the three segment
builders (fp32 step, bf16 step, predict) became one, twice, with identical output.

Per case (CASES below; a training step, or a forward-only predict):
  kinds           the kinds of segments() / predict_segments()
  trace           the _lib.call entries of the SECOND eager step, one list per segment (the
                  first list: calls made while the segment list was built - none).  An entry is
                  [entry point, args...]: ints, floats, bools and None as they are; a pointer
                  into device memory or the stream handle as "p<k>", k its order of first
                  appearance in this trace (aliasing and main-versus-side stream, not
                  addresses); anything else (byref, host structs, cast arrays) as "*".  A
                  profile= hook adds ["prof", group name] entries.
  capture_trace   the same for one capture() / capture_predict() of the batch, flat: "same"
                  when it equals the eager trace (always, but for the profile= case, whose
                  capture has no hook)
  capture_mode, graphs_per_step (training), replays (graphs one replay launched)
  sha256          after the second eager step plus one replay, of the raw bytes of prob, loss,
                  weights, params and, where they exist, momentum, adagrad_sum, grads;
                  predict: of the returned prob (and the EvalState's log and counters)

Usage:  python tests/golden/make_golden_step_trace.py [--out FILE] [--only NAME ...]
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "dlrm-yx_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

DEV = "cuda:0"
RATES = {"sgd": (0.1, 0.05), "rwsadagrad": (1e-3, 2e-3)}  # (dense, embedding) rates
# bf16: the options without an effect in that mode, each off its default
NO_EFFECT = dict(group_wgrad=False, full_last_wgrad=True, bot_sched="partial", tbe_role=False,
                 tbe_role_at=(1, 2), head_role=False, fuse_bottom=False,
                 dist_bottom_in_lookup=False, overlaps={"fwd", "bot"})
NO_EFFECT_CASE, NO_EFFECT_BASE = "one_c2_sgd_noeffect-bf16", "one_c2_sgd-bf16"


def shapes():
    import oracle as O
    return {  # the small shapes of test_gpu_trainer / test_gpu_lr_trainer
        "c2_small": dict(D=16, rows=[min(r, 5000) for r in O.KAGGLE_ROWS],
                         bot=[13, 512, 256, 64, 16], top=[512, 256, 1], B=128),
        "c3_small": dict(D=128, rows=[min(r, 2000) for r in O.TERABYTE_ROWS],
                         bot=[13, 512, 256, 128], top=[1024, 1024, 512, 256, 1], B=256),
    }


def _cases():
    out = {}

    def add(name, precisions=("fp32", "bf16"), **kw):
        for p in precisions:
            case = dict(shape="c2_small", optimizer="sgd", world="one", L=1, cfg={}, attrs={},
                        comm=None, profile=False, mode="train", metrics=False, precision=p)
            case.update(kw)
            out[f"{name}-{p}"] = case

    fp32 = ("fp32",)
    # 1. one GPU
    add("one_c2_sgd")
    add("one_c3_sgd", shape="c3_small")
    add("one_c2_rws", optimizer="rwsadagrad")
    add("one_c2_devlr", cfg=dict(device_lr=True))
    # 2. one GPU, batch kinds
    add("one_c2_L2", L=2)
    for es in (True, 2, False):  # 5120 lookups per table: past the per-table sort cap
        add(f"one_c2_L40_es{es}", L=40, attrs=dict(early_sort=es))
    add("one_c2_qr", cfg=dict(qr_flag=True))
    add("one_c2_nopresort", attrs=dict(tbe_presort=False))
    add("one_c2_nogather", attrs=dict(fuse_gather=False))
    add("one_c2_featpad", attrs=dict(feature_pad=True))
    add("one_c2_profile", profile=True)
    # 3. one GPU, the fp32-only knobs
    for name, attrs in [("norole", dict(tbe_role=False)), ("noheadrole", dict(head_role=False)),
                        ("roleat12", dict(tbe_role_at=(1, 2))), ("full", dict(bot_sched="full")),
                        ("partial", dict(bot_sched="partial")),
                        ("nogroup", dict(group_wgrad=False)),
                        ("fulllast", dict(full_last_wgrad=True)),
                        ("overlaps", dict(overlaps={"fwd", "bot"})),
                        ("nofuse", dict(fuse_bottom=False)), ("parts1", dict(bottom_parts=1))]:
        add("one_c3_" + name, fp32, shape="c3_small", attrs=attrs)
    # 4. rank 2 of 8
    add("w8_c3_sgd", shape="c3_small", world="w8", comm="segments")
    add("w8_c3_rws", shape="c3_small", world="w8", comm="segments", optimizer="rwsadagrad")
    add("w8_c2_whole", world="w8", comm="whole")
    add("w8_c2_eager", world="w8", comm="eager")
    add("w8_c3_nolookupchain", fp32, shape="c3_small", world="w8", comm="segments",
        attrs=dict(dist_bottom_in_lookup=False))
    add("w8_c2_notable", world="w8", comm="segments",
        cfg=dict(allocation=[(0, 1, 3, 4, 5, 6, 7)[t % 7] for t in range(26)]))
    # 5. bf16: the options without an effect there
    add("one_c2_sgd_noeffect", ("bf16",), attrs=NO_EFFECT)
    # 6. predict
    every = ("fp32", "bf16", "fp16")
    add("predict_c2", every, mode="predict")
    add("predict_c2_L2", every, mode="predict", L=2)
    add("predict_c2_overlap", fp32, mode="predict", attrs=dict(overlaps={"fwd"}))
    add("predict_w8_c3", shape="c3_small", mode="predict", world="w8", comm="segments")
    add("predict_c2_metrics", fp32, mode="predict", metrics=True)
    return out


CASES = _cases()


def _comm(kind):
    from dlrm_hip.trainer import EmulatedComm
    comm = EmulatedComm(whole=kind == "whole")
    if kind == "eager":  # no collective captures: the eager segment order
        comm.capture_ar = False
    return comm


def build(case):
    """(trainer, batch) of a case, as test_gpu_lr_trainer._trainer builds them."""
    from dlrm_hip.trainer import DLRMTrainer, TrainerConfig
    c = shapes()[case["shape"]]
    lr, elr = RATES[case["optimizer"]]
    F = len(c["rows"]) + 1
    cfg = TrainerConfig(
        m_spa=c["D"], ln_emb=c["rows"], ln_bot=c["bot"],
        ln_top=[c["D"] + F * (F - 1) // 2] + c["top"], loss_function="bce", learning_rate=lr,
        emb_learning_rate=elr, optimizer=case["optimizer"],
        mlp_precision=case["precision"] if case["mode"] == "train" else "fp32", **case["cfg"])
    if case["world"] == "one":
        tr = DLRMTrainer(cfg, device=DEV, seed=3)
    else:
        tr = DLRMTrainer(cfg, device=DEV, rank=2, world_size=8, comm=_comm(case["comm"]), seed=3)
    for k, v in case["attrs"].items():
        assert hasattr(tr, k), k
        setattr(tr, k, set(v) if isinstance(v, set) else v)
    return tr, tr.synthetic_batch(c["B"], case["L"], seed=11)


class Recorder:
    """Stands in for dlrm_hip._lib.call while installed."""

    def __init__(self):
        self.calls = []
        self._segments = []  # (address, size) of the caching allocator's device segments

    def _device(self, addr):
        import torch
        for _try in range(2):
            if any(a <= addr < a + n for a, n in self._segments):
                return True
            self._segments = [(s["address"], s["total_size"])
                              for s in torch.cuda.memory_snapshot()]
        return False

    def _arg(self, a):
        import torch
        if a is None or isinstance(a, (bool, int, float)):
            return a
        if isinstance(a, ctypes.c_void_p) and a._objects is None:
            v = a.value or 0
            if v == torch.cuda.current_stream(DEV).cuda_stream or (v and self._device(v)):
                return ("ptr", v)
        return "*"

    def __call__(self, name, *args):
        self.calls.append([name] + [self._arg(a) for a in args])
        return self._real(name, *args)

    def take(self):
        calls, self.calls = self.calls, []
        return calls

    @contextlib.contextmanager
    def installed(self):
        from dlrm_hip import _lib
        self._real = _lib.call
        _lib.call = self
        try:
            yield self
        finally:
            _lib.call = self._real

    @contextlib.contextmanager
    def group(self, name):  # the profile= hook
        self.calls.append(["prof", name])
        yield


def label(segments):
    """Pointers of a trace (a list of call lists) -> "p<k>" in order of first appearance."""
    names = {}
    return [[[names.setdefault(a, f"p{len(names)}") if isinstance(a, tuple) else a
              for a in call] for call in calls] for calls in segments]


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


@contextlib.contextmanager
def _count_replays(counter):
    import torch
    real = torch.cuda.CUDAGraph.replay

    def replay(g):
        counter[0] += 1
        return real(g)
    torch.cuda.CUDAGraph.replay = replay
    try:
        yield
    finally:
        torch.cuda.CUDAGraph.replay = real


def run_case(case):
    """The record of one case (see the module docstring)."""
    import torch
    tr, batch = build(case)
    rec = Recorder()
    train = case["mode"] == "train"
    metrics = None
    if case["metrics"]:
        from dlrm_hip.metrics import EvalState
        metrics = EvalState(4 * batch.X.shape[0], DEV)
    if train:
        make = lambda: tr.segments(batch, rec.group if case["profile"] else None)  # noqa: E731
        capture = lambda: tr.capture(batch)  # noqa: E731
        prob, loss = tr.step(batch)  # the first step of a batch size allocates
    else:
        make = lambda: tr.predict_segments(batch, metrics, case["precision"])  # noqa: E731
        capture = lambda: tr.capture_predict(batch, metrics,  # noqa: E731
                                             precision=case["precision"])
        prob = tr.predict(batch, metrics, case["precision"])
    torch.cuda.synchronize()
    replays = [0]
    with rec.installed(), _count_replays(replays):
        segs = make()
        trace = [rec.take()]
        for _kind, fn in segs:
            fn()
            trace.append(rec.take())
        torch.cuda.synchronize()
        run = capture()
        captured = label([rec.take()])[0]
        replays[0] = 0
        run()
        assert not rec.take(), "a replay launches through graphs only"
    torch.cuda.synchronize()
    tr.check_errors()
    trace = label(trace)
    out = dict(kinds=[kind for kind, _fn in segs], trace=trace,
               capture_trace="same" if captured == [c for s in trace for c in s] else captured)
    assert case["profile"] or out["capture_trace"] == "same", "capture launches differently"
    out["replays"] = replays[0]
    if train:
        out.update(capture_mode=tr.capture_mode, graphs_per_step=tr.graphs_per_step)
        state = dict(prob=prob, loss=loss, params=tr.params, momentum=tr.momentum,
                     adagrad_sum=tr.adagrad_sum, grads=tr.grads)
        if tr.total_rows:  # a rank without tables: a placeholder row nobody writes
            state["weights"] = tr.weights
    else:
        state = dict(prob=prob)
        if metrics is not None:  # three passes logged: the eager two and the replay
            n = 3 * batch.X.shape[0]
            assert metrics.count == n
            state.update(log=metrics.keys[:n], counters=metrics.ctrl)
    out["sha256"] = {k: _sha(t) for k, t in sorted(state.items()) if t is not None}
    return out


def first_diff(got, want, path=""):
    """Where two records first differ, as text (None: they are equal)."""
    if type(got) is not type(want):
        return f"{path}: {got!r} vs {want!r}"
    if isinstance(got, dict):
        for k in list(want) + [k for k in got if k not in want]:
            if k not in got or k not in want:
                return f"{path}.{k}: only on one side"
            d = first_diff(got[k], want[k], f"{path}.{k}")
            if d:
                return d
        return None
    if isinstance(got, list) and got and isinstance(got[0], (list, dict)):
        for i, (a, b) in enumerate(zip(got, want)):
            d = first_diff(a, b, f"{path}[{i}]")
            if d:
                return d
        if len(got) != len(want):
            extra = (got if len(got) > len(want) else want)[min(len(got), len(want))]
            return f"{path}: {len(got)} vs {len(want)} entries; first extra: {extra!r}"
        return None
    return None if got == want else f"{path}: {got!r} vs {want!r}"


def device_id():
    import torch
    p = torch.cuda.get_device_properties(DEV)
    return dict(name=p.name, multi_processor_count=p.multi_processor_count)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "step_trace.json"))
    ap.add_argument("--only", nargs="*")
    args = ap.parse_args()
    names = args.only or list(CASES)
    records = {}
    for name in names:
        records[name] = run_case(CASES[name])
        print(name, records[name]["kinds"].count("gpu"), "gpu segments,",
              sum(len(s) for s in records[name]["trace"]), "calls", flush=True)
    d = None if args.only else first_diff(records[NO_EFFECT_CASE], records[NO_EFFECT_BASE])
    assert d is None, f"bf16: an option without an effect had one: {d}"
    with open(args.out, "w") as f:  # one case per line
        f.write('{"device": %s,\n "cases": {\n' % json.dumps(device_id()))
        f.write(",\n".join(f'  {json.dumps(n)}: {json.dumps(records[n], separators=(",", ":"))}'
                           for n in names))
        f.write("\n }\n}\n")
    print("wrote", args.out, len(names), "cases")


if __name__ == "__main__":
    main()
