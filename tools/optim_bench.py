#!/usr/bin/env python
"""optimizer.step() of adam, adamod and lamb on the bert-base arena (bf16 store with a compute copy): HIP-event
medians, 20 warm-up and 50 timed iterations each, random gradients, one model built once.  For LAMB also the three
launches one by one (lamb_moments / lamb_ratio / lamb_apply through their phase bindings).  Starts nothing else on
the GPU.

    python tools/optim_bench.py [--model bert-base-uncased] [--warmup 20] [--iters 50] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ml_recipe_distributed_pytorch_amd._native import kernels  # noqa: E402
from ml_recipe_distributed_pytorch_amd.models.bert import BertForQuestionAnswering  # noqa: E402
from ml_recipe_distributed_pytorch_amd.models.config import get_config  # noqa: E402
from ml_recipe_distributed_pytorch_amd.train.optim import FusedAdaMod, FusedAdamW, FusedLamb  # noqa: E402
from ml_recipe_distributed_pytorch_amd.train.trainer import optimizer_groups  # noqa: E402


def median_us(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(t), t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="bert-base-uncased")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model = BertForQuestionAnswering(get_config(a.model), seed=0).to(dev)
    st = model.store
    assert st.compute.data_ptr() != st.master.data_ptr(), "expected a bf16 store with a compute copy"
    st.grad.copy_(torch.randn(st.grad.shape, generator=torch.Generator().manual_seed(0)).to(dev) * 1e-3)
    clip = torch.tensor([0.5], device=dev)
    n = st.master.numel()

    def groups(lamb=False):
        g = optimizer_groups(list(model.named_parameters()), 1e-4)
        if lamb:
            g[1]["adapt"] = False
        return g

    make = {"adam": lambda: FusedAdamW(groups(), st, lr=1e-5, eps=1e-6, correct_bias=False),
            "adamod": lambda: FusedAdaMod(groups(), st, lr=1e-5),
            "lamb": lambda: FusedLamb(groups(True), st, lr=1e-5, eps=1e-6)}
    out = {"device": torch.cuda.get_device_name(0), "model": a.model, "arena_floats": n, "warmup": a.warmup,
           "iters": a.iters, "step_us": {}}
    print(f"{out['device']}  {a.model}: {n} parameters in the arena, {len(st.segments())} segments")
    print(f"{'optimizer':10s} {'median us':>10s} {'min':>9s} {'max':>9s}")
    lamb = None
    for name, mk in make.items():
        opt = mk()
        med, lo, hi = median_us(lambda: opt.step(clip_coef=clip), a.warmup, a.iters)
        out["step_us"][name] = {"median": med, "min": lo, "max": hi}
        print(f"{name:10s} {med:10.1f} {lo:9.1f} {hi:9.1f}")
        if name == "lamb":
            lamb = opt
        else:
            del opt
    # the three LAMB launches one by one, on the optimizer's own plan and state
    k, plan = kernels(), lamb._lamb_plan()
    pg = lamb.param_groups
    tab = ([g["lr"] for g in pg], [g["weight_decay"] for g in pg], [bool(g["adapt"]) for g in pg])
    hyp = (0.9, 0.999, 1e-6, 1.0 / (1.0 - 0.9 ** 100), 1.0 / (1.0 - 0.999 ** 100))
    m, v = lamb._arenas["exp_avg"], lamb._arenas["exp_avg_sq"]
    phases = {"lamb_moments": lambda: k.lamb_moments(plan, st.master, st.grad, m, v, *tab, *hyp, clip, lamb._partials,
                                                     lamb._norms),
              "lamb_ratio": lambda: k.lamb_ratio(plan, *tab, lamb._partials, lamb._norms),
              "lamb_apply": lambda: k.lamb_apply(plan, st.master, st.compute, m, v, *tab, *hyp, lamb._partials,
                                                 lamb._norms)}
    out["lamb_phase_us"] = {}
    for name, fn in phases.items():
        med, lo, hi = median_us(fn, a.warmup, a.iters)
        out["lamb_phase_us"][name] = {"median": med, "min": lo, "max": hi}
        print(f"  {name:14s} {med:10.1f} {lo:9.1f} {hi:9.1f}")
    adam = out["step_us"]["adam"]["median"]
    print(f"lamb / adam = {out['step_us']['lamb']['median'] / adam:.3f}  (bytes moved: 42 / 30 = 1.4)")
    assert torch.isfinite(st.master).all()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
