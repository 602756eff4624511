#!/usr/bin/env python3
"""Stage-2 training step timing (Edge_denoise.training_forward + backward + AdamW step through trainer.ddp_step) at the
reference's batch shape (bs = 2, H = 256, n = 12 - 30 fragments) and at a beam-sized bs = 24, n = 12; launches per step from the
torch profiler; one gcl_full layer's forward vs forward_train + backward.

    python scratch/stage2_train_timing.py [--out profiles/stage2_train_timing.json] [--steps 10]
"""
import argparse
import copy
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def step_time(H, n_list, stage_list, steps, dev):
    from hierdiff_amd.edge_denoise_train import CLIP_VAL, EdgeDenoise
    from hierdiff_amd.edge_denoise import synthetic_edge_denoise_state_dict
    from hierdiff_amd.trainer import ddp_step
    from oracle.edge_denoise_batches import train_batch
    kw = dict(vocab_size=50, in_node_nf=8, hidden_nf=H, out_node_nf=49)
    mod = EdgeDenoise({"model": dict(array_dict=None, full_softmax=True, focal_loss=5, edge_loss=1, node_loss=2, **kw)})
    mod.model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_edge_denoise_state_dict(3, **kw).items()})
    mod = mod.to(dev)
    [opt], _ = mod.configure_optimizers()
    batch = train_batch(7, n_list, stage_list, vocab_size=50)
    for _ in range(3):
        ddp_step(mod, copy.deepcopy(batch), opt, clip_val=CLIP_VAL, overlap=False)
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        b = copy.deepcopy(batch)
        t0 = time.perf_counter()
        r = ddp_step(mod, b, opt, clip_val=CLIP_VAL, overlap=False)
        float(r["loss"])
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ddp_step(mod, copy.deepcopy(batch), opt, clip_val=CLIP_VAL, overlap=False)
        torch.cuda.synchronize()
    kern = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return {"H": H, "n_list": n_list, "stage_list": stage_list, "step_ms_median": 1e3 * float(np.median(ts)),
            "step_ms_min": 1e3 * float(np.min(ts)), "gpu_ops_per_step": len(kern),
            "gpu_busy_ms": sum(e.device_time for e in kern) / 1e3 if kern and hasattr(kern[0], "device_time") else None}


def layer_time(dev, reps=50):
    """One gcl_full layer (H = 256, attention, edge update, both masks) at bs = 24, n = 12 (E = 3,456)."""
    from hierdiff_amd.stage2 import E_GCL, synthetic_egcl_state_dict
    H, bs, n = 256, 24, 12
    rng = np.random.Generator(np.random.PCG64(5))
    ar = torch.arange(n)
    row = (ar.repeat_interleave(n).repeat(bs) + (torch.arange(bs) * n).repeat_interleave(n * n)).to(dev)
    col = (ar.repeat(n).repeat(bs) + (torch.arange(bs) * n).repeat_interleave(n * n)).to(dev)
    nm = torch.ones(bs * n, 1, device=dev)
    em = (row != col).float().unsqueeze(1)
    m = E_GCL(H, H, H, edges_in_d=H, attention=True, tanh=True, coords_range=30, edge_update=True)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in synthetic_egcl_state_dict(H, H, 0, True, True, 1, coord_gain=0.3).items()})
    m = m.to(dev)
    h = torch.from_numpy(rng.standard_normal((bs * n, H)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((bs * n, 3)).astype(np.float32)).to(dev)
    ea = torch.from_numpy(rng.standard_normal((row.numel(), H)).astype(np.float32)).to(dev)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def fwd():
        with torch.no_grad():
            m(h, [row, col], x, edge_attr=ea, node_mask=nm, edge_mask=em)

    hg = h.clone().requires_grad_(True)
    outs = {}

    def fwd_train():
        outs["o"] = m(hg, [row, col], x, edge_attr=ea, node_mask=nm, edge_mask=em)

    def fwd_bwd():
        o = m(hg, [row, col], x, edge_attr=ea, node_mask=nm, edge_mask=em)
        torch.autograd.backward(o, [torch.ones_like(t) for t in o])

    t_f, t_ft, t_fb = timed(fwd), timed(fwd_train), timed(fwd_bwd)
    return {"layer": "gcl_full H=256 bs=24 n=12", "forward_ms": t_f, "forward_train_ms": t_ft, "forward_train_plus_backward_ms": t_fb,
            "backward_ms_est": t_fb - t_ft}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "stage2_train_timing.json"))
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "steps": a.steps,
           "train_step": [step_time(256, [12, 30], [5, 11], a.steps, dev),
                          step_time(256, [12] * 24, [int(s) for s in np.random.Generator(np.random.PCG64(1)).integers(1, 11, 24)],
                                    a.steps, dev)],
           "layer": layer_time(dev)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
