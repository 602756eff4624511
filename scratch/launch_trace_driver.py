"""One launch of every branch of the kernel-selection policy of csrc/launch.hpp (EXPERIMENTS.md section AS).  Run from the repository
root under `rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scratch/launch_trace_driver.py`, once per library
(HIERDIFF_LIB selects it), then compare the two traces with scratch/launch_trace_diff.py."""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from oracle import egnn_oracle as orc                                   # noqa: E402
from tests.test_gpu_parity import DEV, build_dynamics                   # noqa: E402
from hierdiff_amd import _lib                                           # noqa: E402
from hierdiff_amd.weights import synthetic_state_dict                   # noqa: E402

N = 30
print("library:", _lib.LIB_PATH, flush=True)

# ---- sampler forward: every branch of the edge and node policies
BATCHES = [("split", 2), ("split_fp32_only", 22), ("mixed_both", 46), ("mixed_fp32_only", 64), ("plain", 150), ("fused_fp16x3", 100),
           ("fused_fp32", 190)]
base = ([30, 17, 1, 24, 30, 9] + [30] * 26) * 2 + [30] * 86
def sec_forward():
  with torch.no_grad():
    for H in (64, 256):
        sd_np = synthetic_state_dict(9, 0, H, 1, 2, True, 616, 1.0)
        for prec in ("fp32", "fp16x3"):
            dyn = build_dynamics(sd_np, H, 1, 0)
            dyn.precision = prec
            for name, B in BATCHES:
                if name in ("mixed_both", "mixed_fp32_only", "plain"):      # the batch of test_mixed_edge_launch_is_bit_identical and its heads
                    xh, nm, em = (v[:B].contiguous() for v in orc.random_inputs(base, 8, 36, N))
                else:
                    xh, nm, em = orc.random_inputs([30] * B, 8, 36, N)
                xh, nm, em = xh.to(DEV), nm.to(DEV), em.to(DEV)
                t = torch.linspace(0.05, 0.95, B, device=DEV).view(-1, 1)
                info = dyn.topology(nm, em, B, N).info()
                out = dyn._forward(t, xh, nm, em, None, None)
                torch.cuda.synchronize()
                assert torch.isfinite(out).all()
                print(f"forward H={H} {prec} {name} B={B}: tiles {info['tiles']} nodes {info['nodes']} sum {float(out.double().sum()):.9e}", flush=True)

# ---- training edge layers: hd_edge_layer_forward_s / _backward_s per arithmetic, with and without kept pre2
lib = _lib.load()
orig_fwd = lib.hd_edge_layer_forward_s
def sec_train():
  for H, B in ((256, 32), (64, 7)):
    sd_np = synthetic_state_dict(9, 0, H, 1, 2, True, 78, 0.5)
    xh, nm, em = orc.random_inputs([30] * (B - 2) + [17, 9], 8, 73)
    t = torch.linspace(0.1, 0.9, B).view(B, 1)
    for mode, keep in (("fp32", True), ("fp32", False), ("fp16x3", True)):
        dyn = build_dynamics(sd_np, H, 1)
        dyn.precision = "fp32"
        dyn.training_precision = mode
        dyn.keep_edge_activations = keep
        xg = xh.to(DEV).requires_grad_(True)
        out = dyn._forward(t.to(DEV), xg, nm.to(DEV), em.to(DEV), None, None)
        out.square().sum().backward()
        torch.cuda.synchronize()
        print(f"train H={H} {mode} keep={keep}: out {float(out.double().sum()):.9e} dx {float(xg.grad.double().sum()):.9e}", flush=True)
    # the fp16x3 forward without a kept pre2 (reachable through the C ABI only): strip the buffer, forward alone
    lib.hd_edge_layer_forward_s = lambda *a: orig_fwd(*a[:13], None, a[14])
    try:
        dyn = build_dynamics(sd_np, H, 1)
        dyn.precision = "fp32"
        dyn.training_precision = "fp16x3"
        xg = xh.to(DEV).requires_grad_(True)
        out = dyn._forward(t.to(DEV), xg, nm.to(DEV), em.to(DEV), None, None)
        torch.cuda.synchronize()
        print(f"train H={H} fp16x3 forward, no pre2: out {float(out.double().sum()):.9e}", flush=True)
    finally:
        lib.hd_edge_layer_forward_s = orig_fwd

# ---- E_GCL forward + backward at widths 32 and 128
from tests import fuzz_egcl_grads as fz                                 # noqa: E402
def sec_egcl():
  for H in (32, 128):
    rng = np.random.Generator(np.random.PCG64(100 + H))
    row, col = fz.dense_graph(2, 12)
    c = fz.make_case(rng, H=H, De=H, M=24, row=row, col=col)
    outs, grads = fz.hip_grads(c)
    torch.cuda.synchronize()
    print(f"egcl H={H}: out {float(outs[0].double().sum()):.9e} dh {float(grads['h'].double().sum()):.9e}", flush=True)

# ---- hd_gemm_f32: small, fast, bounds-checked, split-K
from hierdiff_amd import training as tr                                 # noqa: E402
def sec_gemm():
  for M, Nc, K in ((129, 512, 256), (7680, 256, 512), (300, 130, 77)):
    g = torch.Generator().manual_seed(M)
    X, W, b = torch.randn(M, K, generator=g).to(DEV), torch.randn(Nc, K, generator=g).to(DEV), torch.randn(Nc, generator=g).to(DEV)
    y = tr._linear_fwd(X, W, b)
    gy = torch.randn(M, Nc, generator=g).to(DEV)
    dx = tr._linear_dx(gy, W)
    dW, db = tr._linear_dw(gy, X, True)
    torch.cuda.synchronize()
    print(f"gemm {M}x{Nc}x{K}: y {float(y.double().sum()):.9e} dx {float(dx.double().sum()):.9e} dW {float(dW.double().sum()):.9e}", flush=True)
import traceback
failed = []
for sec in (sec_forward, sec_train, sec_egcl, sec_gemm):
    try:
        sec()
    except Exception:
        traceback.print_exc()
        failed.append(sec.__name__)
print("DRIVER DONE, failed sections:", failed, flush=True)
sys.exit(1 if failed else 0)
