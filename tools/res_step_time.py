"""Cost of residual blocks on an MI355X: the training step of the BraTS configuration (examples/brats2020: filters 64..384, 128^3, batch 2,
fp32) with res_block=False against res_block=True, and the kernels of csrc/res_block.hip on their own at the level-0 shape (64 channels,
128^3, batch 2; the shortcut conv from there to 96 channels at 64^3).

    python tools/res_step_time.py [--size 128] [--batch 2] [--steps 10] [--warmup 3] [--rounds 3]

Step time: device events around `steps` whole steps (zero_grad, forward, loss, backward, fused Adam), the two variants alternating
`rounds` times in one process so that they see the same machine state. Kernels: device events around 20 back-to-back calls after a warm-up
(a call of the join backward is its three launches, of the weight gradient its two). Per kernel: the time, the bytes its traffic floor
moves (join forward: 3 tensor passes; join backward: 10; gn_act_bwd on the same tensor, the yardstick of a streaming kernel: 5; the
shortcut: the even voxels of x once, y once), the achieved bytes / s and its fraction of the HBM peak (8.0 TB/s; a float4 copy measures
6.29 TB/s on this part). Prints one JSON line. Needs a GPU."""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dyn = importlib.import_module("3dunetcnn_amd.dynunet")
losses = importlib.import_module("3dunetcnn_amd.losses")
optim = importlib.import_module("3dunetcnn_amd.optim")
ops = importlib.import_module("3dunetcnn_amd.ops")
syn = importlib.import_module("3dunetcnn_amd.synthetic")
BRATS = dict(in_channels=4, out_channels=3, spatial_dims=3, strides=[[1, 1, 1]] + [[2, 2, 2]] * 5, filters=[64, 96, 128, 192, 256, 384],
             kernel_size=[[3, 3, 3]] * 6, upsample_kernel_size=[[2, 2, 2]] * 5)
HBM_PEAK = 8.0e12


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("res_step_time.py measures on an MI355X; no GPU is visible")
    s, n = a.size, a.batch
    x, y = (t.cuda() for t in syn.synthetic_case(n, 4, (s, s, s)))
    variants = {}
    for name, res in (("basic", False), ("residual", True)):
        torch.manual_seed(0)
        m = dyn.HipDynUNet(**dict(BRATS, res_block=res)).cuda().train()
        crit = losses.HipDiceLoss(sigmoid=True)
        opt = optim.HipAdam(m.parameters(), lr=1e-4)

        def step(m=m, crit=crit, opt=opt):
            opt.zero_grad(set_to_none=True)
            crit(m(x), y).backward()
            opt.step()
        variants[name] = step
    for step in variants.values():
        timed(step, a.warmup)
    ms = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, step in variants.items():
            ms[name].append(round(timed(step, a.steps), 3))
    ratio = round(min(ms["residual"]) / min(ms["basic"]), 4)
    del variants, step, m, crit, opt
    torch.cuda.empty_cache()
    # the kernels alone, level 0
    be = ops.default_backend()
    c, co, h = 64, 96, s // 2
    dev = "cuda"
    r2, r3, A, dA, d3 = (be.empty_act(n, s, s, s, c) for _ in range(5))
    for t in (r2, r3, dA):
        t.buf.normal_()
    gamma = torch.rand(c, device=dev) + 0.5
    st = [be.gn_stats(t, c, 1e-5, gamma, torch.zeros(c, device=dev)) for t in (r2, r3)]
    outs = [torch.empty(c, device=dev) for _ in range(4)]
    w = torch.randn(co, c, 1, 1, 1, device=dev) * 0.1
    y3, dy3 = be.empty_act(n, h, h, h, co), be.empty_act(n, h, h, h, co)
    dy3.buf.normal_()
    dw = torch.empty_like(w)
    tensor = r2.buf.numel() * 4
    even, coarse = tensor / 8, y3.buf.numel() * 4
    calls = {
        "res_join_fwd": (lambda: be.res_join_fwd(r2, st[0], r3, st[1], A, 0.01), 3 * tensor),
        "res_join_bwd": (lambda: be.res_join_bwd(A, dA, r2, st[0], gamma, r3, st[1], gamma, dA, d3, *outs, 0.01), 10 * tensor),
        "gn_act_bwd": (lambda: be.gn_act_bwd(r2, dA, dA, c, 0.01, gamma, *st[0], outs[0], outs[1]), 5 * tensor),
        "conv1x1_s2_fwd": (lambda: be.conv1x1_s2_fwd(A, w, y3), even + coarse),
        "conv1x1_s2_wgrad": (lambda: be.conv1x1_s2_wgrad(A, dy3, dw), even + coarse),
        "conv1x1_s2_dgrad_add": (lambda: be.conv1x1_s2_dgrad_add(dy3, w, d3), 2 * even + coarse),
    }
    kernels = {}
    for name, (fn, floor) in calls.items():
        timed(fn, 3)
        t_ms = timed(fn, 20)
        rate = floor / (t_ms * 1e-3)
        kernels[name] = dict(ms=round(t_ms, 4), floor_mb=round(floor / 1e6, 1), tb_per_s=round(rate / 1e12, 3), of_hbm_peak=round(rate / HBM_PEAK, 3))
    flops = 2.0 * n * h ** 3 * c * co
    for name in ("conv1x1_s2_fwd", "conv1x1_s2_wgrad", "conv1x1_s2_dgrad_add"):
        kernels[name]["tflops"] = round(flops / (kernels[name]["ms"] * 1e-3) / 1e12, 2)
    print(json.dumps(dict(config=dict(size=s, batch=n, steps=a.steps, rounds=a.rounds, level0=dict(channels=c, shortcut_to=co)), step_ms=ms,
                          residual_over_basic=ratio, hbm_peak_tb_per_s=HBM_PEAK / 1e12, kernels=kernels)))


if __name__ == "__main__":
    main()
