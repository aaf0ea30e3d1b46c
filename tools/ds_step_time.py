"""Cost of deep supervision on an MI355X: the training step of the BraTS configuration (examples/brats2020: filters 64..384, 128^3, batch 2,
fp32) with deep_supervision=False against deep_supr_num=2 with HipDeepSupervisionLoss(HipDiceLoss(sigmoid=True)), and the two head
kernels on their own at that configuration's head shapes.

    python tools/ds_step_time.py [--size 128] [--batch 2] [--steps 10] [--warmup 3] [--rounds 3]

Step time: device events around `steps` whole steps (zero_grad, forward, loss, backward, fused Adam), the two variants alternating
`rounds` times in one process so that they see the same machine state. Head kernels: device events around 20 back-to-back launches of
mi355_ds_head_fwd / mi355_ds_head_bwd (the backward includes its reduce launch) after a warm-up. Prints one JSON line. Needs a GPU."""
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
        raise SystemExit("ds_step_time.py measures on an MI355X; no GPU is visible")
    s = a.size
    x, y = (t.cuda() for t in syn.synthetic_case(a.batch, 4, (s, s, s)))
    variants = {}
    for name, K in (("plain", 0), ("ds2", 2)):
        torch.manual_seed(0)
        m = dyn.HipDynUNetDS(**dict(BRATS, deep_supervision=K > 0, deep_supr_num=max(K, 1))).cuda().train()
        crit = losses.HipDiceLoss(sigmoid=True)
        if K:
            crit = losses.HipDeepSupervisionLoss(crit)
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
    be = ops.default_backend()
    heads = {}
    for lvl, cin in ((1, 96), (2, 128)):
        f, c = 2 ** lvl, s // 2 ** lvl
        xa = be.empty_act(a.batch, c, c, c, cin)
        xa.buf.normal_()
        dA = be.zeros_act(a.batch, c, c, c, cin)
        w, b = torch.randn(3, cin, device="cuda") * 0.1, torch.zeros(3, device="cuda")
        sc, sh = torch.ones(a.batch, cin, device="cuda"), torch.zeros(a.batch, cin, device="cuda")
        out = torch.empty(a.batch, 3, s, s, s, device="cuda")
        dw, db = torch.empty(3, cin, device="cuda"), torch.empty(3, device="cuda")
        fwd = lambda: be.ds_head_fwd(xa, w, b, out, f, sc, sh, 0.01)
        bwd = lambda: be.ds_head_bwd(xa, w, out, dA, dw, db, f, sc, sh, 0.01)
        timed(fwd, 3), timed(bwd, 3)
        heads[f"level{lvl}_cin{cin}_x{f}"] = dict(fwd_ms=round(timed(fwd, 20), 4), bwd_ms=round(timed(bwd, 20), 4),
                                                 out_mb=round(out.numel() * 4 / 1e6, 1), x_mb=round(xa.buf.numel() * 4 / 1e6, 1))
    print(json.dumps(dict(config=dict(size=s, batch=a.batch, steps=a.steps, rounds=a.rounds), step_ms=ms, head_kernels=heads)))


if __name__ == "__main__":
    main()
