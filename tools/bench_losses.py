"""Developer tool (GPU): forward + backward of the loss modules, and the streaming loss passes on their own, timed with HIP events.

    python tools/bench_losses.py [--reps 30] [--warmup 5] [--out profiles/losses.txt]

Case: logits fp32 [2, 3, 128, 128, 128] (the headline step's output), uint8 one-hot targets (nested regions). One run times the new
HipFocalLoss / HipDiceFocalLoss / HipTverskyLoss AND the existing HipDiceCELoss / HipBCEWithLogitsLoss, so that the focal pass has its
yardstick -- mi355_ce_fwd_bwd, which moves the same bytes -- from the same minutes of the same device.
  per row: median [min, max] of --reps calls between HIP events, the bytes the row MUST move (every kernel pass reads its inputs once and
           writes its outputs once; E = n * c * voxels elements: logits 4 B, uint8 target 1 B, gradient 4 B) and that divided by the time.
           A module row includes autograd's bookkeeping and the in-place `dlogits *= upstream` of backward (8 B per element)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
losses = importlib.import_module("3dunetcnn_amd.losses")
ops = importlib.import_module("3dunetcnn_amd.ops")
syn = importlib.import_module("3dunetcnn_amd.synthetic")
N, C, DHW = 2, 3, (128, 128, 128)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses.txt"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed calls")
    be = ops.default_backend()
    target = syn.synthetic_case(N, 1, DHW, C, 0)[1].to(torch.uint8).cuda().contiguous()
    logits = (torch.randn(N, C, *DHW, generator=torch.Generator().manual_seed(0)) * 2).cuda()
    E = logits.numel()
    dz = torch.zeros_like(logits)
    one = torch.zeros(1, device="cuda")

    def module(crit):
        def run():
            z = logits.detach().requires_grad_(True)
            crit(z, target).backward()
        return run
    # (row, call, bytes per element the row must move)
    rows = (("pass mi355_ce_fwd_bwd (bce), fresh gradient", lambda: be.cross_entropy(logits, target, mode="bce"), 9),
            ("pass mi355_focal_fwd_bwd (sigmoid, gamma 2), fresh gradient", lambda: be.focal(logits, target, gamma=2.0), 9),
            ("pass mi355_focal_fwd_bwd (sigmoid, gamma 2, alpha), fresh", lambda: be.focal(logits, target, gamma=2.0, alpha=0.25), 9),
            ("pass mi355_ce_fwd_bwd (softmax), fresh gradient", lambda: be.cross_entropy(logits, target, mode="softmax"), 9),
            ("pass mi355_focal_fwd_bwd (softmax, gamma 2), fresh gradient", lambda: be.focal(logits, target, mode="softmax", gamma=2.0), 9),
            ("pass mi355_ce_fwd_bwd (bce), accumulating", lambda: be.cross_entropy(logits, target, mode="bce", weight=1e-3, loss=one, dlogits=dz), 13),
            ("pass mi355_focal_fwd_bwd (sigmoid), accumulating", lambda: be.focal(logits, target, gamma=2.0, weight=1e-3, loss=one, dlogits=dz), 13),
            ("HipBCEWithLogitsLoss fwd + bwd", module(losses.HipBCEWithLogitsLoss()), 9 + 8),
            ("HipFocalLoss fwd + bwd", module(losses.HipFocalLoss()), 9 + 8),
            ("HipDiceCELoss(sigmoid) fwd + bwd", module(losses.HipDiceCELoss(sigmoid=True)), 5 + 9 + 13 + 8),
            ("HipDiceFocalLoss(sigmoid) fwd + bwd", module(losses.HipDiceFocalLoss(sigmoid=True)), 5 + 9 + 13 + 8),
            ("HipTverskyLoss(sigmoid) fwd + bwd", module(losses.HipTverskyLoss(sigmoid=True, alpha=0.3, beta=0.7)), 5 + 9))
    lines = [f"tools/bench_losses.py on {torch.cuda.get_device_name(0)}: logits fp32 [{N}, {C}, {DHW[0]}, {DHW[1]}, {DHW[2]}] "
             f"({E / 1e6:.2f} M elements), uint8 targets; median [min, max] of {args.reps} calls between HIP events after {args.warmup} warm-up calls"]
    for name, fn, per in rows:
        med, lo, hi = timed(fn, args.reps, args.warmup)
        byts = per * E
        lines.append(f"  {name:60s} {med * 1e3:8.1f} us [{lo * 1e3:.1f}, {hi * 1e3:.1f}]; must move {byts / 1e6:6.1f} MB = {byts / (med * 1e-3) / 1e9:7.1f} GB/s")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
