"""Developer tool (GPU): the fused training augmentation (Backend.augment_batch, two launches per batch) against the way to the same
tensors without it -- per sample Backend.resample_affine for the image and for the label, Backend.zscore, torch for gain and offset --
timed in the same run, alternating, with HIP events around every repetition.

    python tools/bench_augment.py [--reps 30] [--warmup 5] [--skip-loop] [--out profiles/augment_bench.json]

Cases: batch 2 of 4 image + 3 uint8 label channels at 128^3 -> 128^3 and 192^3 -> 192^3, each with (a) flips only and (b) a rotation of
0.2 rad about all three axes + zoom, `normalize` on, gain and offset drawn. Algorithmic bytes of the fused call: every source voxel read
once, every output voxel written once, the image read and written once more by the finalising pass. The baseline needs fp32 labels
(resample_affine has no uint8 form): it is timed both with the uint8 <-> fp32 conversions it needs to reach the same tensors and with
labels that are fp32 already. Then `ms_per_step` of a 20-step 128^3 batch-2 training loop fed by DeviceStager with and without the
augmentation (the augmentation runs on the copy stream)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module("3dunetcnn_amd.ops")
aug = importlib.import_module("3dunetcnn_amd.augment")
N, CI, CL = 2, 4, 3
GROUPS = [[1, 2, 4], [1, 4], [4]]


def maps(kind, size):
    dhw = (size,) * 3
    flip = lambda axes: {"name": "RandFlipD", "spatial_axis": axes, "prob": 1.0}
    if kind == "flips":
        per_sample = [[flip([0, 1])], [flip(2)]]
    else:
        rot = lambda a: {"name": "RandRotateD", "prob": 1.0, "range_x": [a, a], "range_y": [a, a], "range_z": [a, a]}
        zoom = lambda f: {"name": "RandZoomD", "prob": 1.0, "min_zoom": f, "max_zoom": f}
        per_sample = [[rot(0.2), zoom(1.1)], [rot(-0.2), zoom(0.9)]]
    return torch.cat([aug.HipAugmenter(spatial_augmentations=e).sample_params(1, dhw).matrices for e in per_sample])


def stats(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "iqr_ms": q[2] - q[0], "reps": len(ms)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return e0, e1, out


def bench_case(be, size, kind, reps, warmup):
    dev = be.device
    g = torch.Generator(device="cpu").manual_seed(size)
    img = (torch.randn(N, CI, size, size, size, generator=g) * 3 + 10).to(dev)
    lab = (torch.rand(N, CL, size, size, size, generator=g) < 0.4).to(torch.uint8).to(dev)
    lab32 = lab.float()
    m = maps(kind, size)
    md = m.to(dev)
    gain, offset = (1 + 0.1 * (2 * torch.rand(N, CI, generator=g) - 1)), 0.1 * (2 * torch.rand(N, CI, generator=g) - 1)
    gd, od = gain.to(dev), offset.to(dev)
    dhw = (size,) * 3

    def fused():
        return be.augment_batch(img, lab, md, gd, od, dhw, "border", True)

    def baseline(label, convert):
        outs, labs = [], []
        for s in range(N):
            x = be.zscore(be.resample_affine(img[s], dhw, m[s].reshape(-1).tolist(), "trilinear", "border"))
            outs.append(x * gd[s].view(-1, 1, 1, 1) + od[s].view(-1, 1, 1, 1))
            l = be.resample_affine(label[s].float() if convert else label[s], dhw, m[s].reshape(-1).tolist(), "nearest", "border")
            labs.append(l.to(torch.uint8) if convert else l)
        return torch.stack(outs), torch.stack(labs)

    variants = {"fused": fused, "baseline": lambda: baseline(lab, True), "baseline_fp32_labels": lambda: baseline(lab32, False)}
    for _ in range(warmup):
        for f in variants.values():
            f()
    torch.cuda.synchronize()
    a, b = fused(), baseline(lab, True)
    same = {"image_max_abs_diff": float((a[0] - b[0]).abs().max()), "label_mismatch_share": float((a[1] != b[1]).float().mean())}
    del a, b
    ev = {k: [] for k in variants}
    for _ in range(reps):                                   # alternating, so that drift of the machine hits every variant alike
        for k, f in variants.items():
            e0, e1, out = timed(f)
            ev[k].append((e0, e1))
            del out
    torch.cuda.synchronize()
    res = {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}
    vox = N * size ** 3
    byts = vox * (CI * 4 + CL) * 2 + vox * CI * 4 * 2       # source once + output once + image re-read and re-written by pass B
    res["algorithmic_bytes"] = byts
    res["fused_TB_per_s"] = byts / (res["fused"]["median_ms"] * 1e-3) / 1e12
    for k in ("baseline", "baseline_fp32_labels"):
        res[f"speedup_vs_{k}"] = res[k]["median_ms"] / res["fused"]["median_ms"]
        # "faster by more than the spread": the slowest fused repetition against the fastest baseline repetition
        res[f"faster_than_{k}_beyond_spread"] = res["fused"]["max_ms"] < res[k]["min_ms"]
    res["fused_vs_baseline"] = same
    return res


def train_loop(augment, steps=20, warmup=3, size=128):
    staging = importlib.import_module("3dunetcnn_amd.staging")
    unet = importlib.import_module("3dunetcnn_amd.unet")
    losses = importlib.import_module("3dunetcnn_amd.losses")
    optim = importlib.import_module("3dunetcnn_amd.optim")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    pool = [{"image": (torch.randn(N, CI, size, size, size, generator=g) * 3 + 10).pin_memory(),
             "label": torch.randint(0, 5, (N, 1, size, size, size), generator=g).float().pin_memory()} for _ in range(4)]
    data = [pool[i % len(pool)] for i in range(steps + warmup)]
    m = unet.HipUNet3D(n_features=CI, n_outputs=CL).cuda().train()
    crit, opt = losses.HipDiceLoss(sigmoid=True), optim.HipAdam(m.parameters(), lr=1e-3)
    a = None
    if augment:
        a = aug.HipAugmenter(spatial_augmentations=[{"name": "RandFlipD", "spatial_axis": 0, "prob": 0.5}, {"name": "RandFlipD", "spatial_axis": 1, "prob": 0.5},
                                                    {"name": "RandRotateD", "prob": 1.0, "range_x": 0.2, "range_y": 0.2, "range_z": 0.2}],
                             intensity_augmentations=[{"name": "RandScaleIntensityD", "factors": 0.1, "prob": 1.0},
                                                      {"name": "RandShiftIntensityD", "offsets": 0.1, "prob": 1.0}],
                             normalize=True, generator=torch.Generator().manual_seed(2))
    st = staging.DeviceStager(data, normalize=True, one_hot_labels=GROUPS, augment=a)
    t0 = loss = None
    for i, b in enumerate(st):
        if i == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        opt.zero_grad(set_to_none=True)
        loss = crit(m(b["image"]), b["label"])
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return {"ms_per_step": (time.perf_counter() - t0) * 1e3 / steps, "steps": steps, "final_loss": float(loss.detach())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 192])
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed launches")
    be = ops.default_backend()
    res = {"device": torch.cuda.get_device_name(0), "batch": N, "image_channels": CI, "label_channels": CL, "cases": {}}
    for size in args.sizes:
        for kind in ("flips", "rotate_zoom"):
            r = bench_case(be, size, kind, args.reps, args.warmup)
            res["cases"][f"{size}^3 {kind}"] = r
            print(f"{size}^3 {kind}: fused {r['fused']['median_ms']:.3f} ms [{r['fused']['min_ms']:.3f}, {r['fused']['max_ms']:.3f}] "
                  f"({r['fused_TB_per_s']:.2f} TB/s), baseline {r['baseline']['median_ms']:.3f} ms [{r['baseline']['min_ms']:.3f}, "
                  f"{r['baseline']['max_ms']:.3f}], fp32-label baseline {r['baseline_fp32_labels']['median_ms']:.3f} ms; "
                  f"x{r['speedup_vs_baseline']:.2f} / x{r['speedup_vs_baseline_fp32_labels']:.2f}; {r['fused_vs_baseline']}", flush=True)
    if not args.skip_loop:
        res["train_loop_128^3_batch2"] = {"stager_plain": train_loop(False), "stager_augment": train_loop(True)}
        # a second pair in the other order: the spread of the loop itself
        res["train_loop_128^3_batch2_repeat"] = {"stager_augment": train_loop(True), "stager_plain": train_loop(False)}
        print(json.dumps({k: v for k, v in res.items() if k.startswith("train_loop")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
