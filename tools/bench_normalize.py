"""Developer tool (GPU): the entry points of csrc/intensity.hip (percentile select, windows, z-score over a selected set, any-channel
threshold) and the normalisers composed from them, timed with HIP events against their HBM floor.

    python tools/bench_normalize.py [--reps 20] [--warmup 3] [--out profiles/normalize.txt]

Cases: a 4 x 240 x 240 x 155 fp32 volume (the four BraTS modalities), once RANDOM (Gaussian x 100: every histogram bin of a pass is hit)
and once 60 % ZEROS (exact zeros scattered at random among a Gaussian foreground: the dominant bin of a skull-stripped MR channel, and
the worst placement for it -- no run of zeros is longer than a few voxels, so nothing but the wave-level aggregation helps).
  stream rate: a device-to-device copy of the volume (read 4, write 4 bytes per voxel), median of --reps.
  per op:      median of --reps calls between HIP events; floor = the bytes the op MUST move (every input read once, every output written
               once) at the stream rate; "x floor" = time / floor. The passes of percentiles (four reads of the volume) and of
               zscore_select (two reads, one write) move more than the compulsory bytes: the note says how much."""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
normalize = importlib.import_module("3dunetcnn_amd.normalize")
prepost = importlib.import_module("3dunetcnn_amd.prepost")
ops = importlib.import_module("3dunetcnn_amd.ops")
_lib = importlib.import_module("3dunetcnn_amd._lib")
C, DHW = 4, (240, 240, 155)


def make_volume(kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(C, *DHW, generator=g) * 100
    if kind == "zeros60":
        x = torch.where(torch.rand(C, *DHW, generator=g) < 0.6, torch.zeros(()), x * 0.5 + 300)
    return x.contiguous()


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normalize.txt"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed calls")
    be = ops.default_backend()
    vox = C * DHW[0] * DHW[1] * DHW[2]
    lines = [f"tools/bench_normalize.py on {torch.cuda.get_device_name(0)}: {C} x {DHW[0]} x {DHW[1]} x {DHW[2]} fp32 volume ({vox / 1e6:.1f} M voxels, "
             f"{vox * 4 / 1e6:.0f} MB), median of {args.reps} calls"]
    summary = {}
    for kind in ("random", "zeros60"):
        x = make_volume(kind).cuda()
        y = torch.empty_like(x)
        med, _, _ = timed(lambda: y.copy_(x), args.reps, args.warmup)
        rate = vox * 8 / (med * 1e-3)
        lines.append(f"{kind}: stream rate (device copy, {vox * 8 / 1e6:.0f} MB) {med:.3f} ms = {rate / 1e12:.3f} TB/s")
        flat = x.reshape(C, -1)
        thr = be.percentiles(flat, [1.0, 99.0])[0]
        lo, hi = thr[:, 0].contiguous(), thr[:, 1].contiguous()
        one = x[:1].contiguous()
        wl = torch.tensor([0.0, -50.0, 100.0, 200.0], device=x.device)
        wh = torch.tensor([80.0, 300.0, 400.0, 1700.0], device=x.device)
        # (op, call, compulsory bytes, what the passes move on top)
        rows = (("percentiles nq=1", lambda: be.percentiles(flat, [50.0]), vox * 4, "4 reads of the volume"),
                ("percentiles nq=4", lambda: be.percentiles(flat, [1.0, 50.0, 90.0, 99.0]), vox * 4, "4 reads of the volume"),
                ("percentiles nq=1 above", lambda: be.percentiles(flat, [99.0], above=lo), vox * 4, "4 reads of the volume"),
                ("window CLAMP", lambda: be.window(flat, lo, hi, _lib.WINDOW_CLAMP), vox * 8, ""),
                ("window RESCALE", lambda: be.window(flat, lo, hi, _lib.WINDOW_RESCALE), vox * 8, ""),
                ("window SHIFT_FLOOR", lambda: be.window(flat, lo, None, _lib.WINDOW_SHIFT_FLOOR), vox * 8, ""),
                ("window RESCALE 1 -> 4 channels", lambda: be.window(one, wl, wh, _lib.WINDOW_RESCALE, channels=4), vox * 5, ""),
                ("zscore_select NONZERO", lambda: be.zscore_select(flat, _lib.SELECT_NONZERO, 0.0, True, 0, True), vox * 8, "2 reads, 1 write"),
                ("zscore_select ALL", lambda: be.zscore_select(flat, _lib.SELECT_ALL, 0.0, True, 1, False), vox * 8, "2 reads, 1 write"),
                ("threshold_any", lambda: be.threshold_any(flat, hi), vox * 4 + vox // C, ""),
                ("zero_one_window (21 launches)", lambda: normalize.zero_one_window(x), vox * 8, "9 reads, 1 write"),
                ("zero_floor_normalize (14 launches)", lambda: normalize.zero_floor_normalize_image_data(x), vox * 8, "7 reads, 2 writes"),
                ("percentile_threshold (11 launches)", lambda: normalize.percentile_threshold(x, 0.9), vox * 4 + vox // C, "5 reads"),
                ("normalize_intensity nonzero", lambda: prepost.normalize_intensity(x, nonzero=True), vox * 8, "2 reads, 1 write"))
        for name, fn, byts, note in rows:
            med, lo_ms, hi_ms = timed(fn, args.reps, args.warmup)
            floor_ms = byts / rate * 1e3
            summary[(kind, name)] = (med, floor_ms)
            lines.append(f"  {name:36s} {med:8.3f} ms [min {lo_ms:.3f}, max {hi_ms:.3f}]; must move {byts / 1e6:6.0f} MB: floor {floor_ms:6.3f} ms, "
                         f"{med / floor_ms:5.2f} x floor{'; ' + note if note else ''}")
            print(lines[-1], flush=True)
    lines.append("zeros60 / random, per op: " + ", ".join(
        f"{name} {summary[('zeros60', name)][0] / summary[('random', name)][0]:.2f}" for (kind, name) in summary if kind == "random"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
