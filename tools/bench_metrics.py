"""Developer tool (GPU): metrics.evaluate (overlap counts, mask edges, exact Euclidean distance transforms, surface-distance statistics,
all on the device) and each of its ops, timed with HIP events; scipy.ndimage.distance_transform_edt on the host beside them.

    python tools/bench_metrics.py [--reps 20] [--warmup 3] [--host-channels 3] [--no-trace] [--out profiles/metrics.txt]

Case: a 3-channel 240 x 240 x 155 mask pair (a BraTS prediction and its ground truth): the nested-ellipsoid targets of
synthetic.synthetic_case, and the same moved by (2, -1, 3) voxels. Spacing (1, 1, 1), percentile 95.
  per op:     median of --reps calls between HIP events, and the bytes the op MUST move (each input read once, each output written once)
              divided by that time -- what the passes move on top is in the notes.
  per kernel: one `rocprofv3 --kernel-trace --stats` run of its own over a few calls (a fresh child process: --child).
  host:       scipy.ndimage.distance_transform_edt per channel, wall clock, one call each; skipped with a note when scipy is absent."""
import argparse
import csv
import glob
import importlib
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
metrics = importlib.import_module("3dunetcnn_amd.metrics")
ops = importlib.import_module("3dunetcnn_amd.ops")
syn = importlib.import_module("3dunetcnn_amd.synthetic")
C, DHW = 3, (240, 240, 155)
NOTES = {"seg_counts_kernel": "read 2", "mask_edges_kernel": "read 1 (+ 6 neighbours from cache), write 1",
         "edt_x_kernel": "read 1 twice, write 4, read 4, write 4", "edt_line_kernel": "read 4 x ceil(L / 128) chunks, write 4",
         "surf_stats_kernel": "read 2 (+ 4 at edge voxels)", "surf_hist_kernel": "read 2 (+ 4 at edge voxels)",
         "surf_pick_kernel": "256 bins", "surf_final_kernel": "partials in index order", "zero_words_kernel": "clears counters / scratch"}


def make_pair(seed=0):
    truth = syn.synthetic_case(1, 1, DHW, C, seed)[1][0].to(torch.uint8)
    pred = torch.roll(truth, (2, -1, 3), dims=(1, 2, 3))
    return pred.contiguous(), truth.contiguous()


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


def child():
    pred, truth = (t.cuda() for t in make_pair())
    for _ in range(3):
        metrics.evaluate(pred, truth)
    torch.cuda.synchronize()


def kernel_trace(lines):
    exe = shutil.which("rocprofv3")
    if not exe:
        lines.append("per-kernel times: rocprofv3 not found, skipped")
        return
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "-f", "csv", "-d", td, "-o", "mt", "--", sys.executable, os.path.abspath(__file__),
                            "--child"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            lines.append(f"per-kernel times: rocprofv3 run failed (exit {r.returncode}), skipped")
            return
        rows = list(csv.DictReader(open(files[0])))
    lines.append("per kernel (rocprofv3 --kernel-trace --stats, 3 evaluate calls): calls, average ms, share, bytes per voxel")
    for row in rows:
        name = row["Name"].split("(")[0].replace("void ", "")
        if name in NOTES:
            lines.append(f"  {name:20s} {int(row['Calls']):4d} {float(row['AverageNs']) / 1e6:9.3f} ms {float(row['Percentage']):6.2f} %   {NOTES[name]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-channels", type=int, default=C)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics.txt"))
    args = ap.parse_args()
    if args.child:
        return child()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed calls")
    be = ops.default_backend()
    pred_h, truth_h = make_pair()
    pred, truth = pred_h.cuda(), truth_h.cuda()
    vox = C * DHW[0] * DHW[1] * DHW[2]
    ea, eb = be.mask_edges(pred), be.mask_edges(truth)
    to_b, to_a = be.edt(eb, sqrt=False), be.edt(ea, sqrt=False)
    ev = metrics.evaluate(pred, truth)
    n_edge = int(ev.edge_counts.sum())
    lines = [f"tools/bench_metrics.py on {torch.cuda.get_device_name(0)}: {C} x {DHW[0]} x {DHW[1]} x {DHW[2]} mask pair ({vox / 1e6:.1f} M voxels, "
             f"{n_edge} edge voxels), spacing (1, 1, 1), percentile 95",
             f"  dice {[round(v, 4) for v in ev.dice.tolist()]}, hausdorff {ev.hausdorff.tolist()}, hd95 {[round(v, 4) for v in ev.hausdorff_percentile.tolist()]}, "
             f"asd {[round(v, 4) for v in ev.average_surface_distance.tolist()]}"]
    # (op, call, compulsory bytes)
    rows = (("evaluate (20 launches)", lambda: metrics.evaluate(pred, truth), vox * 2),
            ("seg_counts", lambda: be.seg_counts(pred, truth), vox * 2),
            ("mask_edges", lambda: be.mask_edges(pred), vox * 2),
            ("edt (x, y, z passes)", lambda: be.edt(eb, sqrt=False), vox * (1 + 4)),
            ("surface_stats (10 launches)", lambda: be.surface_stats(ea, eb, to_b, to_a, 95.0), vox * 2 + n_edge * 4))
    for name, fn, byts in rows:
        med, lo, hi = timed(fn, args.reps, args.warmup)
        lines.append(f"  {name:28s} median {med:8.3f} ms of {args.reps} [min {lo:.3f}, max {hi:.3f}]; must move {byts / 1e6:7.1f} MB = "
                     f"{byts / (med * 1e-3) / 1e12:.3f} TB/s")
        print(lines[-1], flush=True)
    lines.append(f"  the three edt passes move 1 + 4, 4 + 4 and 4 + 4 bytes per voxel between them ({vox * 21 / 1e6:.0f} MB) and evaluate "
                 f"{(DHW[1] + DHW[0]) * vox / 1e9:.2f} G line candidates per transform")
    try:
        import scipy.ndimage as ndi
    except Exception:  # noqa: BLE001
        ndi = None
    if ndi is None:
        lines.append("  host: scipy is not installed here, skipped")
    else:
        host = []
        for c in range(min(C, args.host_channels)):
            m = eb[c].cpu().numpy() == 0
            t0 = time.perf_counter()
            ref = ndi.distance_transform_edt(m)
            host.append((time.perf_counter() - t0) * 1e3)
            same = bool(torch.equal(torch.from_numpy(ref ** 2).round().float(), to_b[c].cpu()))
            lines.append(f"  host scipy.ndimage.distance_transform_edt, channel {c}: {host[-1]:.0f} ms; squared distances equal the device's: {same}")
        lines.append(f"  host total for {len(host)} channels of ONE of the two transforms: {sum(host):.0f} ms (evaluate needs two, plus the copies)")
    if not args.no_trace:
        kernel_trace(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
