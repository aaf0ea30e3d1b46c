"""Developer tool (GPU): prepost.finish_prediction (ensemble mean + threshold + connected components + largest component, all on the
device) against the host route it replaces, timed in the same run, alternating.

    python tools/bench_components.py [--reps 20] [--warmup 3] [--host-reps 4] [--no-trace] [--out profiles/components.txt]

Cases: 5 models x 3 x 240 x 240 x 155 (a BraTS prediction) and 5 models x 1 x 192^3 (the sppin shape); probabilities whose mean
thresholds to the nested-ellipsoid targets of synthetic.synthetic_case with 2 % salt-and-pepper flips (thousands of islands).
  device route: finish_prediction on device tensors, HIP events around every call.
  host route:   device-to-host copy of the probabilities, np.mean, >= threshold, scipy.ndimage.label + np.bincount + compare per channel,
                host-to-device copy of the mask (wall clock between synchronisations); skipped with a note when scipy is absent.
  per kernel:   one `rocprofv3 --kernel-trace --stats` run of its own over a few calls (a fresh child process: --child).
Compulsory bytes of the whole call: read M * 4 B and write 1 B per voxel (+ 4 B for the mean); what the passes move on top is printed."""
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

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
prepost = importlib.import_module("3dunetcnn_amd.prepost")
syn = importlib.import_module("3dunetcnn_amd.synthetic")
CASES = {"brats 5x3x240x240x155": (5, 3, (240, 240, 155)), "sppin 5x1x192^3": (5, 1, (192, 192, 192))}
# bytes per voxel of each pass (labels int32, mask uint8, sizes touched at roots only)
PASSES = (("ensemble_threshold_kernel", "read M*4, write 4 + 1"), ("cc_local_kernel", "read 1, write 4"),
          ("cc_merge_kernel", "read 4 (tile-surface voxels: their neighbours too), atomics on roots"), ("cc_flatten_kernel", "read 4 + chain, write 4"),
          ("cc_roots_kernel", "read 4"), ("cc_sizes_kernel", "read 4, one atomic per (workgroup, component)"),
          ("cc_select_kernel", "read 4"), ("cc_write_kernel", "read 4 + 1 + size of the root, write 1"))


def make_probs(m, c, dhw, seed=0):
    g = torch.Generator().manual_seed(seed)
    mask = syn.synthetic_case(1, 1, dhw, c, seed)[1][0] ^ (torch.rand(c, *dhw, generator=g) < 0.02).to(torch.uint8)
    p = torch.empty(m, c, *dhw)
    for i in range(m):
        p[i] = 0.2 + 0.6 * mask + 0.15 * (torch.rand(c, *dhw, generator=g) - 0.5)
    return p


def host_route(pd, threshold=0.5):
    import scipy.ndimage as ndi
    p = pd.cpu().numpy()
    mean = np.mean(p, axis=0)
    mask = mean >= threshold
    out = np.zeros(mask.shape, dtype=np.uint8)
    for c in range(mask.shape[0]):
        lab, n = ndi.label(mask[c])
        if n:
            out[c] = lab == (np.bincount(lab.ravel())[1:].argmax() + 1)
    return torch.from_numpy(out).to(pd.device)


def child():
    for m, c, dhw in CASES.values():
        pd = make_probs(m, c, dhw).cuda()
        for _ in range(3):
            prepost.finish_prediction(pd)
        torch.cuda.synchronize()
        del pd


def kernel_trace(lines):
    exe = shutil.which("rocprofv3")
    if not exe:
        lines.append("per-kernel times: rocprofv3 not found, skipped")
        return
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "-f", "csv", "-d", td, "-o", "cc", "--", sys.executable, os.path.abspath(__file__),
                            "--child"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            lines.append(f"per-kernel times: rocprofv3 run failed (exit {r.returncode}), skipped")
            return
        rows = list(csv.DictReader(open(files[0])))
    note = dict(PASSES)
    lines.append("per kernel (rocprofv3 --kernel-trace --stats, 3 calls per case, both cases together): calls, average ms, share, bytes per voxel")
    for row in rows:
        name = row["Name"].split("(")[0].replace("void ", "")
        if name in note:
            lines.append(f"  {name:28s} {int(row['Calls']):4d} {float(row['AverageNs']) / 1e6:9.3f} ms {float(row['Percentage']):6.2f} %   {note[name]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=4)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components.txt"))
    args = ap.parse_args()
    if args.child:
        return child()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed calls")
    try:
        import scipy.ndimage  # noqa: F401
        have_scipy = True
    except Exception:  # noqa: BLE001
        have_scipy = False
    lines = [f"tools/bench_components.py on {torch.cuda.get_device_name(0)}: finish_prediction (threshold 0.5, faces, keep largest)"]
    for name, (m, c, dhw) in CASES.items():
        pd = make_probs(m, c, dhw).cuda()
        vox = c * dhw[0] * dhw[1] * dhw[2]
        for _ in range(args.warmup):
            out = prepost.finish_prediction(pd)
        torch.cuda.synchronize()
        dev_ms, host_ms, same = [], [], None
        every = max(1, args.reps // max(1, args.host_reps))
        evs = []
        for i in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = prepost.finish_prediction(pd)
            e1.record()
            evs.append((e0, e1))
            if have_scipy and i % every == 0 and len(host_ms) < args.host_reps:       # alternating with the device route
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                href = host_route(pd)
                torch.cuda.synchronize()
                host_ms.append((time.perf_counter() - t0) * 1e3)
                same = bool(torch.equal(href, out[1]))
        torch.cuda.synchronize()
        dev_ms = [a.elapsed_time(b) for a, b in evs]
        med = statistics.median(dev_ms)
        compulsory = vox * (m * 4 + 4 + 1)
        lines.append(f"{name}: {vox / 1e6:.1f} M voxels, kept {int(out[1].sum())} of {int((pd.mean(dim=0) >= 0.5).sum())} foreground voxels")
        lines.append(f"  device route: median {med:.3f} ms of {len(dev_ms)} [min {min(dev_ms):.3f}, max {max(dev_ms):.3f}]; compulsory bytes "
                     f"{compulsory / 1e6:.0f} MB ({m * 4 + 5} B per voxel) = {compulsory / (med * 1e-3) / 1e12:.2f} TB/s if nothing else moved")
        if have_scipy:
            hm = statistics.median(host_ms)
            lines.append(f"  host route:   median {hm:.1f} ms of {len(host_ms)} [min {min(host_ms):.1f}, max {max(host_ms):.1f}]; same mask: {same}; "
                         f"device route x{hm / med:.0f} faster; slowest device call {'<' if max(dev_ms) < min(host_ms) else '>='} fastest host call")
        else:
            lines.append("  host route:   scipy is not installed here, skipped")
        print("\n".join(lines[-3:]), flush=True)
        del pd, out
    if not args.no_trace:
        kernel_trace(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
