"""Developer tool (GPU): the two kernels of csrc/permute.hip (signed axis permutation; its inverse fused with the activation and the running
mean) and the permutation ensembles built on them, each timed with HIP events against the torch chain it replaces, in the same run.

    python tools/bench_permute.py [--reps 20] [--warmup 3] [--out profiles/permute.txt]

Cases: a 4 x 128^3 fp32 input batch and 3 x 128^3 fp32 logits (one sample of the benchmark's workload).
  stream rate  a device-to-device copy of the input (read 4, write 4 bytes per voxel), median of --reps.
  permute      a W-preserving key (all three flips: rows reversed), a W-preserving key that turns D and H, two W-moving keys (H <-> W,
               D <-> W), fp32; the W-moving key on uint8 and bf16 as well. Bytes moved = one read + one write of the batch; GB/s = that
               over the median. The torch chain = the key as torch.rot90 / flip / transpose calls and the final .contiguous().
  fold         mi355_unpermute_accumulate per activation, init = 0, W-preserving and W-moving: one read of the logits, one read and one
               write of the accumulator. The torch chain = activation, the inverse chain, acc.add_(p, alpha = 1 / K).
  ensemble     PermutationEnsemble over the 8 mirror keys and all 48 keys around an identity predictor, softmax, against the same loop
               written with torch calls (chain, softmax, inverse chain, add_; the division folded into alpha)."""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
permute = importlib.import_module("3dunetcnn_amd.permute")
ops = importlib.import_module("3dunetcnn_amd.ops")
EDGE = 128


def chain(x, key):
    (rx, ry, rz), fx, fy, fz, transpose = key
    if rx:
        x = torch.rot90(x, rx, dims=(3, 4))
    if ry:
        x = torch.rot90(x, ry, dims=(2, 4))
    if rz:
        x = torch.rot90(x, rz, dims=(2, 3))
    for on, axis in ((fx, 2), (fy, 3), (fz, 4)):
        if on:
            x = torch.flip(x, dims=(axis,))
    if transpose:
        x = x.transpose(3, 4)
    return x.contiguous()


def unchain(y, key):
    (rx, ry, rz), fx, fy, fz, transpose = key
    if transpose:
        y = y.transpose(3, 4)
    for on, axis in ((fz, 4), (fy, 3), (fx, 2)):
        if on:
            y = torch.flip(y, dims=(axis,))
    if rz:
        y = torch.rot90(y, -rz, dims=(2, 3))
    if ry:
        y = torch.rot90(y, -ry, dims=(2, 4))
    if rx:
        y = torch.rot90(y, -rx, dims=(3, 4))
    return y


def activate(y, activation):
    return torch.sigmoid(y) if activation == "sigmoid" else (torch.softmax(y, dim=1) if activation == "softmax" else y)


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
    return statistics.median(a.elapsed_time(b) for a, b in evs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permute.txt"))
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps: at least 20 timed calls")
    be = ops.default_backend()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, EDGE, EDGE, EDGE, generator=g).cuda()
    logits = (torch.randn(1, 3, EDGE, EDGE, EDGE, generator=g) * 2).cuda()
    lines = [f"tools/bench_permute.py on {torch.cuda.get_device_name(0)}: input 4 x {EDGE}^3 fp32 ({x.numel() * 4 / 1e6:.1f} MB), logits 3 x {EDGE}^3 fp32 "
             f"({logits.numel() * 4 / 1e6:.1f} MB); median of {args.reps} calls between HIP events after {args.warmup} warm-up calls"]

    def say(text):
        lines.append(text)
        print(text, flush=True)

    y = torch.empty_like(x)
    med = timed(lambda: y.copy_(x), args.reps, args.warmup)
    say(f"stream rate (device copy, {x.numel() * 8 / 1e6:.0f} MB moved): {med:.4f} ms = {x.numel() * 8 / med / 1e6:.0f} GB/s")

    keys = (("W kept, rows reversed (flip D, H, W)", ((0, 0, 0), 1, 1, 1, 0)), ("W kept, D and H turned", ((0, 0, 1), 0, 0, 0, 0)),
            ("W moves (H <-> W turn)", ((1, 0, 0), 0, 0, 0, 0)), ("W moves (D <-> W turn, flips, transpose)", ((0, 1, 0), 1, 0, 1, 1)))
    rates = {}
    say("permute_data, 4 x 128^3:")
    for dtype in (torch.float32, torch.bfloat16, torch.uint8):
        xd = x.to(dtype) if dtype != torch.uint8 else (x * 40).to(torch.uint8)
        moved = xd.numel() * xd.element_size() * 2
        for name, key in keys if dtype == torch.float32 else keys[::2]:
            assert torch.equal(permute.permute_data(xd, key), chain(xd, key))
            ours = timed(lambda: permute.permute_data(xd, key), args.reps, args.warmup)
            theirs = timed(lambda: chain(xd, key), args.reps, args.warmup)
            rates[(dtype, name)] = moved / ours / 1e6
            say(f"  {str(dtype)[6:]:9s}{name:42s} {ours:7.4f} ms = {moved / ours / 1e6:5.0f} GB/s ({moved / 1e6:.0f} MB moved); torch chain {theirs:7.4f} ms "
                f"({theirs / ours:4.1f} x)")
    slow, fast = rates[(torch.float32, keys[2][0])], rates[(torch.float32, keys[0][0])]
    say(f"  fp32: W-moving / W-preserving rate = {slow / fast:.2f}")

    say("unpermute_accumulate, 3 x 128^3 fp32 logits onto an fp32 accumulator, init = 0 (3 passes of 25.2 MB = 75.5 MB moved):")
    acc = torch.zeros_like(logits)
    moved = logits.numel() * 4 * 3
    for name, key in keys[::2]:
        code = [permute.key_code(key)]
        src = chain(logits, key)
        for activation in (None, "sigmoid", "softmax"):
            def theirs_fn():
                acc.add_(unchain(activate(src, activation), key), alpha=0.125)
            ours = timed(lambda: be.unpermute_accumulate(src, code, acc, activation, 0.125, init=False), args.reps, args.warmup)
            theirs = timed(theirs_fn, args.reps, args.warmup)
            say(f"  {name:42s} {str(activation):8s} {ours:7.4f} ms = {moved / ours / 1e6:5.0f} GB/s; torch chain {theirs:7.4f} ms ({theirs / ours:4.1f} x)")
        half = src.to(torch.bfloat16)
        ours = timed(lambda: be.unpermute_accumulate(half, code, acc, "softmax", 0.125, init=False), args.reps, args.warmup)
        say(f"  {name:42s} softmax, bf16 logits {ours:7.4f} ms = {logits.numel() * 10 / ours / 1e6:5.0f} GB/s ({logits.numel() * 10 / 1e6:.1f} MB moved)")

    say("ensembles around an identity predictor on the 3 x 128^3 logits, softmax:")
    for which in ("flips", "all"):
        ens = permute.PermutationEnsemble(lambda t: t, which, "softmax")
        k = len(ens.keys)

        def theirs_fn():
            total = torch.zeros_like(logits)
            for key in ens.keys:
                total.add_(unchain(torch.softmax(chain(logits, key), dim=1), key), alpha=1.0 / k)
            return total
        assert float((ens(logits) - theirs_fn()).abs().max()) < 1e-5
        ours = timed(lambda: ens(logits), args.reps, args.warmup)
        theirs = timed(theirs_fn, args.reps, args.warmup)
        moved = logits.numel() * 4 * (2 * k + 3 * k - 1)                # per key: permute read + write, fold read + acc read + write (the first: no read)
        say(f"  {k:2d} keys: {ours:8.4f} ms ({2 * k} launches) = {moved / ours / 1e6:5.0f} GB/s over {moved / 1e6:.0f} MB; torch chain {theirs:8.4f} ms "
            f"({theirs / ours:4.1f} x)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
