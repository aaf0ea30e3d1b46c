"""TEST INFRASTRUCTURE (oracle) -- generates tests/golden/unet3d_small.pt by importing and running the REFERENCE's own
UNet3D from /root/reference (build container only; see oracle/reference_shim.py). Commit the output.

    python oracle/make_golden.py

Contents: constructor kwargs, the reference's state_dict under seed 1234, a synthetic input/target,
the reference's logits (eval mode: Dropout3d off, myronenko.py:70-79), sigmoid-Dice loss (oracle/torch_ops.py) and every
parameter gradient -- fp32 CPU.
"""
import importlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import reference_shim, torch_ops, unet3d_ref  # noqa: E402


def make(path, kwargs, dhw, n):
    model = reference_shim.build_reference_unet3d(seed=1234, **kwargs).eval()
    x, y = unet3d_ref.synthetic_case(n, kwargs["n_features"], dhw, kwargs["n_outputs"], seed=0)
    logits = model(x)
    loss = torch_ops.dice_loss(logits, y)
    loss.backward()
    bundle = {
        "kwargs": kwargs, "state_dict": {k: v.detach().clone() for k, v in model.state_dict().items()},
        "x": x, "y": y, "logits": logits.detach(), "loss": loss.detach(),
        "grads": {k: p.grad.detach().clone() for k, p in model.named_parameters()},
        "generator": "oracle/make_golden.py: reference unet3d.models.pytorch.segmentation.unet.UNet3D, torch "
                     + torch.__version__ + " CPU fp32",
    }
    torch.save(bundle, path)
    print(path, os.path.getsize(path) // 1024, "KiB; loss", float(loss))


def make_autocast(path, bundle_path):
    """The reference's UNet3D graph (same weights and input as `bundle_path`) under torch.autocast -- what its AutocastUNet
    (models/pytorch/segmentation/unet.py:53-58) adds around UNet3D.forward. The class itself enters torch.cuda.amp.autocast, which
    is a no-op without a CUDA device, so the context is entered here for the CPU device type with the two 16-bit dtypes: convolutions run
    on fp16 / bf16 operands and return that dtype, the norms run in fp32 (torch's autocast policy, the same op lists as on CUDA)."""
    b = torch.load(bundle_path)
    model = reference_shim.build_reference_unet3d(seed=1234, **b["kwargs"]).eval()
    model.load_state_dict(b["state_dict"])
    out = {"kwargs": b["kwargs"], "bundle": os.path.basename(bundle_path),
           "generator": "oracle/make_golden.py: reference UNet3D under torch.autocast('cpu', dtype), torch " + torch.__version__}
    with torch.no_grad():
        ref = model(b["x"])
        for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            with torch.autocast("cpu", dtype=dt):
                o = model(b["x"])
            out["logits_" + name] = o.float()
            print(name, "max rel. difference to the fp32 logits:", float((o.float() - ref).abs().max() / ref.abs().max()))
    torch.save(out, path)
    print(path, os.path.getsize(path) // 1024, "KiB")


# The checks tests/ used to run against the imported reference, recorded once (tests/golden/reference_checks.pt): the suite then needs
# nothing outside the repository. The cases are the ones the tests name; the tests assert the same conditions on the recorded values.
LIVE_CASES = [(dict(n_features=4, n_outputs=3, base_width=8), (16, 16, 16)),
              (dict(n_features=4, n_outputs=3, base_width=8, encoder_blocks=[1, 1, 2], use_transposed_convolutions=True), (12, 16, 8)),
              (dict(n_features=4, n_outputs=3, base_width=8, encoder_blocks=[1, 2, 1]), (15, 13, 10))]     # odd sizes: crop path
INIT_CASES = [dict(n_features=4, n_outputs=3), dict(n_features=4, n_outputs=3, use_transposed_convolutions=True),
              dict(n_features=4, n_outputs=3, base_width=16, encoder_blocks=[1, 2, 2, 2, 4])]
TILE_KW = dict(n_features=4, n_outputs=3, base_width=8, encoder_blocks=[1, 1, 1])          # tests/test_boundary.py KW


# Floating-point results are kept as a fixed seeded sample of their elements plus whole-tensor summaries (max |x|, sum |x|, L2 norm);
# results that must match bit for bit (initialisations, checkpoints, integer label maps) as sha256 digests. The fixture stays small.
GRAD_SAMPLE = 32
LOGIT_SAMPLE = 1024


def sample_index(numel, k):
    """The elements of a flattened tensor a fixture keeps: all of a small tensor, else a fixed seeded k of them (ascending)."""
    if numel <= k:
        return torch.arange(numel)
    return torch.randperm(numel, generator=torch.Generator().manual_seed(0))[:k].sort().values


def summary(t):
    """float64 [max |x|, sum |x|, L2 norm] of the whole tensor."""
    t = t.detach().double().reshape(-1)
    return torch.tensor([float(t.abs().max()), float(t.abs().sum()), float(t.norm())], dtype=torch.float64)


def sampled(t, k):
    """{sample at sample_index(numel, k), summary}."""
    flat = t.detach().reshape(-1)
    return {"shape": tuple(t.shape), "sample": flat[sample_index(flat.numel(), k)].clone(), "summary": summary(flat)}


def key_digests(sd):
    """{key: the first 16 hex digits of its tensor's digest}, in key order: names the tensor that differs, at 64 bits per key."""
    return {k: torch_ops.tensor_digest(v)[:16] for k, v in sd.items()}


def state_dict_digest(sd):
    """One sha256 over a state_dict's keys (in order) and the digests of its tensors."""
    import hashlib
    return hashlib.sha256("".join(f"{k}={torch_ops.tensor_digest(v)};" for k, v in sd.items()).encode()).hexdigest()


def _reference_one_hot_module():
    reference_shim.import_reference_unet()
    if "monai.data" not in sys.modules:
        md = types.ModuleType("monai.data")

        class MetaTensor(torch.Tensor):        # minimal stand-in: a Tensor subclass that survives torch ops and has `.meta`
            meta = {}

            @staticmethod
            def __new__(cls, x, meta=None, **kw):
                return torch.Tensor._make_subclass(cls, x)
        md.MetaTensor = MetaTensor
        sys.modules["monai.data"] = md
        sys.modules["monai"].data = md
    return importlib.import_module("unet3d.utils.one_hot")


def make_reference_checks(path):
    unet = importlib.import_module("3dunetcnn_amd.unet")
    out = {"generator": "oracle/make_golden.py make_reference_checks: the reference's UNet3D, unet3d.utils.one_hot and "
                        "unet3d.models.build, torch " + torch.__version__ + " CPU fp32"}
    # tests/test_oracle_pinned.py test_oracle_matches_live_reference: logits and parameter gradients of the reference at seed 11
    live = []
    for kw, dhw in LIVE_CASES:
        ref = reference_shim.build_reference_unet3d(seed=11, **kw).eval()
        x, y = unet3d_ref.synthetic_case(2, 4, dhw)
        want = ref(x)
        torch_ops.dice_loss(want, y).backward()
        keys = [k for k, p in ref.named_parameters()]
        grads = [sampled(p.grad, GRAD_SAMPLE) for _, p in ref.named_parameters()]
        live.append({"kwargs": kw, "dhw": dhw, "state_dict_sha256": state_dict_digest(ref.state_dict()), "logits": sampled(want, LOGIT_SAMPLE),
                     "grad_keys": keys, "grad_samples": torch.cat([g["sample"] for g in grads]),
                     "grad_summaries": torch.stack([g["summary"] for g in grads])})
    out["live_cases"] = live
    # test_state_dict_contract_and_same_seed_init: the reference's state_dict keys (in order), shapes, dtypes and default init at seed 1234
    out["init_cases"] = []
    for kw in INIT_CASES:
        sd = reference_shim.build_reference_unet3d(seed=1234, **kw).state_dict()
        out["init_cases"].append({"kwargs": kw, "sha256": key_digests(sd)})      # keys in order; a digest covers dtype, shape and values
    # tests/test_input_channels.py test_empty_batch_matches_reference_behaviour: the reference's output shape on an empty batch
    ref = reference_shim.build_reference_unet3d(n_features=4, n_outputs=3, base_width=8, encoder_blocks=[1, 1]).eval()
    out["empty_batch_logits_shape"] = tuple(ref(torch.zeros(0, 4, 8, 8, 8)).shape)
    # tests/test_prepost.py test_oracle_matches_live_reference_functions: the reference's one-hot encode / decode on seeded inputs
    ref = _reference_one_hot_module()
    g = torch.Generator().manual_seed(0)
    lm = torch.randint(0, 5, (1, 1, 9, 8, 7), generator=g).float()
    enc = [(labels, ref.compile_one_hot_encoding(sys.modules["monai.data"].MetaTensor(lm), 3 if labels is None else len(labels),
                                                 labels=labels).as_subclass(torch.Tensor).clone())
           for labels in ([1, 2, 4], [[1, 2], [4]], None)]
    oh = torch.rand(3, 9, 8, 7, generator=g)
    dec = [(labels, kw, ref.convert_one_hot_to_label_map(oh, labels, **kw).clone())
           for labels, kw in (([2, 1, 4], dict(label_hierarchy=True)), ([2, 1, 4], dict()), ([2, 1, 4], dict(sum_then_threshold=True)),
                              ([2, 1, 4], dict(threshold=0.7)), ([[2, 1], [4]], dict()))]
    out["one_hot"] = {"label_map_sha256": torch_ops.tensor_digest(lm), "one_hot_sha256": torch_ops.tensor_digest(oh),
                      "encode": [(labels, torch_ops.tensor_digest(t)) for labels, t in enc],
                      "decode": [(labels, kw, torch_ops.tensor_digest(t)) for labels, kw, t in dec]}
    # tests/test_boundary.py test_reference_loader_tiles_a_narrower_checkpoint: the reference loader's match_state_dict_shapes applied to a
    # narrower HipUNet3D checkpoint (seed 3, half the input modalities and half the widths) for a TILE_KW model
    build = importlib.import_module("unet3d.models.build")
    torch.manual_seed(3)
    narrow = unet.HipUNet3D(**{**TILE_KW, "n_features": 2, "base_width": 4}).state_dict()
    tiled = build.match_state_dict_shapes(unet.HipUNet3D(**TILE_KW).state_dict(), {k: v.clone() for k, v in narrow.items()})
    out["tiled_checkpoint"] = {"kwargs": TILE_KW, "narrow_seed": 3, "narrow_sha256": state_dict_digest(narrow),
                               "tiled_sha256": key_digests(tiled)}
    torch.save(out, path)
    print(path, os.path.getsize(path) // 1024, "KiB")


def make_brats_config(path):
    """The `model` section of the reference's examples/brats2020/brats2020_config.json (the DynUNet configuration HipDynUNet takes)."""
    import json
    cfg = json.load(open(os.path.join(reference_shim.REFERENCE_ROOT, "examples", "brats2020", "brats2020_config.json")))
    with open(path, "w") as f:
        json.dump({"model": cfg["model"]}, f, indent=1)
        f.write("\n")
    print(path)


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden")
    os.makedirs(out, exist_ok=True)
    make(os.path.join(out, "unet3d_small.pt"), dict(n_features=4, n_outputs=3, base_width=8, encoder_blocks=[1, 2, 1]), (20, 16, 24), 2)
    make(os.path.join(out, "unet3d_small_transposed.pt"),
         dict(n_features=4, n_outputs=3, base_width=8, encoder_blocks=[1, 1, 1], use_transposed_convolutions=True), (16, 16, 16), 1)
    make_autocast(os.path.join(out, "unet3d_small_autocast.pt"), os.path.join(out, "unet3d_small.pt"))
    make_reference_checks(os.path.join(out, "reference_checks.pt"))
    make_brats_config(os.path.join(out, "brats2020_config_model.json"))
