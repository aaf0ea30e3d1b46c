"""Residual blocks (csrc/res_block.hip, HipDynUNet / HipDynUNetDS with res_block=True) on the CPU emulator of the same kernel sources, and
the host-side behaviour of the module. The cases and their criteria: tests/res_block_cases.py."""
import json
import os

import pytest
import torch

import deep_supervision_cases as DS
import res_block_cases as RB
import scratch_guard as G
import stream_form_cases as SF
import test_launch_audit as TLA
from oracle import unet3d_ref as R

dyn, losses = RB.dyn, RB.losses
BRATS = dict(in_channels=4, out_channels=3, spatial_dims=3, strides=[[1, 1, 1]] + [[2, 2, 2]] * 5, filters=[64, 96, 128, 192, 256, 384],
             kernel_size=[[3, 3, 3]] * 6, upsample_kernel_size=[[2, 2, 2]] * 5, res_block=True)   # examples/brats2020/brats2020_config.json + res_block
SMALL, DHW = [8, 12, 16], (8, 12, 8)
BLOCK_KEYS = ["conv1.conv.weight", "conv2.conv.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias", "conv3.conv.weight",
              "norm3.weight", "norm3.bias"]


# ---- the ops -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(RB.JOIN))
def test_join_against_float64(emu_backend, cid):
    RB.join_case(emu_backend, *RB.JOIN[cid])


@pytest.mark.parametrize("cid", sorted(RB.SHORTCUT))
def test_shortcut_conv_against_float64(emu_backend, cid):
    RB.shortcut_case(emu_backend, *RB.SHORTCUT[cid])


def test_the_shortcut_bound_is_the_conv_bound():
    assert RB.CONV_BOUND == TLA.BOUNDS["conv_fwd"] == TLA.BOUNDS["conv_wgrad"] and SF.BOUND == TLA.BOUNDS["gn_act_bwd"]


def test_launch_counts_and_kernel_forms(emu_backend):
    """One launch for the join forward, three for its backward (two streaming passes and the finalisation of the sums); one for the shortcut's
    forward and for dgrad_add, two for its weight gradient. 16-bit views with c % 8 == 0 take the 8-channel-per-lane kernels."""
    be = emu_backend
    SF.take(be)
    RB.join_case(be, *RB.JOIN["f32-c12-v33"])
    bwd = ["(res_join_bwd_partial_kernel<T, 4>)", "res_join_bwd_finalize_kernel", "(res_join_bwd_apply_kernel<T, 4>)"]
    assert SF.take(be) == ["(res_join_fwd_kernel<T, 4>)"] + bwd * 2
    RB.join_case(be, *RB.JOIN["f16-c16-v105"])
    assert SF.take(be) == [k.replace("T, 4", "T, 8") for k in ["(res_join_fwd_kernel<T, 4>)"] + bwd * 2]
    RB.shortcut_case(be, *RB.SHORTCUT["f32-4-8-v105"])
    assert SF.take(be) == ["(c1s2_gemm_kernel<T, 1>)"] + ["(c1s2_wgrad_kernel<T>)", "c1s2_wgrad_reduce_kernel", "(c1s2_gemm_kernel<T, 0>)"] * 2


def test_ops_refuse(emu_backend):
    RB.refusals(emu_backend)


# ---- constructor and state dict ------------------------------------------------------------------------------------------------------------
def test_reference_config_constructs_with_res_block():
    cfg = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brats2020_config_model.json")))["model"]
    assert cfg.pop("name") == "DynUNet"
    m = dyn.HipDynUNet(**dict(cfg, res_block=True))
    assert m.res_block and m.filters == [64, 96, 128, 192, 256, 384] and isinstance(m.bottleneck, dyn._ResBlock)
    assert not dyn.HipDynUNet(**cfg).res_block
    with pytest.raises(NotImplementedError, match="identity"):
        dyn.HipDynUNet(**dict(RB.kw([4, 8, 12])))                       # in_channels == filters[0]
    with pytest.raises(NotImplementedError, match="identity"):
        dyn.HipDynUNetDS(**dict(RB.kw([4, 8, 12], 1)))
    with pytest.raises(NotImplementedError, match="384"):
        dyn.HipDynUNet(**dict(RB.kw([8, 12, 388])))
    for refused in (dict(dropout=0.1), dict(trans_bias=True), dict(norm_name="batch"), dict(act_name="relu")):
        with pytest.raises(NotImplementedError):
            dyn.HipDynUNet(**dict(RB.kw(SMALL), **refused))
    with pytest.raises(RuntimeError, match="MI355X"):
        m(torch.randn(1, 4, 32, 32, 32))


def test_state_dict_layout():
    m = dyn.HipDynUNet(**BRATS)
    sd = m.state_dict()
    keys = list(sd)
    own = [k for k in keys if not k.startswith("skip_layers.")]
    blocks = (["input_block"] + [f"downsamples.{i}" for i in range(4)] + ["bottleneck"])
    want = [f"{b}.{k}" for b in blocks for k in BLOCK_KEYS]
    for k in range(5):
        want += [f"upsamples.{k}.transp_conv.conv.weight"] + [f"upsamples.{k}.conv_block.{b}" for b in BLOCK_KEYS]
    want += ["output_block.conv.conv.weight", "output_block.conv.conv.bias"]
    assert own == want
    assert sd["input_block.conv3.conv.weight"].shape == (64, 4, 1, 1, 1) and sd["bottleneck.conv3.conv.weight"].shape == (384, 256, 1, 1, 1)
    assert sd["upsamples.4.conv_block.conv3.conv.weight"].shape == (64, 128, 1, 1, 1) and sd["downsamples.0.norm3.bias"].shape == (96,)
    assert sd["downsamples.2.conv1.conv.weight"].shape == (192, 128, 3, 3, 3)
    assert sum(p.numel() for p in m.parameters()) == RB.restatement_parameter_count(4, 3, BRATS["filters"])
    plain = dyn.HipDynUNet(**dict(BRATS, res_block=False))
    extra = sum(v.numel() for k, v in sd.items() if not k.startswith("skip_layers.") and (".conv3." in k or ".norm3." in k))
    assert sum(p.numel() for p in m.parameters()) == sum(p.numel() for p in plain.parameters()) + extra
    # every tensor but the output block's is aliased exactly once under skip_layers.*, the same storage
    alias = keys[len(own):]
    assert all(k.startswith("skip_layers.") for k in alias) and len(alias) == len(own) - 2 and len(set(alias)) == len(alias)
    by_ptr = {}
    for k in alias:
        by_ptr.setdefault(sd[k].data_ptr(), []).append(k)
    for k in own[:-2]:
        assert len(by_ptr[sd[k].data_ptr()]) == 1, k
        assert by_ptr[sd[k].data_ptr()][0].endswith(k.split(".", 2 if k[0] in "du" else 1)[-1]) and sd[by_ptr[sd[k].data_ptr()][0]].shape == sd[k].shape
    nl = "skip_layers." + "next_layer." * 4
    for a, c in [("skip_layers.downsample.conv3.conv.weight", "input_block.conv3.conv.weight"),
                 ("skip_layers.next_layer.downsample.norm3.bias", "downsamples.0.norm3.bias"),
                 (nl + "next_layer.norm3.weight", "bottleneck.norm3.weight"),
                 ("skip_layers.upsample.conv_block.conv3.conv.weight", "upsamples.4.conv_block.conv3.conv.weight")]:
        assert sd[a].data_ptr() == sd[c].data_ptr(), (a, c)
    # strict round trips with and without the aliases
    other = dyn.HipDynUNet(**BRATS)
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), other.parameters()))
    other = dyn.HipDynUNet(**BRATS)
    other.load_state_dict({k: v for k, v in sd.items() if not k.startswith("skip_layers.")}, strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), other.parameters()))
    with pytest.raises(RuntimeError):
        plain.load_state_dict(sd, strict=True)
    # kaiming_normal_(a=0.01) reaches conv3 too: std = sqrt(2 / (1 + a^2) / fan_in), fan_in = cin of a 1x1x1 kernel
    w = sd["bottleneck.conv3.conv.weight"]
    assert abs(float(w.std()) / (2.0 / (1 + 1e-4) / 256) ** 0.5 - 1) < 0.1
    assert float(sd["bottleneck.norm3.weight"].min()) == 1.0 and float(sd["bottleneck.norm3.bias"].abs().max()) == 0.0


# ---- the network against the oracle --------------------------------------------------------------------------------------------------------
# Recorded on the emulator (`pytest -s` prints the dictionaries; n_loose describes the conditioning of the case and is not asserted):
#   [8, 12, 16] (8, 12, 8) batch 2: logits 7.3e-7, loss 0, grad 0.0021, n_loose 0, max_err_vs_fp32 2.9e-6 (device records: the GPU twin)
def test_emulated_network_fwd_bwd(emu_backend):
    torch.manual_seed(5)
    m = dyn.HipDynUNet(**RB.kw(SMALL)).eval()
    e = RB.pair(m, emu_backend, DHW, 2, "cpu")
    print("record", {k: e[k] for k in ("n_loose", "max_err_vs_fp32")}, e)
    assert e["logits"] < RB.TOL and e["loss"] < RB.TOL and e["grad"] <= 1.0, e
    assert e["max_err_vs_fp32"] < RB.TOL, e         # this small case is well conditioned: plain 1e-3 on every gradient


def test_emulated_network_with_heads_fwd_bwd(emu_backend):
    torch.manual_seed(5)
    m = dyn.HipDynUNetDS(**RB.kw(SMALL, 1)).train()
    assert m.res_block and m.deep_supervision
    e = RB.pair(m, emu_backend, DHW, 2, "cpu")
    print("record", {k: e[k] for k in ("n_loose", "max_err_vs_fp32")}, e)
    assert e["logits"] < RB.TOL and e["loss"] < RB.TOL and e["grad"] <= 1.0, e


def test_forward_launches_one_join_per_block_and_reads_plain(emu_backend):
    """Five blocks at three levels: five join launches each way, two stride-2 shortcuts; the inference forward (no grad) launches the same
    kernels and gives the same logits."""
    be = emu_backend
    torch.manual_seed(2)
    m = dyn.HipDynUNet(**RB.kw(SMALL)).train()
    crit = RB.make_criterion(0)
    DS.bind(be, m, crit)
    crit._be = be
    x, y = R.synthetic_case(1, 4, (4, 8, 4), 3)
    SF.take(be)
    out = m(x)
    fwd = SF.take(be)
    assert sum("res_join_fwd_kernel" in k for k in fwd) == 5 and sum("c1s2_gemm_kernel<T, 1>" in k for k in fwd) == 2
    crit(out, y).backward()
    bwd = SF.take(be)
    assert sum("res_join_bwd_apply_kernel" in k for k in bwd) == 5 and sum("c1s2_wgrad_kernel" in k for k in bwd) == 2
    assert sum("c1s2_gemm_kernel<T, 0>" in k for k in bwd) == 2 and not any("gn_bwd_partial_kernel" in k for k in bwd)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in m.parameters())
    with torch.no_grad():
        again = m(x)
    assert torch.equal(again, out.detach()) and [k for k in SF.take(be) if "res_join" in k or "c1s2" in k] == [k for k in fwd if "res_join" in k or "c1s2" in k]


def test_gradient_accumulation_and_grad_ready_callback(emu_backend):
    be = emu_backend
    torch.manual_seed(3)
    m = dyn.HipDynUNet(**RB.kw(SMALL)).train()
    crit = RB.make_criterion(0)
    DS.bind(be, m, crit)
    crit._be = be
    batches = [R.synthetic_case(1, 4, (4, 8, 4), 3, seed=s) for s in (0, 1)]
    single = []
    for x, y in batches:
        m.zero_grad(set_to_none=True)
        seen = []
        m.grad_ready_callback = seen.extend
        single.append(DS.train_step(m, crit, x, y)[1])
        assert sorted(id(p) for p in seen) == sorted(id(p) for p in m.parameters())
    m.grad_ready_callback = None
    m.zero_grad(set_to_none=True)
    for x, y in batches:
        crit(m(x), y).backward()
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, single[0][k] + single[1][k]), k


def test_16bit_activation_storage_runs(emu_backend):
    """bf16 operands with fp32 tensors next to bf16-stored activations: losses within 2e-3 (the bound of tests/test_act_storage_gpu.py),
    gradients finite, the backend left in its own mode."""
    x, y = R.synthetic_case(2, 4, DHW, 3)
    got = {}
    for storage in (None, torch.bfloat16):
        torch.manual_seed(5)
        m = dyn.HipDynUNet(**RB.kw(SMALL)).train()
        m.backward_side_stream = False
        m.conv_precision, m.act_storage = "bf16", storage
        crit = RB.make_criterion(0)
        DS.bind(emu_backend, m, crit)
        crit._be = emu_backend
        loss, grads = DS.train_step(m, crit, x, y)
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
        got[storage] = float(loss)
        assert emu_backend.act_dtype == torch.float32 and emu_backend.precision == 0
    print("record", got)
    assert abs(got[None] - got[torch.bfloat16]) < 2e-3, got


# ---- hostile memory ------------------------------------------------------------------------------------------------------------------------
HOSTILE = {"join": lambda be: RB.join_case(be, *RB.JOIN["bf16-c100-v33"]), "shortcut": lambda be: RB.shortcut_case(be, *RB.SHORTCUT["f32-12-16-v1"]),
           "step": lambda be: RB.step_case(be, "cpu")}


@pytest.mark.parametrize("rid", sorted(HOSTILE))
def test_on_hostile_memory(emu_backend, rid):
    assert G.hold(emu_backend, lambda: HOSTILE[rid](emu_backend), (G.QNAN, G.ONES)).results > 0
