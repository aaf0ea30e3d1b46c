"""HipDynUNet: drop-in for MONAI `DynUNet` as the reference's shipped configs select it
(examples/brats2020/brats2020_config.json:2-107 -> unet3d/models/build.py:9-13 via `from monai.networks.nets import *`,
unet3d/models/pytorch/__init__.py:1). MONAI is an un-vendored, unpinned dependency of the reference (requirements.txt:4)
and is not installed here: the structure below follows SURVEY.md section 8a-B / appendix D (MONAI >= 1.2 `DynUNet`,
`UnetBasicBlock`, `UnetUpBlock`, `UnetOutBlock`), parity is against the plain-torch restatement oracle/dynunet_ref.py
("parity unpinned": no MONAI golden vectors exist in the reference).

  UnetBasicBlock(ci, co, s): Conv3d(k3, stride s, pad 1, no bias) -> InstanceNorm3d(affine) -> LeakyReLU(0.01), twice
  UnetUpBlock(ci, co):       ConvTranspose3d(k2, s2, no bias) -> cat((up, skip), 1) -> UnetBasicBlock(2co, co, 1)
  UnetOutBlock:              Conv3d(filters[0] -> out_channels, k1, bias)
  res_block=True [MONAI-memory]: every UnetBasicBlock above is a UnetResBlock(ci, co, s):
      out = lrelu(norm1(conv1(x))); out = norm2(conv2(out)); res = norm3(conv3(x)); out = lrelu(out + res)
      conv3 = Conv3d(k1, stride s, no bias), present when ci != co or s != 1 (every block of a DynUNet but an input block with
      in_channels == filters[0], whose identity shortcut is refused here)

MI355X execution: every conv writes its RAW output; InstanceNorm statistics are one streaming pass (mi355_gn_stats with
G == C) and the normalise + affine + LeakyReLU is applied by the CONSUMER while it stages its LDS tile (conv prologue), so
normalised tensors never exist in HBM. The skip-concat is a channel slice of one buffer: [0, co) = raw transposed-conv output
(identity prologue: scale 1, shift 0, slope 1), [co, 2co) = the encoder block's raw output with its own norm prologue.
Residual mode: a block's output is a function of two raw tensors with two sets of statistics, which no prologue expresses, so it is
MATERIALISED: A = lrelu(sc2 r2 + sh2 + sc3 r3 + sh3) in one pass (csrc/res_block.hip, mi355_res_join_fwd), written straight into the
encoder half of the concat buffer; every consumer (next block, transposed conv, projection, deep-supervision head) reads it IN_PLAIN and
the concat buffer needs no per-half prologue vectors. Backward: mi355_res_join_bwd turns dA into d_r2 (in place) and d_r3 with both norms'
parameter gradients in two passes; the stride-2 shortcut is mi355_conv1x1_s2_{fwd,wgrad,dgrad_add}, the stride-1 one the 1x1x1 conv.
ConvTranspose3d(k2, s2) is ONE 1x1x1 GEMM with 8*co logical output channels whose epilogue scatters depth-to-space
(MI355_OUT_D2S); its dgrad / wgrad read the fine gradient through the space-to-depth view (MI355_IN_S2D / OUT_D2S).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._lib import IN_AFFINE_ACT, IN_PLAIN, IN_S2D, IN_ZERO_INSERT, OUT_D2S
from .engine import HipNetBase

IN_EPS = 1e-5
SLOPE = 0.01


def _all_equal(v, val):
    if isinstance(v, (list, tuple)):
        return all(_all_equal(e, val) for e in v)
    return v == val


# ---- parameter holders (MONAI attribute names; never called) ------------------------------------------------------------
class _Conv(nn.Module):
    """monai Convolution(conv_only=True): a Sequential whose only member is `conv`."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv


class _BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = _Conv(nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False))
        self.conv2 = _Conv(nn.Conv3d(cout, cout, 3, stride=1, padding=1, bias=False))
        self.norm1 = nn.InstanceNorm3d(cout, affine=True)
        self.norm2 = nn.InstanceNorm3d(cout, affine=True)
        self.stride = stride


class _ResBlock(nn.Module):
    """monai UnetResBlock with cin != cout or stride != 1 (registration order: conv1, conv2, norm1, norm2, conv3, norm3). [MONAI-memory]"""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = _Conv(nn.Conv3d(cin, cout, 3, stride=stride, padding=1, bias=False))
        self.conv2 = _Conv(nn.Conv3d(cout, cout, 3, stride=1, padding=1, bias=False))
        self.norm1 = nn.InstanceNorm3d(cout, affine=True)
        self.norm2 = nn.InstanceNorm3d(cout, affine=True)
        self.conv3 = _Conv(nn.Conv3d(cin, cout, 1, stride=stride, bias=False))
        self.norm3 = nn.InstanceNorm3d(cout, affine=True)
        self.stride = stride


class _UpBlock(nn.Module):
    def __init__(self, cin, cout, block=_BasicBlock):
        super().__init__()
        self.transp_conv = _Conv(nn.ConvTranspose3d(cin, cout, 2, stride=2, bias=False))
        self.conv_block = block(2 * cout, cout, 1)


class _OutBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = _Conv(nn.Conv3d(cin, cout, 1, bias=True))


class _In:
    """A block input: Act + optional lazy prologue (per-(n,c) scale/shift, scalar or per-channel slope)."""
    __slots__ = ("act", "scale", "shift", "slope_vec")

    def __init__(self, act, scale=None, shift=None, slope_vec=None):
        self.act, self.scale, self.shift, self.slope_vec = act, scale, shift, slope_vec

    def kw(self):
        if self.scale is None:
            return dict(in_mode=IN_PLAIN)
        return dict(in_mode=IN_AFFINE_ACT, scale=self.scale, shift=self.shift, slope=SLOPE, in_slope=self.slope_vec)


def _tw_fwd(w):
    """ConvTranspose3d weight [ci, co, 2,2,2] -> 1x1x1 GEMM weight [(p, co), ci, 1,1,1], p = 4a+2b+e."""
    ci, co = w.shape[0], w.shape[1]
    return w.permute(2, 3, 4, 1, 0).reshape(8 * co, ci, 1, 1, 1)


class HipDynUNet(HipNetBase):
    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size, strides, upsample_kernel_size, filters=None,
                 dropout=None, norm_name=("INSTANCE", {"affine": True}),
                 act_name=("leakyrelu", {"inplace": True, "negative_slope": 0.01}), deep_supervision=False, deep_supr_num=1,
                 res_block=False, trans_bias=False):
        super().__init__()
        bad = []
        if spatial_dims != 3:
            bad.append("spatial_dims != 3")
        if not _all_equal(kernel_size, 3):
            bad.append("kernel_size != 3")
        if not (_all_equal(strides[0], 1) and _all_equal(list(strides[1:]), 2)):
            bad.append("strides other than [1, 2, 2, ...]")
        if not _all_equal(upsample_kernel_size, 2) or len(upsample_kernel_size) != len(strides) - 1:
            bad.append("upsample_kernel_size other than 2 per level")
        if deep_supervision:
            bad.append("deep_supervision=True")
        if dropout is not None:
            bad.append("dropout")
        if trans_bias:
            bad.append("trans_bias=True")
        nn_ = norm_name[0] if isinstance(norm_name, (tuple, list)) else norm_name
        if str(nn_).lower() != "instance" or (isinstance(norm_name, (tuple, list)) and not norm_name[1].get("affine", False)):
            bad.append("norm other than InstanceNorm(affine=True)")
        an = act_name[0] if isinstance(act_name, (tuple, list)) else act_name
        if str(an).lower() != "leakyrelu" or (isinstance(act_name, (tuple, list)) and act_name[1].get("negative_slope", 0.01) != 0.01):
            bad.append("activation other than LeakyReLU(0.01)")
        if bad:
            raise NotImplementedError("HipDynUNet implements the configuration the reference ships (brats2020_config.json); "
                                      "unsupported: " + ", ".join(bad)
                                      + (" (deep supervision: HipDynUNetDS, same arguments)" if deep_supervision else ""))
        L = len(strides)
        if filters is None:
            filters = [min(2 ** (5 + i), 320) for i in range(L)]     # MONAI default for spatial_dims == 3
        filters = list(filters)[:L]
        if len(filters) != L or any(f % 4 for f in filters) or out_channels > 8 or filters[0] > 96:
            raise NotImplementedError("filters must be multiples of 4, one per level; out_channels <= 8; filters[0] <= 96")
        self.spatial_dims, self.in_channels, self.out_channels = spatial_dims, in_channels, out_channels
        self.kernel_size, self.strides, self.upsample_kernel_size = kernel_size, strides, upsample_kernel_size
        self.filters = filters
        self.deep_supervision = False
        self.res_block = bool(res_block)
        if self.res_block and in_channels == filters[0]:
            raise NotImplementedError("res_block=True with in_channels == filters[0]: the input block's shortcut is then the identity "
                                      "(UnetResBlock without conv3 / norm3), which is not implemented")
        if self.res_block and max(filters) > 384:
            raise NotImplementedError("res_block=True: the 1x1x1 stride-2 shortcut convolution takes at most 384 channels (filters <= 384)")
        block = _ResBlock if self.res_block else _BasicBlock
        # registration order == MONAI's (state_dict key order)
        self.input_block = block(in_channels, filters[0], 1)
        self.downsamples = nn.ModuleList(block(filters[i - 1], filters[i], 2) for i in range(1, L - 1))
        self.bottleneck = block(filters[-2], filters[-1], 2)
        self.upsamples = nn.ModuleList(_UpBlock(filters[L - 1 - k], filters[L - 2 - k], block) for k in range(L - 1))
        self.output_block = _OutBlock(filters[0], out_channels)
        self.deep_supervision_heads = nn.ModuleList()
        # DynUNet.initialize_weights: kaiming_normal_(a=0.01) on conv / transposed-conv weights, zero biases
        for m in self.modules():
            if isinstance(m, (nn.Conv3d, nn.ConvTranspose3d)):
                nn.init.kaiming_normal_(m.weight, a=0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.n_in_channels = in_channels
        self._init_engine()

    # MONAI registers the same blocks a second time under `skip_layers.*`: DynUNet.__init__ ends with
    #   self.skip_layers = create_skips(0, [input_block] + downsamples, upsamples[::-1], bottleneck)
    # a chain of DynUNetSkipLayer(downsample, next_layer, upsample) modules (attributes registered in that order) whose innermost
    # `next_layer` is the bottleneck block itself. nn.Module.state_dict() does not de-duplicate shared modules, so a MONAI checkpoint
    # carries every encoder / decoder tensor twice: under its own name and under the alias. Emitting the aliases (same tensors, MONAI's
    # order: after output_block) makes a HipDynUNet checkpoint load into MONAI's DynUNet with strict=True; loading accepts and ignores
    # them. [MONAI-memory: the class is not importable here; the key names follow SURVEY.md 8a-b5 / MONAI's dynunet.py.]
    def _skip_layer_aliases(self):
        L = len(self.filters)
        downs = [("input_block", self.input_block)] + [(f"downsamples.{i}", m) for i, m in enumerate(self.downsamples)]
        ups = [(f"upsamples.{k}", m) for k, m in enumerate(self.upsamples)][::-1]
        out = []

        def walk(prefix, depth):
            if depth == L - 1:
                out.append((prefix, "bottleneck"))
                return
            out.append((prefix + ".downsample", downs[depth][0]))
            walk(prefix + ".next_layer", depth + 1)
            out.append((prefix + ".upsample", ups[depth][0]))
            if 1 <= depth <= len(self.deep_supervision_heads):        # DynUNetSkipLayer.super_head: the head of this depth (HipDynUNetDS)
                out.append((prefix + ".super_head", f"deep_supervision_heads.{depth - 1}"))
        walk("skip_layers", 0)
        return out                                   # [(alias prefix, canonical prefix)]

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        sd = super().state_dict(*args, destination=destination, prefix=prefix, keep_vars=keep_vars)
        own = [k for k in sd.keys() if k.startswith(prefix)]
        for alias, canon in self._skip_layer_aliases():
            for k in own:
                if k.startswith(prefix + canon + "."):
                    sd[prefix + alias + k[len(prefix + canon):]] = sd[k]
        return sd

    def load_state_dict(self, state_dict, strict=True, **kw):
        sd = {k: v for k, v in state_dict.items() if not k.startswith("skip_layers.")}
        return super().load_state_dict(sd, strict=strict, **kw)

    def forward(self, x):
        return self._run(x)

    def _supervised(self):
        """Heads this forward evaluates (HipDynUNetDS in training mode); 0: the logits alone."""
        return 0

    def _prepare_dout(self, dout):
        """The stacked output's gradient [N, 1 + K, ...] in the order of the buffer the forward wrote, [1 + K][N]...: no copy when it
        already has that order (HipDeepSupervisionLoss returns it so), one otherwise."""
        if dout.dim() == 6:
            return dout.transpose(0, 1).contiguous()
        return dout.contiguous()

    # ---- forward -------------------------------------------------------------------------------------------------------
    def _blocks(self):
        return [self.input_block] + list(self.downsamples) + [self.bottleneck]

    @staticmethod
    def _ci_pad(blk, cin):
        """Weight transform for a block whose input Act carries more channels than conv1 has (the network input, zero-padded to a
        multiple of 4 channels because NDHWC rows are float4 multiples): zero input-channel columns."""
        pad = cin - blk.conv1.conv.in_channels
        return None if pad == 0 else (lambda w: F.pad(w, (0, 0, 0, 0, 0, 0, 0, pad)))

    def _block_fwd(self, be, blk, xin, dst, keep):
        if self.res_block:
            return self._res_block_fwd(be, blk, xin, dst, keep)
        n = xin.act.shape[0]
        cout = blk.norm1.num_features
        d, h, w = dst.shape[1:4]
        r1 = be.empty_act(n, d, h, w, cout)
        # InstanceNorm statistics are not passes over r1 / dst: each conv's epilogue leaves the moment records of what it wrote
        # (csrc/gn_fuse.h) and gn_stats finalises those
        be.conv_fwd(xin.act, self._packed_weight(blk.conv1.conv.weight, 0, self._ci_pad(blk, xin.act.c)), r1, 3, blk.stride, moments=True,
                    **xin.kw())
        st1 = be.gn_stats(r1, cout, IN_EPS, blk.norm1.weight.data, blk.norm1.bias.data)
        r1.mom = None
        be.conv_fwd(r1, self._packed_weight(blk.conv2.conv.weight, 0), dst, 3, 1, in_mode=IN_AFFINE_ACT, scale=st1[1], shift=st1[2],
                    slope=SLOPE, moments=True)
        st2 = be.gn_stats(dst, cout, IN_EPS, blk.norm2.weight.data, blk.norm2.bias.data)
        dst.mom = None
        out = _In(dst, st2[1], st2[2])
        return dict(xin=xin, r1=r1, st1=st1, r2=dst, st2=st2, out=out) if keep else dict(out=out)

    def _res_block_fwd(self, be, blk, xin, dst, keep):
        """UnetResBlock: xin is PLAIN (a materialised A, the network input, or the concat buffer); dst receives A."""
        x = xin.act
        n, cout = x.shape[0], blk.norm1.num_features
        d, h, w = dst.shape[1:4]
        r1 = be.empty_act(n, d, h, w, cout)
        be.conv_fwd(x, self._packed_weight(blk.conv1.conv.weight, 0, self._ci_pad(blk, x.c)), r1, 3, blk.stride, moments=True)
        st1 = be.gn_stats(r1, cout, IN_EPS, blk.norm1.weight.data, blk.norm1.bias.data)
        r1.mom = None
        r2 = be.empty_act(n, d, h, w, cout)
        be.conv_fwd(r1, self._packed_weight(blk.conv2.conv.weight, 0), r2, 3, 1, in_mode=IN_AFFINE_ACT, scale=st1[1], shift=st1[2],
                    slope=SLOPE, moments=True)
        st2 = be.gn_stats(r2, cout, IN_EPS, blk.norm2.weight.data, blk.norm2.bias.data)
        r2.mom = None
        # the shortcut reads the block input in the activations' storage type (the fp32 network input of a 16-bit network: one small cast)
        x3 = x if x.dtype == r1.dtype else be.cast(x, r1.dtype)
        r3 = be.empty_act(n, d, h, w, cout)
        w3 = blk.conv3.conv.weight
        if blk.stride == 2:
            be.conv1x1_s2_fwd(x3, w3.data, r3)
            be.moments(r3)                      # r3 has 1/8 of the input's voxels: its statistics are one standalone pass
        else:
            be.conv_fwd(x3, self._packed_weight(w3, 0, self._ci_pad(blk, x.c)), r3, 1, moments=True)
        st3 = be.gn_stats(r3, cout, IN_EPS, blk.norm3.weight.data, blk.norm3.bias.data)
        r3.mom = None
        be.res_join_fwd(r2, st2, r3, st3, dst, SLOPE)
        out = _In(dst)
        return dict(xin=xin, x3=x3, r1=r1, st1=st1, r2=r2, st2=st2, r3=r3, st3=st3, out=out) if keep else dict(out=out)

    def _forward_impl(self, x, keep):
        be = self._begin_forward()
        n, _, D, H, W = x.shape
        f, L = self.filters, len(self.filters)
        sizes = [(D, H, W)]
        for _ in range(L - 1):
            if any(s % 2 for s in sizes[-1]):
                raise ValueError(f"HipDynUNet: spatial size {tuple(x.shape[2:])} must be divisible by {2 ** (L - 1)} "
                                 "(ConvTranspose3d(k2,s2) output must match the skip, as in MONAI DynUNet)")
            sizes.append(tuple(s // 2 for s in sizes[-1]))
        cpad = (self.in_channels + 3) // 4 * 4
        # the network input stays fp32 when it has the first-layer kernels' 4 channels (they read fp32 and store either type), as in
        # HipUNet3D; wider inputs are stored like every other activation
        xa_dtype = torch.float32 if cpad == 4 else be.act_dtype
        if cpad == self.in_channels:
            xa = be.empty_act(n, D, H, W, self.in_channels, dtype=xa_dtype)
            be.ncdhw_to_ndhwc(x, xa)
        else:
            xa = be.zeros_act(n, D, H, W, cpad, dtype=xa_dtype)
            be.ncdhw_to_ndhwc(x, xa.slice(0, self.in_channels))
        cats = [be.empty_act(n, *sizes[i], 2 * f[i]) for i in range(L - 1)]
        enc = []
        cur = _In(xa)
        for i, blk in enumerate(self._blocks()):
            dst = cats[i].slice(f[i], f[i]) if i < L - 1 else be.empty_act(n, *sizes[i], f[i])
            s = self._block_fwd(be, blk, cur, dst, keep)
            enc.append(s)
            cur = s["out"]
        ups = []
        ones = zeros = None
        # deep supervision: the logits and the K head outputs are slots of one buffer [1 + K][N][C][D][H][W]
        K = self._supervised()
        stack = torch.empty(1 + K, n, self.out_channels, D, H, W, dtype=torch.float32, device=x.device) if K else None
        for k, up in enumerate(self.upsamples):
            lvl = L - 2 - k
            co = f[lvl]
            cat = cats[lvl]
            be.conv_fwd(cur.act, self._packed_weight(up.transp_conv.conv.weight, 0, _tw_fwd), cat.slice(0, co), 1, out_mode=OUT_D2S,
                        **cur.kw())
            if self.res_block:                 # both halves are plain: the raw transposed conv and the encoder's materialised A
                cin_ = _In(cat)
            else:
                sk = enc[lvl]["out"]
                ones = torch.ones(n, co, dtype=torch.float32, device=be.device)
                zeros = torch.zeros(n, co, dtype=torch.float32, device=be.device)
                sc = torch.cat((ones, sk.scale), 1).contiguous()
                sh = torch.cat((zeros, sk.shift), 1).contiguous()
                sl = torch.cat((ones[0], torch.full((co,), SLOPE, dtype=torch.float32, device=be.device))).contiguous()
                cin_ = _In(cat, sc, sh, sl)
            dst = be.empty_act(n, *sizes[lvl], co)
            s = self._block_fwd(be, up.conv_block, cin_, dst, keep)
            s["tin"] = cur
            ups.append(s)
            cur = s["out"]
            if 1 <= lvl <= K:                 # head lvl - 1 reads this level's activated output: raw + its norm prologue, or the plain A
                hd = self.deep_supervision_heads[lvl - 1].conv.conv
                be.ds_head_fwd(cur.act, hd.weight.data.reshape(self.out_channels, -1), hd.bias.data, stack[lvl], 2 ** lvl, cur.scale, cur.shift,
                               SLOPE)
        logits = stack[0] if K else torch.empty(n, self.out_channels, D, H, W, dtype=torch.float32, device=x.device)
        ob = self.output_block.conv.conv
        be.proj_fwd(cur.act, ob.weight.data.reshape(self.out_channels, -1), ob.bias.data, logits, cur.scale, cur.shift, SLOPE)
        self._end_forward()
        saved = dict(enc=enc, ups=ups, sizes=sizes, n=n, last=cur, heads=K) if keep else None
        return (stack.transpose(0, 1) if K else logits), saved       # [N, 1 + K, C, D, H, W]: every out[:, l] contiguous

    # ---- backward ------------------------------------------------------------------------------------------------------
    def _block_bwd(self, be, blk, s, dA2, need_dx, dx_residual=None):
        """dA2: gradient wrt the block's ACTIVATED output (modified in place). Returns the gradient wrt the block's ACTIVATED
        input (Act) or None."""
        cout = blk.norm1.num_features
        r1, r2, st1, st2, xin = s["r1"], s["r2"], s["st1"], s["st2"], s["xin"]
        d_r3 = None
        if self.res_block:
            # join backward: d_r2 overwrites dA2, d_r3 is a tensor of its own; both norms' parameter gradients
            d_r3 = be.empty_act(*r2.shape)
            be.res_join_bwd(s["out"].act, dA2, r2, st2, blk.norm2.weight.data, s["r3"], s["st3"], blk.norm3.weight.data, dA2, d_r3,
                            self._gslice(blk.norm2.weight), self._gslice(blk.norm2.bias), self._gslice(blk.norm3.weight),
                            self._gslice(blk.norm3.bias), SLOPE)
        else:
            be.gn_act_bwd(r2, dA2, dA2, cout, SLOPE, blk.norm2.weight.data, st2[0], st2[1], st2[2],
                          self._gslice(blk.norm2.weight), self._gslice(blk.norm2.bias))
        d_r2 = dA2
        with self._wgrad_stream(be, r1, d_r2, st1[1], st1[2]):
            be.conv_wgrad(r1, d_r2, self._gslice(blk.conv2.conv.weight), 3, 1, in_mode=IN_AFFINE_ACT, scale=st1[1], shift=st1[2], slope=SLOPE)
        dA1 = be.empty_act(*r1.shape)
        # the dgrad's epilogue also leaves the first pass of the norm backward (sum du, sum du*xhat per tile)
        p1 = be.conv_fwd(d_r2, self._packed_weight(blk.conv2.conv.weight, 1), dA1, 3, 1, gnb=(r1, st1, cout, SLOPE))
        be.gn_act_bwd(r1, dA1, dA1, cout, SLOPE, blk.norm1.weight.data, st1[0], st1[1], st1[2],
                      self._gslice(blk.norm1.weight), self._gslice(blk.norm1.bias), partials=p1)
        d_r1 = dA1
        w1 = blk.conv1.conv.weight
        with self._wgrad_stream(be, xin.act, d_r1, xin.scale, xin.shift, xin.slope_vec):
            if xin.act.c == w1.shape[1]:
                be.conv_wgrad(xin.act, d_r1, self._gslice(w1), 3, blk.stride, **xin.kw())
            else:                                  # zero-padded network input: wgrad over the padded channels, sliced back
                tw = torch.empty(w1.shape[0], xin.act.c, 3, 3, 3, dtype=torch.float32, device=w1.device)
                be.conv_wgrad(xin.act, d_r1, tw, 3, blk.stride, **xin.kw())
                self._gslice(w1).copy_(tw[:, :w1.shape[1]])
        if d_r3 is not None:
            x3, w3 = s["x3"], blk.conv3.conv.weight
            with self._wgrad_stream(be, x3, d_r3):
                if blk.stride == 2:
                    be.conv1x1_s2_wgrad(x3, d_r3, self._gslice(w3))
                elif x3.c == w3.shape[1]:
                    be.conv_wgrad(x3, d_r3, self._gslice(w3), 1, 1)
                else:                              # zero-padded network input, as for conv1
                    tw = torch.empty(w3.shape[0], x3.c, 1, 1, 1, dtype=torch.float32, device=w3.device)
                    be.conv_wgrad(x3, d_r3, tw, 1, 1)
                    self._gslice(w3).copy_(tw[:, :w3.shape[1]])
        self._flush_ready()
        if not need_dx:
            return None
        n, d, h, w, cin = xin.act.shape
        dAin = be.empty_act(n, d, h, w, cin, dtype=xin.act.dtype)          # a tensor's gradient is stored like the tensor
        wp = self._packed_weight(blk.conv1.conv.weight, 1, self._ci_pad(blk, cin))
        if blk.stride == 1:
            if d_r3 is not None:
                # stride-1 shortcut (input block, decoder blocks: no skip gradient arrives here): its dgrad is the 1x1x1 conv, carried into
                # conv1's dgrad through the residual epilogue
                assert dx_residual is None
                dx_residual = be.empty_act(n, d, h, w, cin, dtype=d_r3.dtype)
                be.conv_fwd(d_r3, self._packed_weight(blk.conv3.conv.weight, 1, self._ci_pad(blk, cin)), dx_residual, 1)
                if dx_residual.dtype != dAin.dtype:
                    dx_residual = be.cast(dx_residual, dAin.dtype)
            be.conv_fwd(d_r1, wp, dAin, 3, 1, residual=dx_residual)
        else:
            be.conv_fwd(d_r1, wp, dAin, 3, 1, pad=1, in_mode=IN_ZERO_INSERT, residual=dx_residual, out_dhw=(d, h, w))
            if d_r3 is not None:                   # after conv1's dgrad has written dAin: one voxel in eight gets the shortcut's share added
                be.conv1x1_s2_dgrad_add(d_r3, blk.conv3.conv.weight.data, dAin)
        return dAin

    def _backward_impl_body(self, be, saved, dlogits, need_dx):
        f, L = self.filters, len(self.filters)
        enc, ups, n = saved["enc"], saved["ups"], saved["n"]
        last = saved["last"]
        K = saved["heads"]
        dstack = dlogits if K else None      # [1 + K][N][C][D][H][W] (_prepare_dout)
        if K:
            dlogits = dstack[0]
        for head in self.deep_supervision_heads[K:]:
            # heads this forward did not evaluate (eval mode with grad): no kernel writes their slices of the persistent gradient
            # buffer, which would otherwise still hold an earlier step's values. Their gradient is zero, as autograd's is for MONAI's
            hd = head.conv.conv
            self._gslice(hd.weight).zero_()
            self._gslice(hd.bias).zero_()
        ob = self.output_block.conv.conv
        dA = be.empty_act(*last.act.shape)
        be.proj_bwd(last.act, ob.weight.data.reshape(self.out_channels, -1), dlogits, dA,
                    self._gslice(ob.weight).view(self.out_channels, -1), self._gslice(ob.bias), last.scale, last.shift, SLOPE)
        d_skip = [None] * (L - 1)
        for k in range(L - 2, -1, -1):
            lvl = L - 2 - k
            co = f[lvl]
            up = self.upsamples[k]
            s = ups[k]
            if 1 <= lvl <= K:
                # dA holds the gradient from the finer up block; the head adds its own before this level's norm backward consumes the sum.
                # On the launch stream, not the weight-gradient side stream: the kernel that writes dw / dbias is the one that adds to dA
                hd = self.deep_supervision_heads[lvl - 1].conv.conv
                o = s["out"]
                be.ds_head_bwd(o.act, hd.weight.data.reshape(self.out_channels, -1), dstack[lvl], dA,
                               self._gslice(hd.weight).view(self.out_channels, -1), self._gslice(hd.bias), 2 ** lvl, o.scale, o.shift, SLOPE)
            dcat = self._block_bwd(be, up.conv_block, s, dA, True)
            d_up, d_skip[lvl] = dcat.slice(0, co), dcat.slice(co, co)
            tin = s["tin"]                                  # activated input of the transposed conv (raw + prologue)
            w = up.transp_conv.conv.weight
            cin = w.shape[0]
            with self._wgrad_stream(be, tin.act, d_up, tin.scale, tin.shift, tin.slope_vec):
                dw1 = torch.empty(8 * co, cin, dtype=torch.float32, device=be.device)
                be.conv_wgrad(tin.act, d_up, dw1, 1, out_mode=OUT_D2S, **tin.kw())
                self._gslice(w).copy_(dw1.view(2, 2, 2, co, cin).permute(4, 3, 0, 1, 2))
            dA = be.empty_act(*tin.act.shape)
            be.conv_fwd(d_up, self._packed_weight(w, 1, _tw_fwd), dA, 1, in_mode=IN_S2D)
            self._flush_ready()
        blocks = self._blocks()
        dx = None
        for i in range(L - 1, -1, -1):
            need = need_dx or i > 0
            dA = self._block_bwd(be, blocks[i], enc[i], dA, need, d_skip[i - 1] if i > 0 else None)
            if i == 0:
                dx = dA
        dx_t = None
        if need_dx and dx is not None:
            sizes = saved["sizes"]
            dx_t = torch.empty(n, self.in_channels, *sizes[0], dtype=torch.float32, device=dlogits.device)
            be.ndhwc_to_ncdhw(dx.slice(0, self.in_channels), dx_t)
        return dx_t


class HipDynUNetDS(HipDynUNet):
    """HipDynUNet with MONAI's deep supervision (the nnU-Net training form). [MONAI-memory, parity unpinned: MONAI is not installed here
    and the reference holds no fixture for the model; the structure follows MONAI >= 1.2 `dynunet.py` as restated in
    tests/deep_supervision_cases.py, like oracle/dynunet_ref.py for the plain model.]

      deep_supervision_heads = ModuleList(UnetOutBlock(filters[i + 1], out_channels) for i in range(deep_supr_num)),
                               1 <= deep_supr_num < len(strides) - 1; kaiming_normal_(a=0.01) weights, zero biases
      head i reads the activated output of the up block at level i + 1 (resolution input / 2^(i + 1))
      training mode: torch.stack([out] + [F.interpolate(head_i, out.shape[2:]) for i], dim=1)     -> [N, 1 + K, C, D, H, W]
                     (interpolation "nearest": source index floor(dst / 2^(i + 1)))
      eval mode:     `out` alone; the heads are not evaluated
      state dict:    deep_supervision_heads.{i}.conv.conv.{weight,bias} after output_block.*; each DynUNetSkipLayer of depth i + 1 registers
                     the same module again as `super_head` (after downsample, next_layer, upsample)

    With deep_supervision=False this is HipDynUNet. MI355X execution: the logits and the K head outputs are slots of ONE buffer
    [1 + K][N][C][D][H][W], returned as its transpose(0, 1) view; slot 0 is written by mi355_proj_fwd, slot 1 + i by mi355_ds_head_fwd
    (projection + nearest up-sampling in one launch, csrc/deep_supervision.hip). Backward: mi355_ds_head_bwd pools the slot's gradient,
    writes the head's dw / dbias and adds wT dz to the level's gradient before that level's norm backward reads it. Pair it with
    losses.HipDeepSupervisionLoss, which returns its gradient in the buffer's order (no copy)."""

    def __init__(self, spatial_dims, in_channels, out_channels, kernel_size, strides, upsample_kernel_size, filters=None,
                 dropout=None, norm_name=("INSTANCE", {"affine": True}),
                 act_name=("leakyrelu", {"inplace": True, "negative_slope": 0.01}), deep_supervision=False, deep_supr_num=1,
                 res_block=False, trans_bias=False):
        super().__init__(spatial_dims, in_channels, out_channels, kernel_size, strides, upsample_kernel_size, filters=filters, dropout=dropout,
                         norm_name=norm_name, act_name=act_name, deep_supervision=False, deep_supr_num=deep_supr_num, res_block=res_block,
                         trans_bias=trans_bias)
        self.deep_supr_num = deep_supr_num
        if not deep_supervision:
            return
        L = len(self.filters)
        if not 1 <= deep_supr_num < L - 1:             # MONAI: "deep_supr_num should be less than the number of up sample layers."
            raise ValueError(f"deep_supr_num should be at least 1 and less than the number of up sample layers ({L - 1}), got {deep_supr_num}")
        if any(self.filters[i + 1] > 320 for i in range(deep_supr_num)):
            raise NotImplementedError("deep-supervision heads read at most 320 channels (filters[1 .. deep_supr_num] <= 320)")
        self.deep_supervision = True
        for i in range(deep_supr_num):
            head = _OutBlock(self.filters[i + 1], out_channels)
            nn.init.kaiming_normal_(head.conv.conv.weight, a=0.01)
            nn.init.constant_(head.conv.conv.bias, 0)
            self.deep_supervision_heads.append(head)

    def _supervised(self):
        return self.deep_supr_num if self.deep_supervision and self.training else 0

    def forward(self, x):
        K = self._supervised()
        if K and x.dim() == 5 and x.shape[0] == 0:
            self._check_input(x)                       # empty batch: the matching empty stack, linked to the parameters (engine._run)
            return x.new_zeros((0, 1 + K, self.out_channels) + tuple(x.shape[2:])) + sum(p.sum() * 0 for p in self._params())
        return self._run(x)
