"""``GRL`` -- drop-in replacement for the reference network at its own boundary.

Boundary: the reference engine does ``self.model = hydra.utils.instantiate(cfg.model)``
(engines/base.py:44) and then only calls ``model(x)``, ``parameters()``, ``state_dict()`` /
``load_state_dict(strict=True)`` and ``convert_checkpoint`` (tools/trainer.py:93-115).  This class
accepts the constructor arguments of ``models.networks.grl.GRL`` (grl.py:220-256, unknown YAML keys
swallowed like the reference does), owns parameters with the *same names and shapes*, and runs
the forward pass (grl.py:506-551) on MI355X through libgrl_hip.so.

There is no CPU / eager fallback for the hot path: calling the model on CPU tensors raises.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib as L
from . import autograd as AG
from . import forward_infer, forward_train, ops
from . import plan as P
from . import switches as SW
from .geometry import pad_multiple, to_2tuple


# ------------------------------------------------------------------------------------------------
# parameter containers (names mirror the reference so state_dicts are interchangeable)
# ------------------------------------------------------------------------------------------------
class _Affine(nn.Module):  # mixed_attn_block_efficient.py:23-34
    def __init__(self, nh):
        super().__init__()
        self.logit_scale = nn.Parameter(torch.log(10 * torch.ones((nh, 1, 1))))
        self.cpb_mlp = nn.Sequential(nn.Linear(2, 512, bias=True), nn.ReLU(inplace=True), nn.Linear(512, nh, bias=False))


class _Body(nn.Module):
    def __init__(self, body):
        super().__init__()
        self.body = body


class _AnchorLinear(nn.Module):  # mixed_attn_block.py:714-725
    def __init__(self, cin, cout):
        super().__init__()
        self.reduction = nn.Linear(cin, cout, bias=True)


class _WindowAttn(nn.Module):
    def __init__(self, nh):
        super().__init__()
        self.attn_transform = _Affine(nh)


class _StripeAttn(nn.Module):
    def __init__(self, nh):
        super().__init__()
        self.attn_transform1 = _Affine(nh)
        self.attn_transform2 = _Affine(nh)


class _MixedAttention(nn.Module):  # mixed_attn_block_efficient.py:317-349
    def __init__(self, dim, nh_w, nh_s):
        super().__init__()
        self.qkv = _Body(nn.Linear(dim, dim * 3, bias=True))
        self.anchor = _Body(nn.ModuleList([_AnchorLinear(dim, dim // 2)]))
        self.window_attn = _WindowAttn(nh_w)
        self.stripe_attn = _StripeAttn(nh_s)
        self.proj = nn.Linear(dim, dim)


class _ChannelAttention(nn.Module):  # mixed_attn_block.py:948-963
    def __init__(self, c, reduction):
        super().__init__()
        self.attention = nn.Sequential(
            nn.AdaptiveAvgPool2d(1), nn.Conv2d(c, c // reduction, 1, padding=0), nn.ReLU(inplace=True),
            nn.Conv2d(c // reduction, c, 1, padding=0), nn.Sigmoid(),
        )


class _CAB(nn.Module):  # mixed_attn_block.py:970-979
    def __init__(self, c, compress_ratio=4, reduction=18):
        super().__init__()
        self.cab = nn.Sequential(
            nn.Conv2d(c, c // compress_ratio, 3, 1, 1), nn.GELU(), nn.Conv2d(c // compress_ratio, c, 3, 1, 1),
            _ChannelAttention(c, reduction),
        )


class _Mlp(nn.Module):  # swin_v1_block.py:15-35
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(nn.Module):  # mixed_attn_block_efficient.py:406-508
    def __init__(self, dim, nh_w, nh_s, mlp_ratio, local_connection):
        super().__init__()
        self.attn = _MixedAttention(dim, nh_w, nh_s)
        self.norm1 = nn.LayerNorm(dim)
        if local_connection:
            self.conv = _CAB(dim)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))
        self.norm2 = nn.LayerNorm(dim)


class _Stage(nn.Module):  # grl.py:31-137
    def __init__(self, dim, depth, nh_w, nh_s, mlp_ratio, local_connection):
        super().__init__()
        self.blocks = nn.ModuleList([_Block(dim, nh_w, nh_s, mlp_ratio, local_connection) for _ in range(depth)])
        self.conv = nn.Conv2d(dim, dim, 3, 1, 1)


class _Up(nn.Module):  # upsample.py:6-50
    def __init__(self, mods):
        super().__init__()
        self.up = nn.Sequential(*mods)


_BUFFER_PREFIXES = ("table_", "index_", "mask_")


class GRL(nn.Module):
    """MI355X-native GRL.  Constructor signature of models/networks/grl.py:220-256."""

    def __init__(
        self,
        img_size=64,
        in_channels=3,
        out_channels=None,
        embed_dim=96,
        upscale=2,
        img_range=1.0,
        upsampler="",
        depths=[6, 6, 6, 6, 6, 6],
        num_heads_window=[3, 3, 3, 3, 3, 3],
        num_heads_stripe=[3, 3, 3, 3, 3, 3],
        window_size=8,
        stripe_size=[8, 8],
        stripe_groups=[None, None],
        stripe_shift=False,
        mlp_ratio=4.0,
        qkv_bias=True,
        qkv_proj_type="linear",
        anchor_proj_type="avgpool",
        anchor_one_stage=True,
        anchor_window_down_factor=1,
        out_proj_type="linear",
        local_connection=False,
        drop_rate=0.0,
        attn_drop_rate=0.0,
        drop_path_rate=0.1,
        norm_layer=nn.LayerNorm,
        pretrained_window_size=[0, 0],
        pretrained_stripe_size=[0, 0],
        conv_type="1conv",
        init_method="n",
        fairscale_checkpoint=False,
        offload_to_cpu=False,
        euclidean_dist=False,
        precision="auto",  # not a reference option: "fast" | "high" | "auto" (operand precision of the HIP path, see below)
        **kwargs,  # name, double_window, stripe_square, separable_conv_act, use_buffer, ... (swallowed, grl.py:255)
    ):
        super().__init__()
        unsupported = []
        if qkv_proj_type != "linear":
            unsupported.append(f"qkv_proj_type={qkv_proj_type!r}")
        if anchor_proj_type != "avgpool" or not anchor_one_stage:
            unsupported.append(f"anchor_proj_type={anchor_proj_type!r}/anchor_one_stage={anchor_one_stage}")
        if out_proj_type != "linear":
            unsupported.append(f"out_proj_type={out_proj_type!r}")
        if conv_type != "1conv":
            unsupported.append(f"conv_type={conv_type!r}")
        if euclidean_dist:
            unsupported.append("euclidean_dist=True")
        if not qkv_bias:
            unsupported.append("qkv_bias=False")
        if list(pretrained_window_size) != [0, 0] or list(pretrained_stripe_size) != [0, 0]:
            unsupported.append("pretrained_*_size != [0, 0]")
        if init_method not in ("n", "r", "l", "w") and init_method.find("t") < 0:
            unsupported.append(f"init_method={init_method!r}")
        if unsupported:
            raise NotImplementedError(
                "grl_image_restoration_amd.GRL implements the configurations the reference ships "
                "(config/model/grl/*.yaml); not supported: " + ", ".join(unsupported)
            )
        out_channels = out_channels or in_channels
        self.in_channels, self.out_channels = in_channels, out_channels
        self.embed_dim, self.upscale, self.upsampler, self.img_range = embed_dim, upscale, upsampler, img_range
        self.depths = list(depths)
        self.num_heads_window, self.num_heads_stripe = list(num_heads_window), list(num_heads_stripe)
        self.window_size = to_2tuple(window_size)
        self.stripe_size, self.stripe_groups = list(stripe_size), list(stripe_groups)
        self.stripe_shift = stripe_shift
        self.mlp_ratio = mlp_ratio
        self.df = anchor_window_down_factor
        self.local_connection = local_connection
        self.res_scale = 0.1 if init_method == "r" else 1.0
        self.input_resolution = to_2tuple(img_size)
        self.pad_size = pad_multiple(self.window_size[0], self.stripe_size, self.stripe_groups, self.df)
        # Operand precision of the linear / conv contractions (attention always runs on fp16 operands):
        #   fast : fp16 operands (2^-11 relative rounding), fused block-tail / register-resident / streaming kernels; per-site
        #          exceptions on split operands: conv_first always, the convolutions named in `split_sites`, and the q / k /
        #          anchor projection of blocks whose logit scale exceeds `hiq_scale`
        #   high : split operands a = hi + lo, w = hi + lo (3 MFMA terms, ~22 mantissa bits) everywhere, fp32 intermediates
        #   auto : (resolved per weight set, plan.resolve_precision: the narrow models switch to `high` at checkpoint-like logit scales)
        #          measured on the fixtures (max |err| against the reference, bar 1e-3; tests/test_gpu_model.py):
        #          GRL-Base SR                 fast                                    2.1e-4 (clamp-scale checkpoints 6.5e-4)
        #          GRL-Base deblur (no upsampler: y = x + conv_last(body), no smoothing tail)
        #                                      fast 1.16e-3 -> + stage/after/last convs split 1.0e-3 -> + CAB conv1 split 8.2e-4
        #                                      (with the q/k projection split instead: 7.8e-4, but 4.0 instead of 5.6 MP/s)
        #          GRL-Small denoise           fast 1.14e-3 -> + stage/after/last convs split 7.2e-4
        #          GRL-Small demosaic (8x8 windows, 32x32 stripes: the `dm` preset)
        #                                      fast + those splits 1.07e-3 -> calibrated (plan.calibrated_plan, 6 of 16 blocks split) 5.4e-4,
        #                                      +17 % time at 512x512; so narrow models with windows of 8 or less always calibrate
        #          GRL-Tiny                    high (fast + splits 6e-4 .. 8e-4, but 8e-3 at clamp scales)
        precision = SW.text("GRL_PRECISION", default=precision)
        if precision not in ("auto", "fast", "high"):
            raise ValueError(f"precision={precision!r}: expected 'auto', 'fast' or 'high'")
        narrow = embed_dim < 160 or not upsampler
        self._precision_arg, self._narrow = precision, narrow
        # (`auto` is resolved again whenever the packed weights are rebuilt, see plan.resolve_precision: it depends on the logit scales)
        self.precision = precision if precision != "auto" else ("high" if embed_dim < 100 else "fast")
        # fast mode: comma list of conv sites kept on split operands (see plan.build_plan); logit scale above which a block's q / k / anchor
        # planes come from the split-operand projection (0: always)
        # (a site may be given as `name:x` = only its activations split, two MFMA terms.  Tried as the default for the stage conv --
        # the per-operand emulation said its weights' rounding does not matter: deblur 384 8.3e-4 with both split, 8.0e-4 with x only,
        # 1.04e-3 with W only -- but measured on the GPU the fixtures moved from 8.2e-4 to 8.8e-4 (deblur) and from 7.2e-4 to 9.0e-4
        # (Small) for 4-5 % of a step: not kept, the margin to the 1e-3 bar is worth more.)
        self.split_sites = ("stage_conv,after,last,cab0" if embed_dim >= 160 else "stage_conv,after,last") if narrow else ""
        self.hiq_scale = SW.num("GRL_HIQ_SCALE")
        if embed_dim % 2 or any((embed_dim // 2) % h for h in self.num_heads_window + self.num_heads_stripe):
            raise ValueError("embed_dim/2 must be divisible by the number of heads")
        if max((embed_dim // 2) // h for h in self.num_heads_window + self.num_heads_stripe) > 32:
            raise NotImplementedError("head_dim > 32 is not supported by the gfx950 attention kernel")
        if in_channels == 3:
            mean = torch.tensor((0.4488, 0.4371, 0.4040)).view(1, 3, 1, 1)
        else:
            mean = torch.zeros(1, 1, 1, 1)
        self.register_buffer("_mean", mean, persistent=False)

        num_out_feats = 64
        self.conv_first = nn.Conv2d(in_channels, embed_dim, 3, 1, 1)
        self.norm_start = nn.LayerNorm(embed_dim)
        self.layers = nn.ModuleList(
            [
                _Stage(embed_dim, depths[i], num_heads_window[i], num_heads_stripe[i], mlp_ratio, local_connection)
                for i in range(len(depths))
            ]
        )
        self.norm_end = nn.LayerNorm(embed_dim)
        self.conv_after_body = nn.Conv2d(embed_dim, embed_dim, 3, 1, 1)
        if upsampler == "pixelshuffle":
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_out_feats, 3, 1, 1), nn.LeakyReLU(inplace=True))
            m = []
            if (upscale & (upscale - 1)) == 0:
                for _ in range(int(math.log(upscale, 2))):
                    m += [nn.Conv2d(num_out_feats, 4 * num_out_feats, 3, 1, 1), nn.PixelShuffle(2)]
            elif upscale == 3:
                m += [nn.Conv2d(num_out_feats, 9 * num_out_feats, 3, 1, 1), nn.PixelShuffle(3)]
            else:
                raise ValueError(f"scale {upscale} is not supported. Supported scales: 2^n and 3.")
            self.upsample = _Up(m)
            self.conv_last = nn.Conv2d(num_out_feats, out_channels, 3, 1, 1)
        elif upsampler == "pixelshuffledirect":
            self.upsample = _Up([nn.Conv2d(embed_dim, (upscale**2) * out_channels, 3, 1, 1), nn.PixelShuffle(upscale)])
        elif upsampler == "nearest+conv":
            assert upscale == 4, "only support x4 now."
            self.conv_before_upsample = nn.Sequential(nn.Conv2d(embed_dim, num_out_feats, 3, 1, 1), nn.LeakyReLU(inplace=True))
            self.conv_up1 = nn.Conv2d(num_out_feats, num_out_feats, 3, 1, 1)
            self.conv_up2 = nn.Conv2d(num_out_feats, num_out_feats, 3, 1, 1)
            self.conv_hr = nn.Conv2d(num_out_feats, num_out_feats, 3, 1, 1)
            self.conv_last = nn.Conv2d(num_out_feats, out_channels, 3, 1, 1)
        else:
            self.conv_last = nn.Conv2d(embed_dim, out_channels, 3, 1, 1)

        self.apply(self._init_weights)  # grl.py:381,455-469
        self._init_method_rescale(init_method)
        # stochastic depth decay rule (grl.py:299-300): block j of the whole network drops its branches with probability dpr[j]
        self.drop_path_rate = float(drop_path_rate)
        self._dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self._plan_cache = {}
        self._register_load_state_dict_pre_hook(self._drop_reference_buffers)
        # fires on the recursive path too (a parent module's load_state_dict, tools/trainer.py:108-111)
        self.register_load_state_dict_post_hook(lambda module, incompatible_keys: module.invalidate_plan())

    # ---- init / checkpoint contract ------------------------------------------------------------
    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _init_method_rescale(self, init_method):
        """TransformerStage._init_weights (grl.py:139-162) for the 'l' / 'w' / 't*' variants."""
        if not (init_method in ("l", "w") or init_method.find("t") >= 0):
            return
        for layer in self.layers:
            for n, m in layer.named_modules():
                if init_method == "w":
                    if isinstance(m, (nn.Linear, nn.Conv2d)) and n.find("cpb_mlp") < 0:
                        m.weight.data *= 0.1
                elif init_method == "l":
                    if isinstance(m, nn.LayerNorm):
                        nn.init.constant_(m.bias, 0)
                        nn.init.constant_(m.weight, 0)
                else:
                    scale = 0.1 ** (len(init_method) - 1) * int(init_method[-1])
                    if isinstance(m, nn.Linear) and n.find("cpb_mlp") < 0:
                        nn.init.trunc_normal_(m.weight, std=scale)
                    elif isinstance(m, nn.Conv2d):
                        m.weight.data *= 0.1

    @staticmethod
    def _drop_reference_buffers(state_dict, prefix, *args):
        """The reference keeps 13 table/index/mask buffers in its state_dict (grl.py:309-310) and never
        trusts them from disk (convert_checkpoint, grl.py:556-569).  This implementation needs none of
        them, so they are dropped on load to keep ``load_state_dict(strict=True)`` working."""
        for k in list(state_dict.keys()):
            if k[len(prefix):].startswith(_BUFFER_PREFIXES):
                state_dict.pop(k)

    def convert_checkpoint(self, state_dict):
        """grl.py:556-569: drop buffers that depend on the geometry from a Lightning checkpoint."""
        for k in list(state_dict.keys()):
            if (
                k.find("relative_coords_table") >= 0 or k.find("relative_position_index") >= 0
                or k.find("attn_mask") >= 0 or k.find("model.table_") >= 0 or k.find("model.index_") >= 0
                or k.find("model.mask_") >= 0
            ):
                state_dict.pop(k)
        return state_dict

    def invalidate_plan(self):
        """Drops the packed weights / tables (rebuilt lazily), every captured graph that points at them, the cached fp16
        training weights and the cached parameter list.  Called by the load_state_dict post-hook; in-place parameter updates
        through autograd-visible ops (optimizer steps, ``p.mul_()``, ``p.copy_()``) are caught by the version stamp in ``_plan``.
        NOT caught -- call this method yourself afterwards: updates through ``.data`` (``p.data.mul_()``, ``m.weight.data *= s``:
        torch does not bump the version counter for them) and parameters REPLACED by new tensors
        (``load_state_dict(assign=True)``, ``m.weight = nn.Parameter(...)``)."""
        self._plan_cache = {}
        self._plist = None
        if getattr(self, "_graphs", None):
            self._graphs = {}
        AG.forget_parameters(self)

    def _param_stamp(self):
        """Changes whenever a parameter is modified in place or replaced (torch bumps ``_version`` on every in-place op)."""
        plist = getattr(self, "_plist", None)
        if plist is None:
            plist = self._plist = list(self.parameters())
        return sum(p._version for p in plist)

    def train(self, mode: bool = True):
        if mode:
            self.invalidate_plan()
        return super().train(mode)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"absolute_pos_embed"}

    @torch.jit.ignore
    def no_weight_decay_keywords(self):
        return {"relative_position_bias_table"}

    # ---- plan cache (plan.py packs, forward_infer.py launches) ---------------------------------------
    def _plan(self, x_size, dev):
        key = (tuple(x_size), str(dev), self._param_stamp())
        plan = self._plan_cache.get(key)
        if plan is not None:
            return plan
        self._calibrate_narrow = False
        self.precision = P.resolve_precision(self)
        self.calibration = None
        if (self._precision_arg == "auto" and self.precision == "fast" and (not self._narrow or self._calibrate_narrow)
                and SW.on("GRL_CALIBRATE")):
            plan = P.calibrated_plan(self, x_size, dev, force=self._calibrate_narrow)
        else:
            plan = P.build_plan(self, x_size, dev, self.precision)
        self._plan_cache = {key: plan}  # one geometry at a time keeps memory bounded (captured graphs hold their own plan)
        return plan

    # ---- forward -------------------------------------------------------------------------------
    def check_image_size(self, x):
        """grl.py:479-489."""
        _, _, h, w = x.size()
        ph = (self.pad_size - h % self.pad_size) % self.pad_size
        pw = (self.pad_size - w % self.pad_size) % self.pad_size
        try:
            x = F.pad(x, (0, pw, 0, ph), "reflect")
        except BaseException:
            x = F.pad(x, (0, pw, 0, ph), "constant")
        return x

    def forward_features(self, f, plan, B, H, W):
        """grl.py:491-504 on the token matrix f [B*H*W, CP] (fp32) -> [B*H*W, CP]."""
        return forward_infer.forward_features(self, f, plan, B, H, W)

    @staticmethod
    def stream_groups(B: int) -> int:
        """Number of tile groups / HIP streams a batch of B tiles is processed in (GRL_SPLIT_STREAMS, default 2;
        measured on MI355X: 2 groups +6 % tiles/s over one stream, 4 groups are host-launch bound)."""
        n = SW.num("GRL_SPLIT_STREAMS")
        if SW.on("GRL_CHECK_RANGE"):
            return 1
        return n if n > 1 and B >= n and B % n == 0 else 1

    def enable_graph(self, flag: bool = True):
        """Replay the whole forward as one captured HIP graph per input shape.  A forward is ~500
        kernel launches; at one 256x256 tile the eager path is bound by the host issuing them, the graph is not.
        Every cached graph owns the plan (packed weights / tables) it was captured with; ``load_state_dict`` and in-place
        parameter updates drop the graphs (post-hook / version stamp).
        """
        self._use_graph = bool(flag)
        self._graphs = {}
        return self

    def forward(self, x):
        """grl.py:506-551.  Eager launch sequence, or a captured HIP graph (``enable_graph`` / GRL_GRAPH=1)."""
        if getattr(self, "_use_graph", None) is None:
            self._use_graph, self._graphs = SW.on("GRL_GRAPH"), {}
        if not (self._use_graph and x.is_cuda) or ops.profiling() or torch.is_grad_enabled():
            return self._forward_eager(x)
        key = (tuple(x.shape), x.dtype, str(x.device))
        stamp = self._param_stamp()
        ent = self._graphs.get(key)
        if ent is not None and ent[4] != stamp:            # parameters changed in place since the capture
            self.invalidate_plan()
            ent = None
        if ent is None:
            with torch.no_grad():
                self._forward_eager(x)                     # builds the plan, warms the allocator and kernel attributes
                torch.cuda.synchronize(x.device)
                static_in = x.clone()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    static_out = self._forward_eager(static_in)
            # the captured kernels point at the packed weights / tables of THIS shape's plan: the entry keeps them alive
            # (the plan cache itself holds one geometry at a time)
            ent = self._graphs[key] = (static_in, graph, static_out, next(iter(self._plan_cache.values())), stamp)
        static_in, graph, static_out = ent[:3]
        static_in.copy_(x)
        graph.replay()
        return static_out.clone()                          # the engine clamps its output in place (utils_image.py:31)

    def _forward_eager(self, x, plan=None):
        if not x.is_cuda:
            # CPU tensor: the composite torch path (composite.py; SURVEY 8(b) "errors", BASELINE configs[0]).  Not a fallback of the
            # GPU path -- a CUDA tensor never gets here and still fails loudly below when the HIP library is missing.
            if SW.on("GRL_NO_CPU_COMPOSITE"):
                raise RuntimeError("grl_image_restoration_amd.GRL: got a CPU tensor and GRL_NO_CPU_COMPOSITE=1 forbids the composite torch path "
                                   "(no CPU fallback)")
            if any(p.is_cuda for p in self.parameters()):
                raise RuntimeError("grl_image_restoration_amd.GRL: CPU input but the parameters live on the GPU")
            from . import composite
            composite.announce()
            return forward_train.forward(self, x)
        L.lib()  # fail loudly if the extension is missing
        if plan is None and torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return forward_train.forward(self, x)      # autograd path: every contraction, forward and backward, in libgrl_hip.so
        H0, W0 = x.shape[2:]
        x = self.check_image_size(x.float())
        mean = self._mean.to(x.device, x.dtype)
        x = (x - mean) * self.img_range
        if plan is None:
            plan = self._plan(tuple(x.shape[2:]), x.device)
        y = forward_infer.forward(self, x, plan) / self.img_range + mean
        return y[:, :, : H0 * self.upscale, : W0 * self.upscale].contiguous()
