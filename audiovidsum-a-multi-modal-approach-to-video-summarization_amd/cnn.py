"""CNN trunks of the visual extractor on the MI355X.

The reference builds ``torchvision.models.resnet50(pretrained=True)`` minus its
``fc`` as an ``nn.Sequential`` (features/extractors.py:25,29) and
``inception_v3(pretrained=True, aux_logits=True)`` with ``fc = Identity``
(:26,32-36).  torchvision and its weight files are not available offline, so
this module supplies

  * parameter containers with torchvision's module structure and state-dict
    keys (weights come from ``load_state_dict`` or a seeded init), and
  * runners that execute the trunks through libavsum_hip.so on NHWC tensors:
    every convolution is the implicit-GEMM kernel (fp32 MFMA = parity mode,
    bf16 MFMA = throughput mode); ResNet BatchNorm runs in BATCH-STATISTICS
    mode per micro-batch group, because the reference never puts that trunk in
    eval mode; Inception BatchNorm (eval mode, eps 1e-3) is folded
    into the convolution weights.

The containers deliberately have no torch forward: the product path is HIP only.
"""
from typing import NamedTuple

import torch
import torch.nn as nn

from . import ops

RESNET_MEAN = (0.485, 0.456, 0.406)
RESNET_STD = (0.229, 0.224, 0.225)


class _NoTorchForward(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover - guard
        raise RuntimeError("this module only holds parameters; the trunk runs through the HIP runner")


# ============================================================================ ResNet-50 container
class Bottleneck(_NoTorchForward):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)  # v1.5: stride on the 3x3
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


def _make_layer(inplanes, planes, blocks, stride):
    downsample = None
    if stride != 1 or inplanes != planes * 4:
        downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride, bias=False), nn.BatchNorm2d(planes * 4))
    layers = [Bottleneck(inplanes, planes, stride, downsample)]
    for _ in range(1, blocks):
        layers.append(Bottleneck(planes * 4, planes))
    return nn.Sequential(*layers)


def resnet50_trunk():
    """``nn.Sequential(*list(resnet50().children())[:-1])`` with torchvision's init (kaiming fan_out, BN 1/0)."""
    trunk = nn.Sequential(
        nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2, 1),
        _make_layer(64, 64, 3, 1), _make_layer(256, 128, 4, 2), _make_layer(512, 256, 6, 2),
        _make_layer(1024, 512, 3, 2), nn.AdaptiveAvgPool2d((1, 1)),
    )
    for m in trunk.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
        elif isinstance(m, nn.BatchNorm2d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)
    return trunk


# ============================================================================ helpers
def _ohwi(weight, dtype):
    """OIHW conv weight -> [O, kh*kw*I] in the kernel's reduction order."""
    o, i, kh, kw = weight.shape
    return weight.detach().permute(0, 2, 3, 1).reshape(o, kh * kw * i).to(dtype).contiguous()


def _stem_weight(weight, px, dtype):
    """Stem conv [O,3,kh,kw] on the 4-channel pre-padded image: each kernel row becomes ``px`` pixels x 4
    channels (zero beyond kw and in channel 3) so that one reduction step is a contiguous run of pixels."""
    o, i, kh, kw = weight.shape
    w = torch.zeros((o, kh, px, 4), dtype=torch.float32, device=weight.device)
    w[:, :, :kw, :i] = weight.detach().permute(0, 2, 3, 1)
    return w.reshape(o, kh * px * 4).to(dtype).contiguous()


class _W:
    """A convolution weight in kernel layout: `rows` = [cout, kh*kw*cin] (what the 1x1 BatchNorm kernels and the stem
    read) and, when the reduction is a multiple of a 64-byte step, `kstep` = the same matrix reduction-step major
    (ops.weights_kstep32: whole cache lines per weight DMA instruction of the contraction kernel)."""
    __slots__ = ("rows", "kstep")

    def __init__(self, rows):
        self.rows = rows
        step = 32 if rows.dtype == torch.bfloat16 else 16   # elements of a 64-byte reduction step
        self.kstep = ops.weights_kstep32(rows) if rows.shape[1] % step == 0 else None

    def conv_operand(self):
        """(tensor, w_layout) for avs_conv2d_nhwc*."""
        return (self.kstep, 1) if self.kstep is not None else (self.rows, 0)


class Step(NamedTuple):
    """One step of the trunk (ResNet50Runner.plan), in launch order.
    name   torchvision's key of the convolution ("conv1", "layer1.0.conv2", "layer1.0.downsample"); layer 1's shared Gram
           step is "layer1.0.conv1+downsample"
    form   how it runs (the class docstring)
    inp    "finished", or "raw": the input is the previous step's raw output, whose BatchNorm (+ ReLU) this step applies
           (gram / gram_pair: in its staging; stats: in the nine-tap kernel's staging where the library takes it, else by an
           apply pass over the input first; split: an apply pass first)
    out    "finished"; "deferred": the raw output + its affine, applied by the consumer; "p8": stored as AVS_F16P8
    res    conv3's residual: "none", "identity", "downsample" (finished) or "deferred" (raw, its BatchNorm applied in this
           step's residual add)
    block  bottleneck index (-1: the stem)
    geom   (convolution geometry, input strides, weight row stride) as the avs_conv2d_nhwc* descriptor takes them
    cluster  the clustered form: tiles per group
    packed   the clustered form runs packed: tiles of 224 consecutive rows instead of one 196-row tile per map (quarter)"""
    name: str
    form: str
    inp: str = "finished"
    out: str = "finished"
    res: str = "none"
    block: int = -1
    geom: tuple = None
    cluster: int = 1
    packed: bool = False


class ResNet50Runner:
    """Runs the container's parameters on uint8 frames [N,224,224,3] -> fp32 [N,2048].

    Batch-statistics BatchNorm (the reference's mode) takes one of these forms per convolution, chosen by plan();
    every one of them is deterministic (no float atomics: two runs give bit-identical features):
      local      bf16 / f16x2, equal-sized groups of <= 256 rows (14x14 / 7x7 maps): convolution + whole BatchNorm
                 (+ residual + ReLU) in ONE launch, statistics inside a tile (avs_conv2d_nhwc_bnlocal) - nothing raw in HBM;
      cluster    f16x2: the same with a group spread over several tiles that exchange their statistics
                 (avs_conv2d_nhwc_bncluster; pack_groups: on tiles of 224 consecutive rows where the library takes the groups
                 packed - Step.packed);
      gram       bf16 / f16x2 expanding 1x1 layers with 64 / 128 input channels (conv3 / downsample of layers 1-2):
                 statistics from the input's Gram matrix, then ONE streaming pass with the affine in the epilogue;
      gram_pair  layer 1's first conv1 and downsample read the same input: one Gram matrix, one streaming pass each;
      stats      convolution + per-tile partial statistics in its epilogue, folded in tile order, then an apply pass
                 (bf16, fp32-split, f16x2: equal groups of >= 64 rows);
      split      convolution, avs_bn_batch_stats, avs_bn_apply (fp32 parity mode, ragged groups, shapes the others decline);
      folded     bn_mode="folded": running statistics folded into an apply pass after the convolution.
    The stem is the fused bf16 (stem_bf16) or f16x2 (stem_f16x2) kernel, or the frames' normalisation + "conv1" in one of
    the forms above, followed by the max pooling."""

    def __init__(self, trunk, dtype=torch.float32, bn_mode="batch", f32_split=False):
        """f32_split (fp32 only): True = activations and weights stay fp32 in HBM, the convolutions' products run on the
        bf16 matrix cores as hi*hi + hi*lo + lo*hi (AVS_F32_SPLIT: ~2^-15 relative per product instead of exact);
        "f16x2" = AVS_F16X2: activations and weights are STORED as fp16 hi | lo runs (22 significant bits, the byte
        size of fp32), products are three fp16 MFMAs with no arithmetic on the operands, every output is split once
        where it is produced, BatchNorm statistics are centred two-round sums: the fast parity-grade mode."""
        if bn_mode not in ("batch", "folded"):
            raise ValueError("bn_mode must be 'batch' (reference-faithful) or 'folded'")
        self.trunk, self.dtype, self.bn_mode = trunk, dtype, bn_mode
        self.h2 = f32_split == "f16x2" and dtype == torch.float32
        self.f32_split = bool(f32_split) and not self.h2 and dtype == torch.float32
        self.code = ops.dtype_code(dtype, "f16x2" if self.h2 else self.f32_split)   # the contraction entry points
        self.ecode = self.code if self.h2 else ops.dtype_code(dtype)                 # storage format (elementwise kernels)
        self.fuse_conv_bn = True     # bf16: the Gram form for the 1x1 layers of at least fuse_min_rows rows per group whose
        self.fuse_min_rows, self.fuse_ratio_num, self.fuse_ratio_den = 128, 2, 1   # cout / cin >= num / den (f16x2: >= 2)
        self.bn_local = True         # the one-launch tile-local form where the library takes the shape
        self.bn_cluster = True       # AVS_F16X2: groups of several 14x14 maps in ONE launch (tiles exchange their statistics)
        self.pack_groups = True      # ... on tiles of 224 consecutive rows where the library takes the groups packed (4-frame
                                     # groups of 14x14 maps: 7 full tiles per 2 groups instead of 8 of 196 rows)
        self.fused_stem = True       # uint8 frames -> conv1 -> pooled raw map + partial sums in one kernel
        self.stem_raw = True         # bf16: bn1 + ReLU ride in the staging of layer 1's first conv1 / downsample (both take the
                                     # one-pass form on ONE Gram matrix of the stem output): no finishing pass
        self.defer_bn_apply = True   # bn2 + ReLU applied inside conv3's Gram / one-pass kernels
        self.defer_res_apply = True  # the downsample's BatchNorm applied inside conv3's residual add (layer 2's first block)
        self.fold_input_bn = True    # AVS_F16X2: conv1 of the stride-1 bottlenecks stays RAW and its bn1 + ReLU ride in the
                                     # staging of conv2's nine-tap kernel (avs_conv2d_nhwc_bnstats_xin): no apply pass over it
        self.gram_finish_min_k = 128  # bf16, >= this many input channels: the Gram kernel stores the finished input in place,
                                      # so the convolution pass (N / 128 column slabs) does not transform it per slab
        self.p8_blocks = (0, 1, 3, 4, 5) if self.h2 else ()   # AVS_F16X2: the outputs of these bottlenecks (the inner
                                     # blocks of layers 1-2, whose consumers are the next block's conv1 and residual add - both
                                     # HBM-bound) are stored as AVS_F16P8: fp16 hi + 8-bit remainder, 3 instead of 4 bytes
        self._key = None
        self._w = None
        self._plans = {}     # plan key (shapes + switches) -> steps

    block_hook = None   # study hook: callable(block index, block output) -> block output

    def _blocks(self):
        """(torchvision name, Bottleneck) in forward order."""
        for li in range(4):
            for b, blk in enumerate(self.trunk[4 + li]):
                yield f"layer{li + 1}.{b}", blk

    def _pair_ok(self):
        """Layer 1's first conv1 and downsample read the same input: can ONE Gram matrix give both BatchNorms' statistics?"""
        b0 = self.trunk[4][0]
        d = b0.downsample
        return d is not None and b0.conv1.weight[0].numel() == d[0].weight[0].numel() and b0.bn1.eps == d[1].eps

    # weights in kernel layout, rebuilt when the parameters change / move
    def _prepare(self):
        key = tuple((p.data_ptr(), p._version) for p in self.trunk.parameters()) + (self.dtype,)
        if self._w is not None and key == self._key:
            return self._w
        t, dt = self.trunk, self.dtype
        pack = ops.f16x2_pack if self.h2 else (lambda r: r)   # AVS_F16X2: every weight row as fp16 hi | lo runs, once

        def bn(m):
            return (m.weight.detach().float().contiguous(), m.bias.detach().float().contiguous(), float(m.eps),
                    m.running_mean.detach().float(), m.running_var.detach().float())

        w = {"conv1": (_W(pack(_stem_weight(t[0].weight, 8, dt))), bn(t[1]))}
        if self.h2 and tuple(t[0].weight.shape) == (64, 3, 7, 7):
            # the fused AVS_F16X2 stem: the input normalisation folded into the weights (the constant term in channel 3)
            w["stem_h2"] = ops.stem_h2_operands(t[0].weight, 1.0, RESNET_MEAN, RESNET_STD)
        for name, blk in self._blocks():
            convs = [("conv1", blk.conv1, blk.bn1), ("conv2", blk.conv2, blk.bn2), ("conv3", blk.conv3, blk.bn3)]
            if blk.downsample is not None:
                convs.append(("downsample", *blk.downsample))
            for key_, conv, norm in convs:
                w[f"{name}.{key_}"] = (_W(pack(_ohwi(conv.weight, dt))), bn(norm))
        if self._pair_ok():
            # the Gram step's operands: conv1's and the downsample's weights / BatchNorm parameters stacked
            (c1, b1), (cd, bd) = w["layer1.0.conv1"], w["layer1.0.downsample"]
            w["layer1.0.conv1+downsample"] = (torch.cat([c1.rows, cd.rows]).contiguous(), torch.cat([b1[0], bd[0]]).contiguous(),
                                              torch.cat([b1[1], bd[1]]).contiguous(), b1[2], c1.rows.shape[0])
        self._w, self._key = w, key
        return w

    # ---- convolution geometry ----
    @staticmethod
    def _stem_geom(n):
        # [N,230,232,4] pre-padded image; conv1 7x7/2 reads 8-pixel (32-element) runs: kh = 7 rows x 32 elements
        return (n, 230, 112, 32, 7, 1, 2, 1, 0, 0, 112, 112, 64), (230 * 232 * 4, 232 * 4, 8), 7 * 32

    @staticmethod
    def _nhwc_geom(n, h, cin, k, s, p, cout):
        ho = (h + 2 * p - k) // s + 1
        return (n, h, h, cin, k, k, s, s, p, p, ho, ho, cout), (h * h * cin, h * cin, cin), k * k * cin

    # ---- the plan ----
    def _gram_ok(self, cin, cout, kh, sh, gmax):
        """The Gram form: expanding 1x1 / stride-1 layers with 64 / 128 input channels and groups of >= fuse_min_rows
        rows (measured on MI355X: it wins over the split form where the layer is write-heavy and a group several row
        tiles long)."""
        if not (kh == 1 and sh == 1 and gmax >= self.fuse_min_rows and ops.gram_supported(cin, cout)):
            return False
        if self.h2:
            return cout >= 2 * cin
        return (self.dtype == torch.bfloat16 and self.fuse_conv_bn
                and cout * self.fuse_ratio_den >= cin * self.fuse_ratio_num)

    def _tile_local(self, geom, gsz, cluster):
        """(k, packed): k = 1: the tile-local form takes the layer, k > 1: the clustered form with groups of k tiles (packed:
        in its packed form), 0: neither."""
        g, xs, wrs = geom
        cin, kh, ho, wo, cout = g[3], g[4], g[10], g[11], g[12]
        rows = gsz * ho * wo
        if rows <= 256:
            return int(ops.conv_bnlocal_tile_rows(self.code, *g, *xs, wrs, cout, rows) is not None), False
        if not (self.h2 and cluster):
            return 0, False
        # a group larger than a tile: the map splits into k tiles of 193..224 rows (14 x 14: k = 1, layer 3 with the
        # reference's 4-frame micro-batches; 28 x 28: k = 4) and the group into gsz * k <= 16 of them
        for k in (1, 2, 4, 8, 16):
            # (maps of several tiles: only the wide 1x1 layer that would otherwise take convolution + statistics + an
            #  apply pass - layer 3's first conv1, 512 -> 256 at 28 x 28; measured: layer 2's narrow layers are no faster
            #  clustered than on their Gram / nine-tap / 3-byte forms)
            if k > 1 and not (kh == 1 and cin >= 512 and cout >= 256):
                continue
            if (ho * wo) % k == 0 and 192 < (ho * wo) // k <= 224 and 2 <= gsz * k <= 16:
                # the packed form first (groups of several frames; measured at 4-frame groups only); a shape it declines
                # keeps the unpacked answer
                if self.pack_groups and gsz > 1 and ops.conv_bncluster_ok(self.code, *g, *xs, wrs, cout, rows, gsz * k, packed=True):
                    return gsz * k, True
                return (gsz * k if ops.conv_bncluster_ok(self.code, *g, *xs, wrs, cout, rows, gsz * k) else 0), False
        return 0, False

    def plan(self, n, group_frames=None, bn_cluster=None):
        """The trunk's steps (Step) in launch order for n frames in BatchNorm groups `group_frames` (forward's
        argument).  bn_cluster: a per-call override of the switch.  From shapes, the trunk's structure, the switches and
        the library's host-only queries: no weights are touched."""
        _, gsz, uniform = self._group_sizes(n, group_frames)
        return self._plan(n, gsz, uniform, self.bn_cluster if bn_cluster is None else bn_cluster)

    def _plan(self, n, gsz, uniform, cluster):
        key = (n, gsz, uniform, bool(cluster), bool(self.pack_groups), self.bn_local, self.fused_stem, self.stem_raw, self.fuse_conv_bn,
               self.fuse_min_rows, self.fuse_ratio_num, self.fuse_ratio_den, self.defer_bn_apply, self.defer_res_apply,
               self.fold_input_bn, tuple(self.p8_blocks), self.block_hook is None)
        steps = self._plans.get(key)
        if steps is not None:
            return steps
        batch, bf16, h2 = self.bn_mode == "batch", self.dtype == torch.bfloat16, self.h2
        # statistics from the convolution's epilogue: the bf16 mode, and the fp32-split mode (whose products already carry
        # ~2^-15 of error: the E[y^2] - E[y]^2 form on fp32 sums costs nothing next to that), f16x2 (centred sums); the
        # exact fp32 parity mode keeps the shifted statistics pass over the stored output
        fast = batch and uniform and (bf16 or self.f32_split or h2)
        local = self.bn_local and fast and (bf16 or h2)

        def form(geom, x_p8=False):
            """(form, cluster, packed) of one convolution + BatchNorm on its own."""
            g, xs, wrs = geom
            cin, kh, sh, ho, wo, cout = g[3], g[4], g[6], g[10], g[11], g[12]
            if not batch:
                return "folded", 1, False
            k, packed = self._tile_local(geom, gsz, cluster) if local else (0, False)
            if k:
                return ("local", 1, False) if k == 1 else ("cluster", k, packed)
            if fast and self._gram_ok(cin, cout, kh, sh, gsz * ho * wo):
                return "gram", 1, False
            if fast and ops.conv_bnstats_ok(self.code, *g, *xs, wrs, cout, gsz * ho * wo, x_p8=x_p8):
                return "stats", 1, False
            return "split", 1, False

        split_forms, tiled = ("stats", "split"), ("local", "cluster")
        pair = self._pair_ok()
        cpair = self.trunk[4][0].conv1.out_channels + self.trunk[4][0].downsample[0].out_channels if pair else 0
        x_raw = False    # the block input is the fused stem's RAW pooled map (bn1 + ReLU applied by the Gram step)
        if self.fused_stem and batch and uniform and bf16:
            x_raw = (self.stem_raw and self.fuse_conv_bn and pair and ops.gram_supported(64, cpair)
                     and gsz * 56 * 56 >= self.fuse_min_rows)
            steps = [Step("conv1", "stem_bf16", out="deferred" if x_raw else "finished")]
        elif (self.fused_stem and h2 and batch and uniform and tuple(self.trunk[0].weight.shape) == (64, 3, 7, 7) and pair
              and self._gram_ok(64, cpair, 1, 1, gsz * 56 * 56)):
            x_raw = True
            steps = [Step("conv1", "stem_f16x2", out="deferred")]
        else:
            geom = self._stem_geom(n)
            f, k, pk = form(geom)
            steps = [Step("conv1", f, geom=geom, cluster=k, packed=pk)]
        blocks = list(self._blocks())
        h, cin, x_out = 56, 64, "finished"
        for bi, (name, blk) in enumerate(blocks):
            s, planes = blk.stride, blk.conv1.out_channels
            hout = h // s
            g1 = self._nhwc_geom(n, h, cin, 1, 1, 0, planes)
            g2 = self._nhwc_geom(n, h, planes, 3, s, 1, planes)
            gd = self._nhwc_geom(n, h, cin, 1, s, 0, planes * 4) if blk.downsample is not None else None
            g3 = self._nhwc_geom(n, hout, planes, 1, 1, 0, planes * 4)
            f1, f2, f3 = form(g1, x_out == "p8"), form(g2), form(g3)
            fd = form(gd) if gd is not None else None
            use_pair = bi == 0 and pair and (x_raw or (h2 and fast and f1[0] not in tiled and fd[0] not in tiled
                                                         and self._gram_ok(cin, planes * 4, 1, 1, gsz * h * h)))
            # conv1's output stays raw, its bn1 + ReLU applied by conv2 (the nine-tap kernel's staging, else an apply pass)
            fold1 = (self.fold_input_bn and h2 and uniform and s == 1 and not use_pair and f1[0] in split_forms
                     and f2[0] in split_forms)
            # bn2 + ReLU ride in conv3's Gram / one-pass kernels: conv2 only writes its raw output and statistics
            defer2 = self.defer_bn_apply and f3[0] == "gram" and f2[0] in split_forms
            # a downsample that would take convolution + statistics + apply keeps its output RAW: its BatchNorm is folded
            # into conv3's residual add
            deferd = gd is not None and not use_pair and defer2 and self.defer_res_apply and fd[0] in split_forms
            # 3-byte storage of this block's output: conv3 is the one-pass form here and the next block's conv1 (dense 1x1
            # on this output, convolution + statistics) reads that format
            nxt = blocks[bi + 1][1] if bi + 1 < len(blocks) else None
            p8 = (bi in self.p8_blocks and h2 and f3[0] == "gram" and self.block_hook is None and nxt is not None
                  and nxt.stride == 1 and nxt.downsample is None
                  and form(self._nhwc_geom(n, hout, planes * 4, 1, 1, 0, nxt.conv1.out_channels), True)[0] == "stats")
            if use_pair:
                steps.append(Step(name + ".conv1+downsample", "gram_pair", "raw" if x_raw else "finished", block=bi, geom=g1))
            else:
                steps.append(Step(name + ".conv1", f1[0], out="deferred" if fold1 else "finished", block=bi, geom=g1,
                                  cluster=f1[1], packed=f1[2]))
            steps.append(Step(name + ".conv2", f2[0], "raw" if fold1 else "finished", "deferred" if defer2 else "finished",
                              block=bi, geom=g2, cluster=f2[1], packed=f2[2]))
            if gd is not None and not use_pair:
                steps.append(Step(name + ".downsample", fd[0], out="deferred" if deferd else "finished", block=bi, geom=gd,
                                  cluster=fd[1], packed=fd[2]))
            steps.append(Step(name + ".conv3", f3[0], "raw" if defer2 else "finished", "p8" if p8 else "finished",
                              "deferred" if deferd else "downsample" if gd is not None else "identity", bi, g3, f3[1], f3[2]))
            h, cin, x_out, x_raw = hout, planes * 4, steps[-1].out, False
        if len(self._plans) > 64:
            self._plans.clear()
        self._plans[key] = steps = tuple(steps)
        return steps

    # ---- the executor ----
    @staticmethod
    def _group_sizes(n, group_frames):
        if group_frames is None:
            group_frames = torch.arange(n + 1, dtype=torch.int64)
        group_frames = torch.as_tensor(group_frames, dtype=torch.int64)
        if int(group_frames[0]) != 0 or int(group_frames[-1]) != n:
            raise ValueError("group_frames must start at 0 and end at N")
        sizes = group_frames[1:] - group_frames[:-1]
        gsz = int(sizes.max())
        return group_frames, gsz, bool((sizes == gsz).all())

    def _conv(self, st, w, x, x_aff, groups, residual=None, res_aff=None):
        """One convolution + BatchNorm (+ residual, + ReLU) in the step's form -> (output, its (scale, shift) when the
        step's output is deferred, else None).  The stem's max pooling follows (on the split forms fused with the
        BatchNorm apply: avs_bn_maxpool_nhwc, the normalised full-resolution map is never written)."""
        (geom, xs, _), (wt, (gamma, beta, eps, rmean, rvar)) = st.geom, w[st.name]
        n, cin, kh, ho, wo, cout = geom[0], geom[3], geom[4], geom[10], geom[11], geom[12]
        dev, dt, stem = x.device, self.dtype, st.block < 0
        relu = not st.name.endswith("downsample")
        act = ops.ACT_RELU if relu else ops.ACT_NONE
        grows, gmax = groups[ho * wo]
        wsel, layout = wt.conv_operand()
        y = torch.empty((n, ho, wo, cout), dtype=dt, device=dev)

        def pooled():   # the stem's max pooling 3x3 / 2, pad 1
            return torch.empty((n, (ho + 2 - 3) // 2 + 1, (wo + 2 - 3) // 2 + 1, cout), dtype=dt, device=dev)

        if st.form == "gram":
            x2d = x.view(-1, cin)
            if self.h2:
                # statistics from the input's second moments (the pass that also applies the BatchNorm + ReLU of the layer
                # before, storing the finished input in place), then ONE streaming pass with the affine in its epilogue
                sc, sf = ops.bn_gram_affine_h2(x2d, wt.rows, gmax, gamma, beta, eps, x_aff, store_input=x_aff is not None)
                if st.out == "p8":
                    y = ops.P8.empty((n, ho, wo, cout), dev)
                ops.conv2d_affine(self.code, n, geom[1], geom[2], cin, geom[6], geom[7], ho, wo, cout, x, *xs, wsel,
                                  wsel.stride(0), y, cout, gmax, sc, sf, residual, relu, res_aff, w_layout=layout)
            else:
                ops.conv1x1_gram_bn(x2d, wt.rows, gmax, gamma, beta, eps, y.view(-1, cout), residual, relu, x_aff, res_aff,
                                    finish_input=cin >= self.gram_finish_min_k)
            return y, None

        def conv(**kw):
            return ops.conv2d_raw(self.code, *geom, x, *xs, wsel, wsel.stride(0), y, cout, algo_k=147 if stem else None,
                                  algo_in_elems=x.numel() if stem else None, w_layout=layout, **kw)

        if st.form in ("local", "cluster"):
            conv(act=act, bnlocal=(gmax, gamma, beta, eps, residual), cluster=st.cluster, packed=st.packed)
            return (ops.pool2d(y, "max", 3, 2, 1, pooled(), code=self.ecode) if stem else y), None
        affine = None
        if st.form == "folded":
            conv()
            scale = (gamma / torch.sqrt(rvar + eps)).contiguous()
            affine, grows, gmax = (scale.view(1, -1), (beta - rmean * scale).contiguous().view(1, -1)), None, 0
        else:
            if x_aff is not None:
                if st.form == "stats" and kh == 3:
                    affine = conv(bnstats=(gmax, gamma, beta, eps), x_affine=(x_aff[0], x_aff[1], True))
                if affine is None:   # (the library's nine-tap form declined: the apply pass over x in place, then the plain one)
                    xg = groups[geom[1] * geom[2]]
                    ops.bn_apply(x.view(-1, cin), x_aff[0], x_aff[1], xg[0], xg[1], None, ops.ACT_RELU, x.view(-1, cin),
                                 code=self.ecode)
            if st.form == "stats" and affine is None:
                affine = conv(bnstats=(gmax, gamma, beta, eps))
            elif st.form == "split":
                conv()
                affine = ops.bn_batch_stats(y.view(-1, cout), grows, gamma, beta, eps, code=self.ecode)
            if st.out == "deferred":
                return y, affine
        if stem:
            return ops.bn_maxpool(y, affine[0], affine[1], grows, relu, 3, 2, 1, pooled(), code=self.ecode), None
        ops.bn_apply(y.view(-1, cout), affine[0], affine[1], grows, gmax, residual, act, y.view(-1, cout), code=self.ecode)
        return y, None

    def _gram_pair(self, st, w, x, x_aff, gmax):
        """Layer 1's first conv1 and downsample: ONE Gram matrix gives both BatchNorms' affines (applying the stem's
        bn1 + ReLU on the way in when x is its raw map), then one streaming pass each -> (conv1's output, the downsample's
        as [rows, cout])."""
        wcat, gcat, bcat, eps, c1n = w[st.name]
        block = st.name.split(".conv1+")[0]
        geom, xs, _ = st.geom
        n, h, cin = geom[0], geom[1], geom[3]
        x2d = x.view(-1, cin)
        if self.h2:   # (the finished input is stored in place: the streaming passes read it as it is)
            sc, sf = ops.bn_gram_affine_h2(x2d, wcat, gmax, gcat, bcat, eps, x_aff, store_input=x_aff is not None)
        else:
            sc, sf = ops.bn_gram_affine(x2d, wcat, gmax, gcat, bcat, eps, x_aff)
        outs = []
        for part, cols, relu in (("conv1", slice(0, c1n), True), ("downsample", slice(c1n, None), False)):
            wt = w[f"{block}.{part}"][0]
            cout = wt.rows.shape[0]
            y = torch.empty((n, h, h, cout), dtype=self.dtype, device=x.device)
            if self.h2:
                wsel, layout = wt.conv_operand()
                ops.conv2d_affine(self.code, n, h, h, cin, 1, 1, h, h, cout, x, *xs, wsel, wsel.stride(0), y, cout, gmax,
                                  sc[:, cols].contiguous(), sf[:, cols].contiguous(), None, relu, None, w_layout=layout)
            else:
                ops.conv1x1_affine(x2d, wt.rows, gmax, sc[:, cols].contiguous(), sf[:, cols].contiguous(), y.view(-1, cout),
                                   None, relu, x_aff)
            outs.append(y)
        return outs[0], outs[1].view(-1, outs[1].shape[3])

    def forward(self, frames_u8, group_frames=None, out=None, mid_hook=None, bn_cluster=None):
        """frames_u8: device uint8 [N,224,224,3] (already 224x224, extractors.py:132).
        group_frames: int64 CPU tensor / list [G+1] of frame offsets of the BatchNorm micro-batch groups
        (extractors.py:48-56); default = one group per frame.
        mid_hook: called (no arguments) once layers 1-2 - the HBM-bound half of the trunk - have been launched and
        before layers 3-4 - the matrix-core-bound half: the pipeline records a stream event there, so that the next
        pass (on another stream) runs its memory-bound half under this pass's compute-bound half.
        bn_cluster: this call's choice of the clustered form (None: the runner's switch)."""
        n, h, w_, _ = frames_u8.shape
        if (h, w_) != (224, 224):
            raise ValueError("ResNet50Runner expects 224x224 frames (resize first)")
        if n == 0:
            return torch.zeros((0, 2048), dtype=torch.float32, device=frames_u8.device)
        group_frames, gsz, uniform = self._group_sizes(n, group_frames)
        steps = self._plan(n, gsz, uniform, self.bn_cluster if bn_cluster is None else bn_cluster)
        w = self._prepare()
        dev = frames_u8.device
        groups = {hw: ((group_frames * hw).to(dev), gsz * hw) for hw in (112 * 112, 56 * 56, 28 * 28, 14 * 14, 7 * 7)}
        x = x_aff = t = t_aff = idn = idn_aff = None
        for st in steps:
            part = st.name.rsplit(".", 1)[-1]
            if part in ("conv1", "conv1+downsample") and st.block == 7 and mid_hook is not None:
                mid_hook()   # (blocks 0-2 = layer 1, 3-6 = layer 2)
            if st.form == "stem_bf16":
                # one fused launch: the normalised image and the 112x112x64 map never reach HBM.  bn1 + ReLU: a finishing
                # pass in place, or inside the staging of the first block's Gram step
                gamma, beta, eps = w["conv1"][1][:3]
                x, sc0, sh0 = ops.stem_conv_bn_pool(frames_u8, w["conv1"][0].rows, 1.0, RESNET_MEAN, RESNET_STD, gsz, gamma,
                                                    beta, eps, apply=st.out == "finished")
                x_aff = (sc0, sh0) if st.out == "deferred" else None
            elif st.form == "stem_f16x2":
                # one fused launch (uint8 frames -> conv1 on the fp16 matrix cores -> centred statistics -> the pooled RAW
                # map); bn1 + ReLU are applied by the first block's Gram step, which stores the finished map in place
                gamma, beta, eps = w["conv1"][1][:3]
                x, sc0, sh0 = ops.stem_conv_pool_h2(frames_u8, w["stem_h2"], gsz, gamma, beta, eps)
                x_aff = (sc0, sh0)
            elif st.block < 0:
                # (x - mean)/std without /255 (extractors.py:133-139), conv1 7x7/2 pad 3, bn1, ReLU, maxpool 3x3/2
                x0 = ops.frames_normalize(frames_u8, self.dtype, 1.0, RESNET_MEAN, RESNET_STD, 230, 232, 3, 3, code=self.ecode)
                x = self._conv(st, w, x0, None, groups)[0]
                del x0
            elif part == "conv1+downsample":
                t, idn = self._gram_pair(st, w, x, x_aff, groups[st.geom[0][1] ** 2][1])
                x_aff = None
            elif part == "conv1":
                t, t_aff = self._conv(st, w, x, None, groups)
            elif part == "conv2":
                t, t_aff = self._conv(st, w, t, t_aff, groups)
            elif part == "downsample":
                idn, idn_aff = self._conv(st, w, x, None, groups)
                idn = idn.view(-1, idn.shape[3])
            else:
                if st.res == "identity":
                    idn = x if isinstance(x, ops.P8) else x.view(-1, x.shape[3])
                x, _ = self._conv(st, w, t, t_aff, groups, idn, idn_aff)
                t = t_aff = idn = idn_aff = None
                if self.block_hook is not None:   # study tools only (tools/h3_storage_study.py): a block output's storage format
                    x = self.block_hook(st.block, x)
        return ops.global_avgpool(x, out, code=self.ecode)


# ============================================================================ Inception-v3 container
class BasicConv2d(_NoTorchForward):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)


class InceptionA(_NoTorchForward):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)


class InceptionB(_NoTorchForward):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)


class InceptionC(_NoTorchForward):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)


class InceptionD(_NoTorchForward):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)


class InceptionE(_NoTorchForward):
    def __init__(self, cin):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)


class InceptionAux(_NoTorchForward):
    """Present in the checkpoint the reference loads (aux_logits=True at construction,
    extractors.py:26) but never executed (aux_logits set False at :36, eval mode)."""

    def __init__(self, cin, num_classes):
        super().__init__()
        self.conv0 = BasicConv2d(cin, 128, kernel_size=1)
        self.conv1 = BasicConv2d(128, 768, kernel_size=5)
        self.fc = nn.Linear(768, num_classes)


class Inception3(_NoTorchForward):
    """torchvision ``Inception3`` module tree with ``fc = Identity`` and ``transform_input = True``
    (what ``inception_v3(pretrained=True)`` sets)."""

    def __init__(self):
        super().__init__()
        self.aux_logits = True
        self.transform_input = True
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.maxpool1 = nn.MaxPool2d(kernel_size=3, stride=2)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.maxpool2 = nn.MaxPool2d(kernel_size=3, stride=2)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.AuxLogits = InceptionAux(768, 1000)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280)
        self.Mixed_7c = InceptionE(2048)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.dropout = nn.Dropout(p=0.5)
        self.fc = nn.Identity()
        # Synthetic init (no pretrained weights offline): variance-preserving, so that eval-mode
        # BatchNorm with running stats (0, 1) keeps activations O(1) through 94 convolutions.
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self.eval()


INCEPTION_TRANSFORM = (0.229 / 0.5, 0.224 / 0.5, 0.225 / 0.5,
                       (0.485 - 0.5) / 0.5, (0.456 - 0.5) / 0.5, (0.406 - 0.5) / 0.5)


class InceptionV3Runner:
    """uint8 frames [N,299,299,3] -> fp32 [N,2048]; eval-mode BatchNorm folded into the convolutions."""

    def __init__(self, net, dtype=torch.float32, f32_split=False):
        """f32_split: as ResNet50Runner (True = AVS_F32_SPLIT, "f16x2" = AVS_F16X2 storage and arithmetic)."""
        self.net, self.dtype = net, dtype
        self.h2 = f32_split == "f16x2" and dtype == torch.float32
        self.f32_split = "f16x2" if self.h2 else (bool(f32_split) and dtype == torch.float32)
        self.ecode = ops.dtype_code(dtype, "f16x2") if self.h2 else ops.dtype_code(dtype)   # storage format
        self.pool_after_conv = True   # branch_pool: 1x1 convolution first, average pooling on its (narrow) output
        self.split_tail_columns = False  # cout = 128 k + r (r <= 64): two launches instead of a mostly empty last column tile
        #                                  (measured: no gain - these layers are not bound by the matrix work; off)
        self.stack_pool_head = True      # ... branch_pool's convolution too (its columns without bias / ReLU: they follow the pooling)
        self.stack_heads = True          # AVS_F16X2: the 1x1 heads of a block that read the block input run as ONE contraction
        #                                  over their stacked filters (avs_conv2d_nhwc_split): the input is fetched once
        self._key = None
        self._w = None

    def _fold(self, bc, stem_px=None):
        conv, bn = bc.conv, bc.bn
        with torch.no_grad():
            s = bn.weight.float() / torch.sqrt(bn.running_var.float() + bn.eps)
            wt = conv.weight.float() * s.view(-1, 1, 1, 1)
            bias = (bn.bias.float() - bn.running_mean.float() * s).contiguous()
            rows = _stem_weight(wt, stem_px, self.dtype) if stem_px else _ohwi(wt, self.dtype)
            w = _W(ops.f16x2_pack(rows) if self.h2 else rows)
            # column tiles are 128 wide (64 for cout <= 64): a layer with cout = 128 k + r, 0 < r <= 64 (192, 160, 320, 448:
            # most of Inception-v3) would spend a whole 128-column tile's matrix work on its last r columns - 25 - 37 % of
            # the layer.  Such a layer runs as TWO launches, the first 128 k columns on the wide tile and the last r on
            # the 64-column one, each writing its own channel slice: the same outputs, bit for bit
            parts = None
            cout = conv.out_channels
            r = cout % 128
            if self.split_tail_columns and not stem_px and cout > 128 and 0 < r <= 64:
                parts = []
                for a, b in ((0, cout - r), (cout - r, cout)):
                    pr = rows[a:b].contiguous()
                    parts.append((a, b, _W(ops.f16x2_pack(pr) if self.h2 else pr), bias[a:b].contiguous()))
        kh, kw = conv.kernel_size
        return {"w": w, "b": bias, "kh": kh, "kw": kw, "s": conv.stride[0], "ph": conv.padding[0],
                "pw": conv.padding[1], "cout": conv.out_channels, "parts": parts}

    def _prepare(self):
        key = tuple((p.data_ptr(), p._version) for p in self.net.parameters()) + \
            tuple((b.data_ptr(), b._version) for b in self.net.buffers()) + (self.dtype,)
        if self._w is not None and key == self._key:
            return self._w
        w = {}
        for name, m in self.net.named_modules():
            if isinstance(m, BasicConv2d) and not name.startswith("AuxLogits"):
                w[name] = self._fold(m, stem_px=4 if name == "Conv2d_1a_3x3" else None)
        self._w, self._key = w, key
        return w

    # conv + folded BN + ReLU into `out` (an NHWC view, possibly a channel slice)
    def _conv(self, w, name, x, out=None):
        c = w[name]
        n, h, ww, _ = x.shape
        ho = (h + 2 * c["ph"] - c["kh"]) // c["s"] + 1
        wo = (ww + 2 * c["pw"] - c["kw"]) // c["s"] + 1
        if out is None:
            out = torch.empty((n, ho, wo, c["cout"]), dtype=self.dtype, device=x.device)
        if c["parts"] is not None:
            for a, b, wp, bp in c["parts"]:
                wsel, layout = wp.conv_operand()
                ops.conv2d(x, wsel, c["kh"], c["kw"], c["s"], (c["ph"], c["pw"]), out[..., a:b], bp, ops.ACT_RELU,
                           split=self.f32_split, w_layout=layout)
            return out
        wsel, layout = c["w"].conv_operand()
        return ops.conv2d(x, wsel, c["kh"], c["kw"], c["s"], (c["ph"], c["pw"]), out, c["b"], ops.ACT_RELU,
                          split=self.f32_split, w_layout=layout)

    def _heads(self, w, p, x, first, others, first_out, pool=None):
        """The block's 1x1 convolutions that read x: `first` (or None) writes first_out (its slice of the block's
        concatenated output), `others` feed further convolutions, `pool` (or None) is branch_pool's convolution, whose
        average pooling, bias and ReLU follow (_pool_branch).  Returns the NHWC views of the others' outputs (+ the pool
        head's raw output, or None when it was not run here).  With stack_heads (AVS_F16X2): ONE contraction over the
        stacked filters, two destinations, the pool head's columns without bias / ReLU."""
        names = [p + "." + nm for nm in others]
        couts = [w[nm]["cout"] for nm in names]
        n, h, ww, _ = x.shape
        if not (self.h2 and self.stack_heads) or any(w[nm]["parts"] is not None for nm in names):
            if first is not None:
                self._conv(w, p + "." + first, x, first_out)
            return [self._conv(w, nm, x) for nm in names] + [None]
        with_pool = (pool is not None and first is not None and self.pool_after_conv and self.stack_pool_head
                     and w[p + "." + pool]["parts"] is None)
        key = ("stack", p, first, tuple(others), with_pool)
        st = w.get(key)
        if st is None:
            members = ([p + "." + first] if first is not None else []) + names
            # (an AVS_F16X2 row is packed by itself - runs of 8 inside the row: the stacked image is the rows one after another)
            rows = [w[nm]["w"].rows for nm in members]
            bias = [w[nm]["b"] for nm in members]
            if with_pool:
                rows.append(w[p + "." + pool]["w"].rows)
                bias.append(torch.zeros_like(w[p + "." + pool]["b"]))      # its bias comes after the pooling
            st = (_W(torch.cat(rows).contiguous()), torch.cat(bias).contiguous())
            w[key] = st
        wst, bst = st
        cpool = w[p + "." + pool]["cout"] if with_pool else 0
        tmp = torch.empty((n, h, ww, sum(couts) + cpool), dtype=self.dtype, device=x.device)
        wsel, layout = wst.conv_operand()
        if first is not None:
            ops.conv2d_split(x, wsel, first_out, w[p + "." + first]["cout"], tmp, bst, ops.ACT_RELU, w_layout=layout,
                             relu_cols=(wst.rows.shape[0] - cpool) if with_pool else 0)
        else:
            ops.conv2d(x, wsel, 1, 1, 1, (0, 0), tmp, bst, ops.ACT_RELU, split=self.f32_split, w_layout=layout)
        views, o = [], 0
        for c in couts:
            views.append(tmp[..., o:o + c])
            o += c
        views.append(tmp[..., o:o + cpool] if with_pool else None)
        return views

    def _pool_branch(self, w, name, x, out, z=None):
        """branch_pool = avg_pool2d(3, 1, 1) -> 1x1 conv -> folded BN -> ReLU, run as 1x1 conv (no bias) -> average ->
        + bias -> ReLU: the two linear maps commute (count_include_pad's zero padding included), and the pooling pass
        then moves cout (32-192) instead of cin (192-2048) channels."""
        if not self.pool_after_conv:
            return self._conv(w, name, self._pool(x, "avg", 3, 1, 1), out)
        c = w[name]
        n, h, ww, _ = x.shape
        if z is None:   # (else: the raw 1x1 output came out of the block's stacked-heads contraction)
            z = torch.empty((n, h, ww, c["cout"]), dtype=self.dtype, device=x.device)
            for a, b, wp, _ in (c["parts"] or [(0, c["cout"], c["w"], None)]):
                wsel, layout = wp.conv_operand()
                ops.conv2d(x, wsel, 1, 1, 1, (0, 0), z[..., a:b], None, ops.ACT_NONE, split=self.f32_split, w_layout=layout)
        return ops.pool2d(z, "avg", 3, 1, 1, out, c["b"], ops.ACT_RELU, code=self.ecode)

    def _pool(self, x, mode, k, s, p, out=None):
        n, h, ww, c = x.shape
        ho, wo = (h + 2 * p - k) // s + 1, (ww + 2 * p - k) // s + 1
        if out is None:
            out = torch.empty((n, ho, wo, c), dtype=self.dtype, device=x.device)
        return ops.pool2d(x, mode, k, s, p, out, code=self.ecode)

    def _cat_buffer(self, x, channels, stride=1):
        n, h, ww, _ = x.shape
        if stride == 2:
            h, ww = (h - 3) // 2 + 1, (ww - 3) // 2 + 1
        buf = torch.empty((n, h, ww, sum(channels)), dtype=self.dtype, device=x.device)
        offs = [0]
        for c in channels:
            offs.append(offs[-1] + c)
        return buf, [buf[..., offs[i]:offs[i + 1]] for i in range(len(channels))]

    def _block_a(self, w, p, x, pf):
        buf, (o1, o5, o3, op) = self._cat_buffer(x, [64, 64, 96, pf])
        t5, t3, zp = self._heads(w, p, x, "branch1x1", ["branch5x5_1", "branch3x3dbl_1"], o1, pool="branch_pool")
        self._conv(w, p + ".branch5x5_2", t5, o5)
        t = self._conv(w, p + ".branch3x3dbl_2", t3)
        self._conv(w, p + ".branch3x3dbl_3", t, o3)
        self._pool_branch(w, p + ".branch_pool", x, op, zp)
        return buf

    def _block_b(self, w, p, x):
        buf, (o3, od, op) = self._cat_buffer(x, [384, 96, x.shape[3]], stride=2)
        self._conv(w, p + ".branch3x3", x, o3)
        t = self._conv(w, p + ".branch3x3dbl_2", self._conv(w, p + ".branch3x3dbl_1", x))
        self._conv(w, p + ".branch3x3dbl_3", t, od)
        self._pool(x, "max", 3, 2, 0, op)
        return buf

    def _block_c(self, w, p, x):
        buf, (o1, o7, od, op) = self._cat_buffer(x, [192, 192, 192, 192])
        t7, td, zp = self._heads(w, p, x, "branch1x1", ["branch7x7_1", "branch7x7dbl_1"], o1, pool="branch_pool")
        t = self._conv(w, p + ".branch7x7_2", t7)
        self._conv(w, p + ".branch7x7_3", t, o7)
        t = td
        for i in (2, 3, 4):
            t = self._conv(w, f"{p}.branch7x7dbl_{i}", t)
        self._conv(w, p + ".branch7x7dbl_5", t, od)
        self._pool_branch(w, p + ".branch_pool", x, op, zp)
        return buf

    def _block_d(self, w, p, x):
        buf, (o3, o7, op) = self._cat_buffer(x, [320, 192, x.shape[3]], stride=2)
        t3, t7, _ = self._heads(w, p, x, None, ["branch3x3_1", "branch7x7x3_1"], None)
        self._conv(w, p + ".branch3x3_2", t3, o3)
        t = self._conv(w, p + ".branch7x7x3_2", t7)
        t = self._conv(w, p + ".branch7x7x3_3", t)
        self._conv(w, p + ".branch7x7x3_4", t, o7)
        self._pool(x, "max", 3, 2, 0, op)
        return buf

    def _block_e(self, w, p, x):
        buf, (o1, o3a, o3b, oda, odb, op) = self._cat_buffer(x, [320, 384, 384, 384, 384, 192])
        t, td, zp = self._heads(w, p, x, "branch1x1", ["branch3x3_1", "branch3x3dbl_1"], o1, pool="branch_pool")
        self._conv(w, p + ".branch3x3_2a", t, o3a)
        self._conv(w, p + ".branch3x3_2b", t, o3b)
        t = self._conv(w, p + ".branch3x3dbl_2", td)
        self._conv(w, p + ".branch3x3dbl_3a", t, oda)
        self._conv(w, p + ".branch3x3dbl_3b", t, odb)
        self._pool_branch(w, p + ".branch_pool", x, op, zp)
        return buf

    def forward(self, frames_u8, out=None):
        n, h, w_, _ = frames_u8.shape
        if (h, w_) != (299, 299):
            raise ValueError("InceptionV3Runner expects 299x299 frames (resize first)")
        if n == 0:
            return torch.zeros((0, 2048), dtype=torch.float32, device=frames_u8.device)
        w = self._prepare()
        dt, dev = self.dtype, frames_u8.device
        # (x/255 - mean)/std (extractors.py:151-153) then transform_input; one spare zero
        # pixel on the right so the stem's 4-pixel runs stay inside the row.
        affine = INCEPTION_TRANSFORM if self.net.transform_input else None
        x0 = ops.frames_normalize(frames_u8, dt, 255.0, RESNET_MEAN, RESNET_STD, 299, 300, 0, 0, affine, code=self.ecode)
        c = w["Conv2d_1a_3x3"]
        x = torch.empty((n, 149, 149, 32), dtype=dt, device=dev)
        wsel, layout = c["w"].conv_operand()
        ops.conv2d_raw(ops.dtype_code(dt, self.f32_split), n, 299, 149, 16, 3, 1, 2, 1, 0, 0, 149, 149, 32, x0, 299 * 300 * 4, 300 * 4, 8,
                       wsel, wsel.stride(0), x, 32, c["b"], ops.ACT_RELU, algo_k=27, algo_in_elems=x0.numel(),
                       w_layout=layout)
        del x0
        x = self._conv(w, "Conv2d_2a_3x3", x)
        x = self._conv(w, "Conv2d_2b_3x3", x)
        x = self._pool(x, "max", 3, 2, 0)
        x = self._conv(w, "Conv2d_3b_1x1", x)
        x = self._conv(w, "Conv2d_4a_3x3", x)
        x = self._pool(x, "max", 3, 2, 0)
        x = self._block_a(w, "Mixed_5b", x, 32)
        x = self._block_a(w, "Mixed_5c", x, 64)
        x = self._block_a(w, "Mixed_5d", x, 64)
        x = self._block_b(w, "Mixed_6a", x)
        for name in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
            x = self._block_c(w, name, x)
        x = self._block_d(w, "Mixed_7a", x)
        x = self._block_e(w, "Mixed_7b", x)
        x = self._block_e(w, "Mixed_7c", x)
        return ops.global_avgpool(x, out, code=self.ecode)
