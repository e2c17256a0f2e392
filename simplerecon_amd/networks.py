"""2-D networks of the hot path -- API/state-dict compatible with reference modules/networks.py:
`MLP` (:129-147), `CVEncoder` (:99-127), `DepthDecoderPP` (:20-96).

Activations flow between our layers as channels_last (NHWC-in-memory) torch tensors -- logically
still b,c,h,w, so callers see the reference's shapes -- and every BasicBlock writes straight into
its slice of the next concat buffer (no torch.cat copies)."""
import os

import numpy as np
import torch
from torch import nn

from .layers import BasicBlock


def double_basic_block(num_ch_in, num_ch_out, num_repeats=2):
    """Sequential(0: BasicBlock, conv_0: BasicBlock, ...) -- same child names as reference networks.py:13-17."""
    layers = nn.Sequential(BasicBlock(num_ch_in, num_ch_out))
    for i in range(num_repeats - 1):
        layers.add_module(f"conv_{i}", BasicBlock(num_ch_out, num_ch_out))
    return layers


class MLP(nn.Module):
    """Linear / LeakyReLU(0.01) stack (reference networks.py:129-147).  Inside the feature volume the
    three layers are fused into the HIP sweep kernel (cost_volume.FeatureVolumeManager reads
    `net.{0,2,4}.{weight,bias}`); calling the module directly applies the layers as written."""

    def __init__(self, channel_list, disable_final_activation=False):
        super().__init__()
        layer_list = []
        for i in range(len(channel_list) - 1):
            layer_list.append(nn.Linear(channel_list[i], channel_list[i + 1]))
            layer_list.append(nn.LeakyReLU(inplace=True))
        if disable_final_activation:
            layer_list = layer_list[:-1]
        self.net = nn.Sequential(*layer_list)

    def forward(self, x):
        """Applies the stack over the last dimension.  Device fp32 inputs run on the HIP 1x1 kernel with
        the LeakyReLU fused into each layer's epilogue."""
        from . import ops
        mods = list(self.net)
        i = 0
        while i < len(mods):
            lin = mods[i]
            act = mods[i + 1] if i + 1 < len(mods) and isinstance(mods[i + 1], nn.LeakyReLU) else None
            x = ops.linear(x, lin, leaky=act.negative_slope if act is not None else None)
            i += 2 if act is not None else 1
        return x


class LazyLevels:
    """A sequence of feature levels, each a tensor or a zero-argument callable that yields it -- a stream join (DepthModel's
    pending image-prior pyramid) or launches held back (CVEncoder's deferred last level).  `levels[i]` resolves a callable on
    first use and keeps the tensor; slices and sums are LazyLevels over the SAME items and resolve nothing, so a level is
    resolved once whoever asks first.  Indices are a list's, negative ones included.  A callable may carry the tensor it will
    yield as its `tensor` attribute, for peek()."""

    def __init__(self, items=(), cells=None):
        self._cells = [[x] for x in items] if cells is None else cells   # one shared cell per level

    @classmethod
    def of(cls, levels):
        return levels if isinstance(levels, cls) else cls(levels)

    def __len__(self):
        return len(self._cells)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return LazyLevels(cells=self._cells[i])
        cell = self._cells[i]
        if callable(cell[0]):
            cell[0] = cell[0]()
        return cell[0]

    def __add__(self, other):
        return LazyLevels(cells=self._cells + LazyLevels.of(other)._cells)

    def __radd__(self, other):
        return LazyLevels.of(other) + self

    def unresolved(self, i):
        return callable(self._cells[i][0])

    def peek(self):
        """The levels as far as their tensors are known (None otherwise), resolving nothing: for shapes, channel counts and
        requires_grad -- an unresolved level's tensor is not yet safe to launch work on."""
        return [getattr(x, "tensor", None) if callable(x) else x for x, in self._cells]


class CVEncoder(nn.Module):
    """Cost-volume + image-prior multi-scale encoder (reference networks.py:99-127)."""

    def __init__(self, num_ch_cv, num_ch_enc, num_ch_outs):
        super().__init__()
        self.convs = nn.ModuleDict()
        self.num_ch_enc = []
        self.num_blocks = len(num_ch_outs)
        self._img_ch = list(num_ch_enc)
        for i in range(self.num_blocks):
            num_ch_in = num_ch_cv if i == 0 else num_ch_outs[i - 1]
            num_ch_out = num_ch_outs[i]
            self.convs[f"ds_conv_{i}"] = BasicBlock(num_ch_in, num_ch_out, stride=1 if i == 0 else 2)
            self.convs[f"conv_{i}"] = nn.Sequential(
                BasicBlock(num_ch_enc[i] + num_ch_out, num_ch_out, stride=1),
                BasicBlock(num_ch_out, num_ch_out, stride=1),
            )
            self.num_ch_enc.append(num_ch_out)

    def _forward_train(self, x, img_feats):
        """Differentiable forward (reference networks.py:120-127 as written: concat with torch.cat, which autograd
        splits again on the way back); every conv runs autograd_ops (HIP forward + backward)."""
        outputs = []
        for i in range(self.num_blocks):
            x = self.convs[f"ds_conv_{i}"](x)
            x = self.convs[f"conv_{i}"](torch.cat([x, img_feats[i]], dim=1))
            outputs.append(x)
        return outputs

    def forward(self, x, img_feats, defer_last=False):
        """Returns the `num_blocks` levels as a LazyLevels.  defer_last=True (inference only) leaves the last one unresolved:
        its ds_conv is already launched; resolving it takes the deepest image-prior level and runs the two blocks that need it.
        DepthDecoderPP first launches everything that does not depend on it."""
        from . import autograd_ops, ops
        # `img_feats` may be DepthModel's pending pyramid: taking level i then joins the image-prior encoder's side stream just
        # far enough for it -- AFTER ds_conv_i has been launched, which does not need it
        img_feats = LazyLevels.of(img_feats)
        peek = img_feats.peek()
        if autograd_ops.grad_wanted(x, peek, self):
            return LazyLevels(self._forward_train(x, list(img_feats)))
        outputs = []
        for i in range(self.num_blocks):
            ds = self.convs[f"ds_conv_{i}"]
            c_out = ds.conv2.out_channels
            ho, wo = ops.conv_out_hw(x.shape[2], x.shape[3], ds.stride)
            # concat buffer [x | img_feats[i]] (reference networks.py:124): ds_conv writes its slice in place
            buf = ops.empty_nhwc(x.shape[0], c_out + peek[i].shape[1], ho, wo, x.device)
            ds(x, out=buf[:, :c_out])

            def finish(i=i, buf=buf, c_out=c_out):
                ops.copy_into(buf[:, c_out:], img_feats[i])
                return self.convs[f"conv_{i}"][1](self.convs[f"conv_{i}"][0](buf))
            x = finish if defer_last and i == self.num_blocks - 1 else finish()
            outputs.append(x)
        return LazyLevels(outputs)


_SIDE_STREAMS = {}  # device -> (stream, stream) for DepthDecoderPP's branch parallelism


class DepthDecoderPP(nn.Module):
    """UNet++ depth decoder (reference networks.py:20-96).  Output heads that the reference evaluates
    and then overwrites (`output_i` is recomputed at every node j, the last one wins, networks.py:92)
    are evaluated once, at the node whose value survives."""

    def __init__(self, num_ch_enc, scales=range(4), num_output_channels=1, use_skips=True):
        super().__init__()
        self.num_output_channels = num_output_channels
        self.use_skips = use_skips
        self.upsample_mode = "nearest"
        self.scales = scales
        self.num_ch_enc = num_ch_enc
        self.num_ch_dec = np.array([64, 64, 128, 256])
        self.convs = nn.ModuleDict()
        for j in range(1, 5):
            max_i = 4 - j
            for i in range(max_i, -1, -1):
                num_ch_out = int(self.num_ch_dec[i])
                total = 0
                num_ch_in = int(self.num_ch_enc[i + 1] if j == 1 else self.num_ch_dec[i + 1])
                self.convs[f"diag_conv_{i + 1}{j - 1}"] = BasicBlock(num_ch_in, num_ch_out)
                total += num_ch_out
                num_ch_in = int(self.num_ch_enc[i] if j == 1 else self.num_ch_dec[i])
                self.convs[f"right_conv_{i}{j - 1}"] = BasicBlock(num_ch_in, num_ch_out)
                total += num_ch_out
                if i + j != 4:
                    num_ch_in = int(self.num_ch_dec[i + 1])
                    self.convs[f"up_conv_{i + 1}{j}"] = BasicBlock(num_ch_in, num_ch_out)
                    total += num_ch_out
                self.convs[f"in_conv_{i}{j}"] = double_basic_block(total, num_ch_out)
                self.convs[f"output_{i}"] = nn.Sequential(
                    BasicBlock(num_ch_out, num_ch_out) if i != 0 else nn.Identity(),
                    nn.Conv2d(num_ch_out, self.num_output_channels, 1),
                )

    # The three inputs of a node (right / diagonal / up branch) are independent BasicBlocks writing disjoint channel
    # slices of the node's concat buffer; `_launch_branches` launches any of them, and its order is the schedule:
    #   forked    diagonal on side stream 1, up on side stream 2, then right on the main stream; `forward` joins the side
    #             streams that were used before `in_conv`
    #   in order  right, diagonal, up on the current stream
    # A node forks (`_node_buffer`) at small batch, where a single conv launch leaves CUs idle (150-600 work items for
    # 512 slots): batches <= `branch_stream_max_batch`.  At batch 8 the 240x320 launches fill the chip and the fork / join
    # only costs, but the nodes from 120x160 down (<= 1200 of the convs' 8x16-pixel regions for 512 workgroup slots, their
    # diagonal / up branches a quarter of that) leave part of it idle: those fork at any batch (`branch_stream_max_regions`,
    # 0 = off; measured r02 at batch 8: 32.3 -> 32.0 ms per step with 1300, nothing with 400, nothing more with 5000).
    # When the deepest input is still unresolved, the first column's nodes that do not read it are launched in two calls:
    # right / diagonal before it is resolved (forked or in order), the up branch afterwards in order -- by then nothing is
    # left for the main stream to run beside it, so a third stream's fork / join would only cost.
    branch_stream_max_batch = 2
    branch_stream_max_regions = int(os.environ.get("SR_DECODER_FORK_REGIONS", "1300"))

    @staticmethod
    def _side_streams(device):
        if device not in _SIDE_STREAMS:  # process-wide, so modules stay picklable / deep-copyable
            _SIDE_STREAMS[device] = (torch.cuda.Stream(device=device), torch.cuda.Stream(device=device))
        return _SIDE_STREAMS[device]

    def _forward_train(self, input_features):
        """Differentiable forward: the UNet++ graph of reference networks.py:75-96 on autograd_ops (torch.cat for the
        concats, the HIP bilinear x2 with its adjoint); the head evaluations the reference overwrites are skipped
        (they receive no gradient there either)."""
        from . import autograd_ops
        prev_outputs, outputs, depth_outputs = list(input_features), [], {}
        for j in range(1, 5):
            for i in range(4 - j, -1, -1):
                parts = [self.convs[f"right_conv_{i}{j - 1}"](prev_outputs[i]),
                         autograd_ops.upsample2x(self.convs[f"diag_conv_{i + 1}{j - 1}"](prev_outputs[i + 1]))]
                if i + j != 4:
                    parts.append(autograd_ops.upsample2x(self.convs[f"up_conv_{i + 1}{j}"](outputs[-1])))
                output = self.convs[f"in_conv_{i}{j}"](torch.cat(parts, dim=1))
                outputs.append(output)
                if i + j == 4:
                    head = self.convs[f"output_{i}"]
                    hx = output if isinstance(head[0], nn.Identity) else head[0](output)
                    depth_outputs[f"log_depth_pred_s{i}_b1hw"] = autograd_ops.conv_bias_act(hx, head[1])
            prev_outputs = outputs[::-1]
        return {k: depth_outputs[k] for k in sorted(depth_outputs, reverse=True)}

    def _node_buffer(self, i, j, x, streams):
        """(concat buffer of node (i, j), whose right input is `x`; the streams its branches fork over, or None: in order)."""
        from . import ops
        b, _, h, w = x.shape
        buf = ops.empty_nhwc(b, int(self.num_ch_dec[i]) * (3 if i + j != 4 else 2), h, w, x.device)
        regions = b * ((h + 7) // 8) * ((w + 15) // 16)
        fork = streams is not None and (b <= self.branch_stream_max_batch or regions <= self.branch_stream_max_regions)
        return buf, streams if fork else None

    def _launch_branches(self, i, j, buf, right=None, diag=None, up=None, fork=None):
        """Launches the branches of node (i, j) whose inputs are given, each into its channel slice of `buf`.  `fork` = (main,
        side 1, side 2): diagonal and up go out first, on their side streams behind the main stream's work so far, and are
        in flight beside the right branch; None: right, diagonal, up on the current stream.  Returns the side streams used."""
        from . import ops
        c = int(self.num_ch_dec[i])
        upsampled = [(name, x, k) for k, name, x in ((1, f"diag_conv_{i + 1}{j - 1}", diag), (2, f"up_conv_{i + 1}{j}", up))
                     if x is not None]
        for name, x, k in upsampled if fork else ():   # branch k on side stream k
            fork[k].wait_stream(fork[0])
            with torch.cuda.stream(fork[k]):
                ops.upsample2x(self.convs[name](x), out=buf[:, k * c:(k + 1) * c])
        if right is not None:
            self.convs[f"right_conv_{i}{j - 1}"](right, out=buf[:, :c])
        for name, x, k in () if fork else upsampled:
            ops.upsample2x(self.convs[name](x), out=buf[:, k * c:(k + 1) * c])
        return [fork[k] for _, _, k in upsampled] if fork else []

    def forward(self, input_features):
        """`input_features` may be a LazyLevels.  With a gradient wanted, everything is resolved for `_forward_train`.  Otherwise,
        when the deepest level is still unresolved (CVEncoder.forward(defer_last=True)), the first column launches the right /
        diagonal branches of the nodes that do not read it BEFORE resolving it -- that may join the image-prior encoder's stream,
        and those branches (the full-resolution convolutions among them) run while the encoder finishes.  Same launches, same
        inputs: the result does not change."""
        from . import autograd_ops, ops
        feats = LazyLevels.of(input_features)
        if autograd_ops.grad_wanted(feats.peek(), self):
            return self._forward_train(list(feats))
        prev_outputs = list(feats[:-1])
        outputs = []
        depth_outputs = {}
        dev = prev_outputs[0].device
        streams = (torch.cuda.current_stream(dev), *self._side_streams(dev)) if dev.type == "cuda" else None
        early = {}   # node i of column 1 -> (buf, side streams used) whose right / diagonal branches are already launched
        if feats.unresolved(-1):
            for i in range(len(prev_outputs) - 2, -1, -1):
                buf, fork = self._node_buffer(i, 1, prev_outputs[i], streams)
                early[i] = buf, self._launch_branches(i, 1, buf, prev_outputs[i], prev_outputs[i + 1], fork=fork)
        prev_outputs.append(feats[-1])
        for j in range(1, 5):
            for i in range(4 - j, -1, -1):
                up = outputs[-1] if i + j != 4 else None
                if i in early:
                    buf, used = early.pop(i)
                    self._launch_branches(i, j, buf, up=up)
                else:
                    buf, fork = self._node_buffer(i, j, prev_outputs[i], streams)
                    used = self._launch_branches(i, j, buf, prev_outputs[i], prev_outputs[i + 1], up, fork)
                for side in used:
                    streams[0].wait_stream(side)
                in_conv = self.convs[f"in_conv_{i}{j}"]
                output = in_conv[1](in_conv[0](buf))
                outputs.append(output)
                if i + j == 4:  # last node of scale i: the head value the reference keeps
                    head = self.convs[f"output_{i}"]
                    hx = output if isinstance(head[0], nn.Identity) else head[0](output)
                    depth_outputs[f"log_depth_pred_s{i}_b1hw"] = ops.conv2d(hx, head[1])
            prev_outputs = outputs[::-1]
        # same key order as the reference's dict (s3, s2, s1, s0 first inserted at j = 1)
        return {k: depth_outputs[k] for k in sorted(depth_outputs, reverse=True)}


class _BlurPool(nn.Module):
    """Parameter/buffer holder for antialiased_cnns.BlurPool(filt_size=4, stride=2) -- keeps the `filt` buffer so
    reference checkpoints load; the HIP kernel uses the fixed outer([1,3,3,1])/64 taps."""

    def __init__(self, channels, filt_size=4, stride=2):
        super().__init__()
        if filt_size != 4 or stride != 2:
            raise ValueError("the HIP path implements BlurPool(filt_size=4, stride=2) only")
        a = torch.tensor([1.0, 3.0, 3.0, 1.0])
        filt = a[:, None] * a[None, :]
        self.register_buffer("filt", (filt / filt.sum())[None, None].repeat(channels, 1, 1, 1))


class _ResnetBlock(nn.Module):
    """Holder for a stride-1 ResNet-18 BasicBlock (conv1, bn1, conv2, bn2)."""

    def __init__(self, planes):
        super().__init__()
        self.conv1 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)


class ResnetMatchingEncoder(nn.Module):
    """Matching-feature encoder (reference networks.py:149-205): antialiased ResNet-18 stem + layer1, then
    conv1x1 64->128, InstanceNorm, LeakyReLU(0.2), conv3x3 128->num_ch_out (replicate padding), InstanceNorm.

    `net` has the reference's nn.Sequential numbering (net.0 conv1, net.1 bn1, net.3.1 blur, net.4 layer1,
    net.5 / net.8 tail convs) so its checkpoints load unchanged.  Inference (eval mode, no gradient wanted): BatchNorm
    uses running statistics folded into the conv weights at pack time, fused kernels.  Training: `_forward_train`, the
    same graph on differentiable operators, BatchNorm per its own mode.  The backbone definition follows the public
    antialiased_cnns package, which is not available here -- parity for it is pinned against a torch.nn
    restatement only (oracle/refshim.py)."""

    def __init__(self, num_layers=18, num_ch_out=16, pretrained=False, antialiased=True):
        super().__init__()
        if num_layers != 18:
            raise ValueError("{} is not a valid number of resnet layers".format(num_layers)
                             if num_layers not in (34, 50, 101, 152) else
                             "the HIP path implements the 18-layer backbone (what SimpleRecon uses)")
        if not antialiased:
            raise ValueError("the HIP path implements the antialiased backbone (what SimpleRecon uses)")
        if pretrained:
            raise ValueError("pretrained backbone weights are not downloadable here; load a state_dict instead")
        self.num_ch_enc = np.array([64, 64])
        self.num_ch_out = num_ch_out
        self.net = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False),
            nn.BatchNorm2d(64),
            nn.ReLU(inplace=True),
            nn.Sequential(nn.MaxPool2d(kernel_size=2, stride=1), _BlurPool(64)),
            nn.Sequential(_ResnetBlock(64), _ResnetBlock(64)),
            nn.Conv2d(64, 128, (1, 1)),
            nn.InstanceNorm2d(128),
            nn.LeakyReLU(0.2, True),
            nn.Conv2d(128, num_ch_out, (3, 3), padding=1, padding_mode="replicate"),
            nn.InstanceNorm2d(num_ch_out),
        )

    def forward_pair(self, cur_image, src_image):
        """Features of a batch of reference images [B,3,H,W] and their source images [B,K,3,H,W] in ONE pass over
        B(1+K) images without concatenating the images first: the stem writes both groups into one buffer (every
        later layer is per image -- eval BatchNorm, InstanceNorm -- so the order inside the batch is free).
        Returns (cur_feats [B,C,h,w], src_feats [B,K,C,h,w])."""
        from . import ops
        b, k = src_image.shape[:2]
        h, w = cur_image.shape[-2:]
        if self._train_path(cur_image, src_image):
            # training: one batch of B(1+K) images like the reference's TensorFormatter call (depth_model.py:234-240);
            # BatchNorm statistics run over all of them
            feats = self._forward_train(torch.cat([cur_image.unsqueeze(1), src_image], dim=1).flatten(0, 1))
            feats = feats.unflatten(0, (b, 1 + k))
            return feats[:, 0], feats[:, 1:]
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        stem = ops.empty_nhwc(b * (1 + k), 64, ho, wo, cur_image.device)
        ops.stem7x7(cur_image, self.net[0], self.net[1], out=stem[:b])
        ops.stem7x7(src_image.reshape(b * k, *src_image.shape[2:]), self.net[0], self.net[1], out=stem[b:])
        feats = self._after_stem(stem)
        return feats[:b], feats[b:].unflatten(0, (b, k))

    def _train_path(self, *tensors):
        """Training / differentiable path: autograd is recording and something wants a gradient, or a BatchNorm layer is
        in training mode (batch statistics cannot be folded into the conv weights)."""
        from . import autograd_ops
        return autograd_ops.grad_wanted(list(tensors), self) or autograd_ops.any_batchnorm_training(self)

    def _forward_train(self, image):
        """The reference's nn.Sequential (networks.py:176-201) operator by operator on the differentiable HIP operators
        of train_ops: conv1 -> bn1 (batch statistics when the layer is in training mode) + ReLU -> MaxPool(2,1) +
        BlurPool -> layer1 (two BasicBlocks with BatchNorm) -> conv1x1 -> InstanceNorm + LeakyReLU -> replicate-padded
        conv3x3 -> InstanceNorm."""
        from . import train_ops as T
        net = self.net
        x = T.stem7x7(image, net[0])
        x = T.batch_norm_act(x, net[1], act=0.0)
        x = T.maxblurpool(x)
        for blk in net[4]:
            t = T.batch_norm_act(T.conv(x, blk.conv1), blk.bn1, act=0.0)
            t = T.batch_norm_act(T.conv(t, blk.conv2), blk.bn2)
            x = T.add(t, x, act=0.0)
        x = T.conv(x, net[5])
        x = T.instance_norm_act(x, eps=net[6].eps, leaky=net[7].negative_slope)
        x = T.conv(T.replicate_pad(x, 1), net[8], pads=(0, 0, 0, 0))
        return T.instance_norm_act(x, eps=net[9].eps)

    def forward(self, input_image):
        """input_image [B,3,H,W] (H, W multiples of 4) -> [B,num_ch_out,H/4,W/4] (channels_last memory)."""
        from . import ops
        if self._train_path(input_image):
            return self._forward_train(input_image)
        return self._after_stem(ops.stem7x7(input_image, self.net[0], self.net[1]))   # conv1 + bn1 + relu

    def _after_stem(self, x):
        from . import ops
        net = self.net
        x = ops.maxblurpool(x)                                              # MaxPool(2,1) + BlurPool(4,2)
        for blk in net[4]:
            t = ops.conv2d(x, blk.conv1, bn=blk.bn1, leaky=0.0)
            x = ops.conv2d(t, blk.conv2, bn=blk.bn2, residual=x, leaky=0.0)
        fused_in = net[8].out_channels <= 16 and net[8].in_channels % 32 == 0
        if fused_in and (net[5].in_channels, net[5].out_channels) == (64, 128):
            # the 1x1 conv leaves the InstanceNorm statistics of its output behind (no separate pass over it) ...
            x, stats = ops.conv1x1_stats(x, net[5], eps=net[6].eps)
            x = ops.conv3x3_c16(x, net[8], in_stats=stats, in_leaky=net[7].negative_slope)
        elif fused_in:
            # ... and InstanceNorm + LeakyReLU of the 128-channel map are applied inside the last conv's input
            # staging: the normalised tensor never goes to HBM
            x = ops.conv2d(x, net[5])
            stats = ops.instance_norm_stats(x, eps=net[6].eps)
            x = ops.conv3x3_c16(x, net[8], in_stats=stats, in_leaky=net[7].negative_slope)
        else:
            x = ops.conv2d(x, net[5])
            x = ops.instance_norm(x, eps=net[6].eps, leaky=net[7].negative_slope, inplace=True)
            x = ops.conv2d(x, net[8])
        return ops.instance_norm(x, eps=net[9].eps, inplace=True)
