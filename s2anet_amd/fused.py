"""Convolution with a fused epilogue: MIOpen runs the convolution itself (the carrier, SURVEY.md
#13), the bias / residual / ReLU that follow it are ONE in-place HIP pass (s2a_bias_act_nhwc)
instead of up to three stock elementwise kernels.  Parameter names stay ``weight`` / ``bias`` so
reference state_dicts load unchanged."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def bias_act_(y, bias, residual=None, relu=False, out=None):
    """y = act(y + bias[c] (+ residual)): in place in ONE pass (s2a_bias_act_nhwc) when y is channels-last contiguous
    with whole 16-byte channel vectors, stock ops otherwise.
    out: a dense NHWC buffer of y's shape that receives the result instead (e.g. a level slice of a pyramid-packed tensor).
    The raw pass writes through a pointer, which autograd cannot see: when grad is enabled and y, bias or residual
    requires grad, the stock ops run instead (bias gradient, ReLU mask and residual gradient are autograd's), whatever
    the layout, and out= is refused."""
    _lib.require_cuda(y, bias, residual)
    B, C, H, W = y.shape
    if out is not None:
        assert out.shape == y.shape and out.dtype == y.dtype and out.permute(0, 2, 3, 1).is_contiguous()
    grad = _needs_grad(y, bias, residual)
    if grad and out is not None:
        raise RuntimeError("bias_act_(out=...) writes a caller's buffer and has no backward: call it under torch.no_grad()")
    ok = (not grad and y.is_contiguous(memory_format=torch.channels_last) and
          C % (8 if y.dtype == torch.float16 else 4) == 0 and y.dtype in (torch.float16, torch.float32) and
          (residual is None or (residual.shape == y.shape and residual.dtype == y.dtype and
                                residual.is_contiguous(memory_format=torch.channels_last))))
    if not ok:      # odd channel count / NCHW storage / a gradient is wanted: stock ops (still on the GPU)
        y = y + bias.view(1, -1, 1, 1).to(y.dtype)
        if residual is not None:
            y = y + residual
        y = F.relu(y) if relu else y
        return y if out is None else out.copy_(y)
    return _bias_act_raw(y, bias, residual, relu, out)


def _bias_act_raw(y, bias, residual=None, relu=False, out=None):
    """the one-pass epilogue itself, no checks: writes y (or out) through its pointer, invisible to autograd"""
    B, C, H, W = y.shape
    b = bias if bias.dtype == y.dtype and bias.is_contiguous() else bias.to(y.dtype).contiguous()
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().s2a_bias_act_nhwc_to(_lib.ptr(y), _lib.ptr(b), _lib.ptr(residual),
                                                   _lib.ptr(y if out is None else out), B * H * W, C,
                                                   _lib.dtype_code(y), int(bool(relu)), _lib.stream_ptr(y.device)))
    return y if out is None else out


def own_conv_ok(x, in_channels, out_channels, kernel_size, stride, padding, dilation, groups):
    """shapes the patch-staged MFMA convolution (s2a_conv_nhwc_f16) handles AND wins on (measured on
    MI355X, scripts/bench_ops.py --which convbb): 3x3/s1/p1 or 1x1/p0 (stride 1 or 2), f16
    channels-last, channel counts multiples of 64, enough position tiles to fill the chip"""
    import os
    if not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and
            x.is_contiguous(memory_format=torch.channels_last) and tuple(dilation) == (1, 1) and groups == 1 and
            (in_channels % 64 == 0 or in_channels == 32) and (out_channels % 64 == 0 or out_channels < 64) and
            x.numel() * 2 < (1 << 31)):
        return False
    if os.environ.get("S2A_NO_OWN_CONV"):
        return False
    k, st, pd = tuple(kernel_size), tuple(stride), tuple(padding)
    B, _, H, W = x.shape
    # S2A_OWN_CONV_ALWAYS=1: every shape the kernel handles, also the small grids the library wins on (the size
    # thresholds below are speed heuristics, not limits) -- a network evaluated this way runs no library convolution
    # in the trunk and is therefore bit-reproducible run to run and box to box (tests/test_net_forward.py)
    narrow = out_channels < 64 or bool(os.environ.get("S2A_OWN_CONV_ALWAYS"))
    #         ^ prediction heads (5 / 15 maps): the library's kernels for these cost 13-56 us flat
    if k == (3, 3) and st == (1, 1) and pd == (1, 1):
        return narrow or B * ((H + 7) // 8) * ((W + 15) // 16) >= 64
    if k == (3, 3) and st == (2, 2) and pd == (1, 1) and not os.environ.get("S2A_NO_OWN_CONV_S2"):
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1            # the down-sampling conv2 of a stage's first bottleneck
        return out_channels % 128 == 0 and in_channels % 64 == 0 and (narrow or B * ((Ho + 3) // 4) * ((Wo + 15) // 16) >= 128)
    if k == (1, 1) and pd == (0, 0) and st in ((1, 1), (2, 2)) and not os.environ.get("S2A_NO_OWN_CONV1"):
        Ho, Wo = (H - 1) // st[0] + 1, (W - 1) // st[1] + 1
        return narrow or B * Ho * Wo >= 64 * 128
    return False


def conv_pack_weight(weight):
    """[O,C,k,k] -> MFMA-fragment order (s2a_conv_pack_weight_f16); fewer than 64 filters are
    zero-padded to 64 (the kernel's narrowest output group)"""
    w = weight.detach().to(torch.float16).contiguous()
    if w.shape[0] < 64:
        w = torch.cat([w, w.new_zeros((64 - w.shape[0],) + tuple(w.shape[1:]))], 0).contiguous()
    if w.shape[1] == 32:            # 32 input maps (odm_cls_ls after the orientation pooling): zero-pad to one 64-chunk
        w = torch.cat([w, torch.zeros_like(w)], 1).contiguous()
    out = torch.empty_like(w)
    with torch.cuda.device(w.device):
        _lib.check(_lib.lib().s2a_conv_pack_weight_f16(_lib.ptr(w), w.shape[0], w.shape[1], w.shape[2],
                                                       _lib.ptr(out), _lib.stream_ptr(w.device)))
    return out


def conv_pack_weight_fp8(weight, in_scale):
    """[O,C,3,3] -> (the e4m3 filter in the fragment order of s2a_conv3x3_pyramid_fp8, uint8 [O*C*9];
    scale f32[O] = in_scale * s_w[o]): per-output-channel quantisation (fp8.quantize_weight_e4m3) + a byte permutation"""
    from .fp8 import quantize_weight_e4m3
    wq, s_w = quantize_weight_e4m3(weight)
    O, C = wq.shape[:2]
    assert tuple(wq.shape[2:]) == (3, 3) and O % 64 == 0 and C % 128 == 0
    out = torch.empty((wq.numel(),), dtype=torch.uint8, device=wq.device)
    with torch.cuda.device(wq.device):
        _lib.check(_lib.lib().s2a_conv_pack_weight_fp8(_lib.ptr(wq), O, C, _lib.ptr(out), _lib.stream_ptr(wq.device)))
    return out, (s_w * float(in_scale)).contiguous()


def conv_wino_pack_weight(weight):
    """[O,C,3,3] -> the transformed filter of the Winograd F(2,3) kernel in fragment order (s2a_conv_wino_pack_weight_f16);
    O a multiple of 64, C a multiple of 32"""
    w = weight.detach().to(torch.float16).contiguous()
    O, C = w.shape[:2]
    assert tuple(w.shape[2:]) == (3, 3) and O % 64 == 0 and C % 32 == 0
    L = _lib.lib()
    out = torch.empty((L.s2a_conv_wino_packed_elems(O, C),), dtype=torch.float16, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(L.s2a_conv_wino_pack_weight_f16(_lib.ptr(w), O, C, _lib.ptr(out), _lib.stream_ptr(w.device)))
    return out


def conv_wino_f16(x, packed_wino, bias, out_channels, relu=False, pool=False):
    """relu?(conv3x3(x) + bias) on a plain channels-last tensor through the Winograd kernel (one-level pyramid)"""
    from .pyramid import PyramidLayout, conv3x3_wino
    B, C, H, W = x.shape
    assert x.dtype == torch.float16 and x.is_contiguous(memory_format=torch.channels_last)
    lay = PyramidLayout(B, [(H, W)], [1.0])
    b = None if bias is None else bias.to(torch.float16).contiguous()
    r = conv3x3_wino(lay, x.permute(0, 2, 3, 1).reshape(-1, C), packed_wino, b, out_channels, relu, pool)
    if pool:
        return (r[0].view(B, H, W, out_channels).permute(0, 3, 1, 2), r[1].view(B, H, W, out_channels // 8).permute(0, 3, 1, 2))
    return r.view(B, H, W, out_channels).permute(0, 3, 1, 2)


def conv_f16(x, packed_weight, bias, out_channels, ksize, stride=1, relu=False, residual=None, out=None, chain=None):
    """relu?(conv(x) + bias (+ residual)) in ONE kernel; x f16 channels-last, packed_weight from
    conv_pack_weight; ksize 3 (pad 1, stride 1|2) or 1 (pad 0, stride 1|2).
    chain = a Conv3Chain (this launch is a bottleneck's conv3, chain.conv the next block's conv1, conv3_chain_ok):
    the same launch also leaves relu(conv1(result)) in chain.out (s2a_conv1x1_chain_f16); the return value is the same
    tensor, bit for bit, as without it"""
    B, C, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    O_real = out_channels
    if out_channels < 64:           # narrow head: 64 physical channels, the caller gets the [:, :O] view
        assert residual is None
        out_channels = 64
    if out is None:
        out = torch.empty((B, out_channels, Ho, Wo), dtype=torch.float16, device=x.device,
                          memory_format=torch.channels_last)
    else:       # caller's buffer (e.g. a level slice of a pyramid-packed tensor): dense NHWC storage required
        assert out.shape == (B, out_channels, Ho, Wo) and out.dtype == torch.float16 and \
            out.permute(0, 2, 3, 1).is_contiguous()
    b = None if bias is None else bias.to(torch.float16).contiguous()
    if b is not None and b.numel() < out_channels:
        b = torch.cat([b, b.new_zeros(out_channels - b.numel())])
    if residual is not None:
        assert residual.shape == out.shape and residual.dtype == torch.float16 and \
            residual.is_contiguous(memory_format=torch.channels_last)
    if chain is not None and ksize == 1 and stride == 1 and relu and b is not None and \
            (C, out_channels, chain.conv.out_channels) in CONV3_CHAIN_SHAPES and out.numel() * 2 < (1 << 31):
        wc, bc, _ = chain.conv.packed_args()
        chain.out = torch.empty((B, chain.conv.out_channels, H, W), dtype=torch.float16, device=x.device,
                                memory_format=torch.channels_last)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().s2a_conv1x1_chain_f16(_lib.ptr(x), _lib.ptr(packed_weight), _lib.ptr(b), _lib.ptr(residual),
                                                        _lib.ptr(out), _lib.ptr(wc), _lib.ptr(bc), _lib.ptr(chain.out),
                                                        chain.conv.out_channels, B, C, out_channels, H, W,
                                                        _lib.stream_ptr(x.device)))
        return out
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().s2a_conv_nhwc_f16(_lib.ptr(x), _lib.ptr(packed_weight), _lib.ptr(b), _lib.ptr(residual),
                                                _lib.ptr(out), B, C, H, W, out_channels, int(ksize), int(stride),
                                                int(bool(relu)), _lib.stream_ptr(x.device)))
    return out if O_real == out_channels else out[:, :O_real]


# (conv3 in, conv3 out, next conv1 out) the chained kernel is built for: layer2's blocks, layer2 -> layer3.0, layer3's
# blocks.  (256, 1024, 512), layer3 -> layer4.0, does not fit the register file without scratch (docs/HISTORY.md)
CONV3_CHAIN_SHAPES = {(128, 512, 128), (128, 512, 256), (256, 1024, 256)}


class Conv3Chain:
    """the next bottleneck's conv1 riding on a conv3 launch: conv = that FusedConv2d; out = its result, filled by
    conv_f16 when the launch really chained it (None otherwise: the caller runs conv1 itself)"""

    def __init__(self, conv):
        self.conv, self.out = conv, None


def conv3_chain_ok(conv3, conv1):
    """the next block's conv1 can ride on this block's conv3 launch (s2a_conv1x1_chain_f16): both 1x1 / stride 1 with
    bias and ReLU, f16, conv1 reading what conv3 writes, a (K, O, O3) the kernel is built for, inference only"""
    import os
    def plain(c):
        return (isinstance(c, FusedConv2d) and tuple(c.kernel_size) == (1, 1) and tuple(c.stride) == (1, 1) and
                tuple(c.padding) == (0, 0) and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.bias is not None and
                c.fuse_relu and c.weight.dtype == torch.float16)
    return (not torch.is_grad_enabled() and not os.environ.get("S2A_NO_CONV3_CHAIN") and plain(conv3) and plain(conv1) and
            conv1.in_channels == conv3.out_channels and
            (conv3.in_channels, conv3.out_channels, conv1.out_channels) in CONV3_CHAIN_SHAPES)


def bottleneck_tail_ok(x, conv2, conv3, residual):
    """the 64 -> 64 (3x3/s1) -> 256 (1x1) tail of a layer-1 bottleneck fits s2a_conv3x3_tail1x1_f16"""
    import os
    return (not torch.is_grad_enabled() and not os.environ.get("S2A_NO_FUSED_TAIL") and
            isinstance(conv2, FusedConv2d) and isinstance(conv3, FusedConv2d) and
            conv2.in_channels == 64 and conv2.out_channels == 64 and conv3.out_channels == 256 and
            conv2.fuse_relu and conv3.fuse_relu and conv2.bias is not None and conv3.bias is not None and
            own_conv_ok(x, 64, 64, conv2.kernel_size, conv2.stride, conv2.padding, conv2.dilation, conv2.groups) and
            tuple(conv2.kernel_size) == (3, 3) and tuple(conv2.stride) == (1, 1) and
            tuple(conv3.kernel_size) == (1, 1) and tuple(conv3.stride) == (1, 1) and
            x.shape[0] * x.shape[2] * x.shape[3] * 512 < (1 << 31) and
            (residual is None or (residual.dtype == torch.float16 and residual.shape[1] == 256 and
                                  residual.shape[2:] == x.shape[2:] and
                                  residual.is_contiguous(memory_format=torch.channels_last))))


def bottleneck_chain_ok(conv1):
    """the next block's conv1 can ride on the tail kernel: 1x1, 256 -> 64 (same stage) or 128 (first block of the
    next stage), bias, ReLU"""
    import os
    return (isinstance(conv1, FusedConv2d) and not os.environ.get("S2A_NO_TAIL_CHAIN") and
            conv1.in_channels == 256 and conv1.out_channels in (64, 128) and tuple(conv1.kernel_size) == (1, 1) and
            tuple(conv1.stride) == (1, 1) and tuple(conv1.padding) == (0, 0) and conv1.groups == 1 and
            conv1.fuse_relu and conv1.bias is not None and conv1.weight.dtype == torch.float16)


def bottleneck_tail(x, conv2, conv3, residual=None, chain=None):
    """relu(conv3(relu(conv2(x))) + residual) in ONE kernel (models/backbone.py:72-83, BN folded): the 64-map
    intermediate stays in LDS; bit-identical to the two separate launches.  chain = the NEXT bottleneck's conv1
    (bottleneck_chain_ok): its output relu(conv1(out)) is produced by the same launch -> returns (out, next_conv1_out)"""
    B, C, H, W = x.shape
    out = torch.empty((B, 256, H, W), dtype=torch.float16, device=x.device, memory_format=torch.channels_last)
    w2, b2, _ = conv2.packed_args()
    w3, b3, _ = conv3.packed_args()
    wc = bc = nxt = None
    if chain is not None:
        wc, bc, _ = chain.packed_args()
        nxt = torch.empty((B, chain.out_channels, H, W), dtype=torch.float16, device=x.device,
                          memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().s2a_conv3x3_tail1x1_f16(_lib.ptr(x), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(w3), _lib.ptr(b3),
                                                      _lib.ptr(residual), _lib.ptr(out), _lib.ptr(wc), _lib.ptr(bc),
                                                      _lib.ptr(nxt), 0 if chain is None else chain.out_channels,
                                                      B, 64, 64, 256, H, W, _lib.stream_ptr(x.device)))
    return out if chain is None else (out, nxt)


def conv1x1_add_up2(x, packed_weight, bias, coarse, out_channels):
    """FPN top-down step (models/neck.py:67-79) in one launch:
    conv1x1(x) + bias + nearest-2x-upsample(coarse); x[B,C,H,W], coarse[B,O,H/2,W/2] f16 channels-last"""
    B, C, H, W = x.shape
    assert coarse.shape == (B, out_channels, H // 2, W // 2) and H % 2 == 0 and W % 2 == 0
    assert coarse.dtype == torch.float16 and coarse.is_contiguous(memory_format=torch.channels_last)
    out = torch.empty((B, out_channels, H, W), dtype=torch.float16, device=x.device, memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().s2a_conv1x1_add_up2_f16(_lib.ptr(x), _lib.ptr(packed_weight), _lib.ptr(bias), _lib.ptr(coarse),
                                                      _lib.ptr(out), B, C, H, W, out_channels, _lib.stream_ptr(x.device)))
    return out


class PackedWeightCache:
    """inference-time cache of the packed forms of ONE weight / bias pair: the fragment-order filter (conv_pack_weight),
    the Winograd-transformed filter (conv_wino_pack_weight), the padded f16 bias, or any other packed form through
    lookup().

    Invariant: a key may contain data_ptr() only of a tensor whose storage the cache itself keeps alive, and a cache
    entry is keyed on the *parameter* it derives from, never on an intermediate.  Every entry therefore holds the keyed
    tensor itself plus a detach() alias of it, and hits only for that very tensor object at its recorded version and
    address: the allocator cannot hand the address to other data while the entry lives, and a second tensor object at
    the same address (a fresh temporary, a replaced parameter) misses.  The one intermediate that is handed in,
    ORConv2d's ARF expansion, is itself an entry of ORConv2d.rotate_arf keyed on the 5-D parameter, with or without
    train().

    What a key follows: no_grad in-place ops, optimizer steps, load_state_dict, nn.init.*, `mod.weight = Parameter(..)`,
    `p.data = new`, .float() / .half() / .to().  What NO key can follow: in-place writes through `.data`
    (`p.data.copy_()`, `p.data.normal_()`, `p.data.fill_()`) - they neither bump the version counter nor move the
    storage.  After such a write call drop_weight_caches(module)."""

    def __init__(self):
        self.slots = {}

    def clear(self):
        self.slots = {}

    def lookup(self, slot, t, extra, make, *args):
        """the entry of `slot` if it was made from this very tensor in its current state, else make(*args) -> stored.
        An entry is (tensor, version, address, extra, value, detach() alias): the alias keeps the storage alive, so that
        the same object at the same address and version is the same memory, dtype and device included."""
        e = self.slots.get(slot)
        if e is not None and e[0] is t and e[1] == t._version and e[2] == t.data_ptr() and e[3] == extra:
            return e[4]
        e = (t, t._version, t.data_ptr(), extra, make(*args), t.detach())
        self.slots[slot] = e
        return e[4]

    def get_wino(self, w):
        """the Winograd-transformed filter (conv_wino_pack_weight) of a [O,C,3,3] weight"""
        return self.lookup("wino", w, None, conv_wino_pack_weight, w)

    def get(self, w):
        return self.lookup("direct", w, None, conv_pack_weight, w)

    def get_fp8(self, w, in_scale):
        """(e4m3 fragment-order filter, scale f32[O] = in_scale * s_w) of a [O,C,3,3] weight; the input scale is part of the
        key, so a re-calibration makes a new entry"""
        return self.lookup("fp8", w, float(in_scale), conv_pack_weight_fp8, w, float(in_scale))

    def get_bias_f32(self, b):
        return self.lookup("bias_f32", b, None, lambda t: t.detach().float().contiguous(), b)

    def get_bias(self, b, width):
        """f16 bias zero-padded to the physical channel count"""
        if b is None:
            return None
        return self.lookup("bias", b, width, _pad_bias_f16, b, width)


def _pad_bias_f16(b, width):
    v = b.detach().to(torch.float16)
    if v.numel() < width:
        v = torch.cat([v, v.new_zeros(width - v.numel())])
    return v.contiguous()


def drop_weight_caches(module):
    """forget every packed / expanded weight cached in the module tree (FusedConv2d and ORConv2d packed filters and
    biases, ORConv2d's ARF expansion, AlignConv's stage-major filter, the fused stem's filter and bias); the next
    no-grad forward packs again from the current parameters.  Needed after in-place writes through `.data`
    (`p.data.copy_()`, `p.data.normal_()`, ...), which no cache key can see; every other update route is followed
    without it.  A HIP graph captured before this call replays the dropped buffers: capture it again."""
    for m in module.modules():
        for name in ("_packed", "_stem_cache"):
            c = m.__dict__.get(name)
            if isinstance(c, PackedWeightCache):
                c.clear()
            elif c is not None:
                m.__dict__[name] = None
        if m.__dict__.get("_arf_cache") is not None:
            m._arf_cache = None
    return module


def train_shape_problem(ksize, stride, padding, dilation, groups, C, O, B, H, W):
    """why the dense training kernels cannot run this C -> O convolution on a [B, C, H, W] input, or None.  Plain values, and the
    ONE statement of these limits in Python: the conjunction of what the forward, the input gradient and the weight gradient
    of either stride and the pack accept (tests/test_train_limits_cpu.py holds it against the library's own queries)."""
    k, st, pd = tuple(ksize), tuple(stride), tuple(padding)
    if not (((k == (3, 3) and pd == (1, 1)) or (k == (1, 1) and pd == (0, 0))) and st in ((1, 1), (2, 2)) and
            tuple(dilation) == (1, 1) and groups == 1):
        return "not 3x3 / pad 1 or 1x1 / pad 0 at stride 1 or 2, dilation 1, groups 1"
    if C % 64 != 0 or O % 64 != 0 or (st == (2, 2) and k == (3, 3) and O % 128 != 0):
        return "channel counts are no multiples of 64 (out_channels of 128 for 3x3 at stride 2)"
    Ho, Wo = (H - 1) // st[0] + 1, (W - 1) // st[1] + 1
    ok = (min(B, C, O, H, W) > 0 and H < 32000 and W < 32000 and B < (1 << 31) and C < (1 << 24) and O < (1 << 24) and
          B * H * W * C * 2 < (1 << 31) and B * Ho * Wo * O * 2 < (1 << 31) and O * C * k[0] * k[1] * 4 < (1 << 31))
    return None if ok else "empty, a map side of 32000 or more, or input, output or filter of 2^31 bytes or more"


def train_tensors_problem(x, weight, bias, c_in, residual=None, c_out=None, stride=(1, 1)):
    """what train_shape_problem cannot say, or None: x f16 channels-last 4-D, non-empty, on the GPU, c_in wide (x = None: an
    activation the route itself produces, which is all that); weight f16 or f32 on the GPU, bias of its dtype or None; a
    residual of the output's shape ([B, c_out, Ho, Wo] at `stride`), dtype and layout"""
    CL = torch.channels_last
    if x is not None and not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 4 and x.numel() > 0 and
                              x.is_contiguous(memory_format=CL) and x.shape[1] == c_in):
        return "x is not a non-empty f16 channels-last 4-D tensor of the layer's width on the GPU"
    if weight.dtype not in (torch.float16, torch.float32) or not weight.is_cuda or (bias is not None and bias.dtype != weight.dtype):
        return "the weight is not f16 or f32 on the GPU, or the bias has another dtype"
    if residual is not None and not (
            residual.is_cuda and residual.dtype == torch.float16 and residual.is_contiguous(memory_format=CL) and
            tuple(residual.shape) == (x.shape[0], c_out, (x.shape[2] - 1) // stride[0] + 1, (x.shape[3] - 1) // stride[1] + 1)):
        return "the residual has not the output's shape, dtype and layout"
    return None


def _train_problem(x, weight, bias, stride, padding, dilation, groups, residual=None, widths=None):
    """the two checks on an [O,C,k,k] filter; widths: the (C, O) the kernels would see when not the filter's own (train_pad_widths)"""
    O, C = weight.shape[:2]
    return (train_tensors_problem(x, weight, bias, C, residual, O, tuple(stride)) or
            train_shape_problem(weight.shape[2:], stride, padding, dilation, groups, *(widths or (C, O)), x.shape[0], *x.shape[2:]))


def _train_conv_problem(x, conv, residual=None, widths=None):
    return _train_problem(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups, residual, widths)


def train_conv_ok(x, conv, residual=None):
    """limits of the own training route (FusedConvFunction), and nothing but limits: stride 1, what train_tensors_problem asks
    of x, the parameters and the residual, and what train_shape_problem asks of the geometry, the widths and the sizes.  The
    speed heuristics of own_conv_ok play no part: a layer on this route is bit-reproducible whatever its size."""
    return tuple(conv.stride) == (1, 1) and _train_conv_problem(x, conv, residual) is None


def train_filter_ok(x, weight, bias, stride, padding, dilation, groups):
    """train_conv_ok for a bare [O,C,k,k] filter (ORConv2d's expansion, which is no module's parameter)"""
    return weight.dim() == 4 and tuple(stride) == (1, 1) and _train_problem(x, weight, bias, stride, padding, dilation, groups) is None


def train_conv_strided_ok(x, conv, residual=None):
    """limits of the own training route of the stride-2 layers (FusedConvS2Function), and nothing but limits: stride (2, 2) and
    the two checks of train_conv_ok, in which a 3x3 then needs O % 128 == 0 (the forward kernel's limit) and the residual has
    the OUTPUT's shape.  No speed heuristic plays a part, as in train_conv_ok."""
    return tuple(conv.stride) == (2, 2) and _train_conv_problem(x, conv, residual) is None


def train_pad_widths(x, conv):
    """deterministic mode only: (C', O') when the layer fails train_conv_ok for its width alone and passes at the zero-padded
    width -- fewer than 64 filters (the 5- and 15-map prediction convs: O' = 64) over C % 64 == 0 or C == 32 inputs, or 32
    inputs (odm_cls_ls[0] behind the orientation pooling: C' = 64) under O % 64 == 0 filters; None otherwise"""
    C, O = conv.in_channels, conv.out_channels
    Cp, Op = (64 if C == 32 else C), (64 if 0 < O < 64 else O)
    ok = (Cp, Op) != (C, O) and tuple(conv.stride) == (1, 1) and _train_conv_problem(x, conv, None, (Cp, Op)) is None
    return (Cp, Op) if ok else None


def padded_train_conv(x, weight, bias, relu, Cp, Op):
    """FusedConvFunction at the padded width: filter rows and bias (O -> O') and filter columns and input (C -> C') are
    zero-padded with stock differentiable ops, the result is the [:, :O] view -- autograd slices the gradients back.  The
    padded products are exact zeros, so every real entry is the sum the kernel forms at the layer's own width."""
    O, C = weight.shape[:2]
    if Cp != C:
        x = F.pad(x, (0, 0, 0, 0, 0, Cp - C)).contiguous(memory_format=torch.channels_last)
    if (Cp, Op) != (C, O):
        weight = F.pad(weight, (0, 0, 0, 0, 0, Cp - C, 0, Op - O))
    if bias is not None and Op != O:
        bias = F.pad(bias, (0, Op - O))
    out = FusedConvFunction.apply(x, weight, bias, None, relu)
    return out if Op == O else out[:, :O]


def train_kernels(module, enabled=True, strided=False, entry=False):
    """own_grad = enabled on every FusedConv2d of the tree -> how many were set.  With own_grad a grad-enabled forward of
    an eligible layer (train_conv_ok) runs FusedConvFunction: forward, input gradient, weight gradient, bias gradient and
    ReLU mask on the project's kernels.  Every other layer and every other call keeps its route.
    strided=True: a second opt-in, own_grad_strided = enabled on the same modules (not set or cleared otherwise) -- the
    stride-2 layers (train_conv_strided_ok: the 3x3 / s2 conv2 and the 1x1 / s2 downsample of a stage's first bottleneck,
    FPN's two extra levels) run FusedConvS2Function under grad.  The return value is the same count.
    entry=True: the third opt-in, own_grad_entry = enabled on the same modules (not set or cleared otherwise) -- the stem
    trains from the uint8 batch (DetectorBackbone.forward: StemU8Function, the 7x7 convolution, its ReLU and the max-pool
    in one launch each way) and FPN's top-down steps run FusedConvUp2Function (FPN.forward).  The same count again.
    In deterministic mode (s2anet_amd.deterministic) own_grad also takes the layers that fail train_conv_ok for their width
    alone (train_pad_widths) and, set here as well but not counted, the ORConv2d modules of the tree."""
    from .orn import ORConv2d
    n = 0
    for m in module.modules():
        if isinstance(m, FusedConv2d):
            m.own_grad = bool(enabled)
            if strided:
                m.own_grad_strided = bool(enabled)
            if entry:
                m.own_grad_entry = bool(enabled)
            n += 1
        elif isinstance(m, ORConv2d):
            m.own_grad = bool(enabled)
    return n


def _train_pack(weight, need_x, device):
    """s2a_conv_pack_weight_train -> (the filter in forward order, in input-gradient order when x wants a gradient, else None)"""
    O, C, k, _ = weight.shape
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()            # (a channels-last 3x3 filter: one stock copy)
    fwd = torch.empty((w.numel(),), dtype=torch.float16, device=device)
    dgrad = torch.empty_like(fwd) if need_x else None
    with torch.cuda.device(device):
        _lib.check(_lib.lib().s2a_conv_pack_weight_train(_lib.ptr(w), _lib.dtype_code(w), O, C, k, _lib.ptr(fwd), _lib.ptr(dgrad),
                                                         _lib.stream_ptr(device)))
    return fwd, dgrad


def _train_forward(ctx, x, weight, bias, residual, relu, stride):
    """the forward both training Functions share: pack (forward order and, when x wants a gradient, input-gradient order),
    s2a_conv_nhwc_f16 at `stride` with bias and residual fused, the stock in-place ReLU; saves what the backward needs"""
    O, C, k, _ = weight.shape
    need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    fwd, dgrad = _train_pack(weight, need_x, x.device)
    # the launch's fused ReLU is inference's (NaN -> 0, include/s2anet_hip.h): training runs it with relu = 0 and
    # applies the stock in-place ReLU, which keeps a NaN; the finite entries get the same bits either way
    out = conv_f16(x, fwd, None if bias is None else bias.detach(), O, k, stride, False, residual)
    if relu:
        out.relu_()
    ctx.save_for_backward(x if need_w else None, out if relu else None, dgrad)
    ctx.geom = (tuple(x.shape), O, k, weight.dtype, None if bias is None else bias.dtype)
    return out


def _train_prep(ctx, grad_out, out, positions):
    """the backward's first pass (s2a_conv_backward_prep_f16 on [positions, O]) -> (g, grad_bias): g = grad_out behind the ReLU
    mask as dense f16 channels-last (grad_out itself without a ReLU, or when nothing needs it), the bias gradient or None"""
    O, bdtype = ctx.geom[1], ctx.geom[4]
    need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
    L, dev = _lib.lib(), grad_out.device
    go = grad_out if grad_out.dtype == torch.float16 else grad_out.to(torch.float16)
    go = go.contiguous(memory_format=torch.channels_last)
    g, gb = go, None
    need_g = need_x or need_w or need_r
    if (out is not None and need_g) or need_b:
        if out is not None and need_g:
            g = torch.empty_like(go)
        ws = None
        if need_b:
            gb = torch.empty((O,), dtype=bdtype, device=dev)
            ws = torch.empty((L.s2a_conv_backward_prep_f16_workspace_bytes(positions, O),), dtype=torch.uint8, device=dev)
        _lib.check(L.s2a_conv_backward_prep_f16(_lib.ptr(go), _lib.ptr(out), _lib.ptr(g if g is not go else None),
                                                _lib.ptr(gb), 0 if gb is None else _lib.dtype_code(gb), positions, O,
                                                _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr(dev)))
    return g, gb


def _train_wgrad(x, g, geom):
    """the stride-1 weight gradient (s2a_conv_backward_weight_f16) of ctx.geom, in the weight's dtype; under g's device"""
    (B, C, H, W), O, k, wdtype, _ = geom
    L, dev = _lib.lib(), g.device
    gw = torch.empty((O, C, k, k), dtype=wdtype, device=dev)
    ws = torch.empty((L.s2a_conv_backward_weight_f16_workspace_bytes(B, C, H, W, O, k),), dtype=torch.uint8, device=dev)
    _lib.check(L.s2a_conv_backward_weight_f16(_lib.ptr(x), _lib.ptr(g), _lib.ptr(gw), _lib.dtype_code(gw), B, C, H, W, O, k,
                                              _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return gw


class FusedConvFunction(torch.autograd.Function):
    """relu?(conv(x) + bias (+ residual)) with its backward on the own kernels.  x f16 channels-last; weight / bias f16
    or f32 (masters: rounded to f16 by the pack, gradients straight from the f32 sums); stride 1, 3x3 / pad 1 or 1x1.
    Non-finite values follow torch: a NaN pre-activation stays NaN behind the ReLU, and the backward passes the gradient
    unless out <= 0, so an overflow reaches the gradients and TrainUpdate's found_inf.
    The filter is packed on EVERY call (s2a_conv_pack_weight_train: forward order and input-gradient order in one
    launch), never cached: weights change every step, and a graph replay moves no version counter.  No host read,
    launch geometry from shapes only, workspaces from the torch allocator: forward + backward can be captured."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, relu):
        return _train_forward(ctx, x, weight, bias, residual, relu, 1)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, out, dgrad = ctx.saved_tensors
        (B, C, H, W), _, k = ctx.geom[:3]
        need_x, need_w, _, need_r = ctx.needs_input_grad[:4]
        with torch.cuda.device(grad_out.device):
            g, gb = _train_prep(ctx, grad_out, out, B * H * W)
            gx = conv_f16(g, dgrad, None, C, k, 1, False) if need_x else None
            gw = _train_wgrad(x, g, ctx.geom) if need_w else None
        return gx, gw, gb, (g if need_r else None), None


class FusedConvS2Function(torch.autograd.Function):
    """FusedConvFunction for the stride-2 layers (train_conv_strided_ok): 3x3 / pad 1 or 1x1, stride 2.  Pack, forward (at
    stride 2) and prep (on [B Ho Wo, O]) are shared with it; the backward then runs s2a_conv_backward_input_s2_f16 (a
    stride-2 convolution's input gradient is no convolution of g: four parity classes of the input pixel, nine tap products
    per 2 x 2 pixels) and s2a_conv_backward_weight_s2_f16 + _reduce (per-slice f32 sums in the gradient's layout, summed in
    slice order).  Only what needs_input_grad asks for is computed.  No host read, no float atomic, no memset node, geometry
    from shapes only, buffers from the torch allocator: capturable, and bit-equal from run to run."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, relu):
        return _train_forward(ctx, x, weight, bias, residual, relu, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, out, dgrad = ctx.saved_tensors
        (B, C, H, W), O, k, wdtype, _ = ctx.geom
        need_x, need_w, _, need_r = ctx.needs_input_grad[:4]
        L, dev = _lib.lib(), grad_out.device
        st = _lib.stream_ptr(dev)
        gx = gw = None
        with torch.cuda.device(dev):
            g, gb = _train_prep(ctx, grad_out, out, B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1))
            if need_x:
                gx = torch.empty((B, C, H, W), dtype=torch.float16, device=dev, memory_format=torch.channels_last)
                _lib.check(L.s2a_conv_backward_input_s2_f16(_lib.ptr(g), _lib.ptr(dgrad), _lib.ptr(gx), B, C, H, W, O, k, st))
            if need_w:
                slices = L.s2a_conv_backward_weight_s2_slices(B, C, H, W, O, k)
                partial = torch.empty((slices, O, C * k * k), dtype=torch.float32, device=dev)
                gw = torch.empty((O, C, k, k), dtype=wdtype, device=dev)
                _lib.check(L.s2a_conv_backward_weight_s2_f16(_lib.ptr(x), _lib.ptr(g), _lib.ptr(partial), slices, B, C, H, W, O,
                                                             k, st))
                _lib.check(L.s2a_conv_backward_weight_s2_reduce(_lib.ptr(partial), slices, gw.numel(), _lib.ptr(gw),
                                                                _lib.dtype_code(gw), st))
        return gx, gw, gb, (g if need_r else None), None


def train_up2_ok(x, conv, coarse):
    """limits of FusedConvUp2Function, and nothing but limits: a 1x1 lateral inside train_conv_ok, a coarser level of
    exactly half the size in f16 channels-last with the lateral's output width, and something that requires grad"""
    # (s2a_conv1x1_add_up2_f16 has no pointer-free query to hold its own limits against: what stands here beyond train_conv_ok
    # is read off its entry point, not pinned by tests/test_train_limits_cpu.py)
    return (train_conv_ok(x, conv) and tuple(conv.kernel_size) == (1, 1) and coarse.is_cuda and coarse.dtype == torch.float16 and
            coarse.dim() == 4 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and
            tuple(coarse.shape) == (x.shape[0], conv.out_channels, x.shape[2] // 2, x.shape[3] // 2) and
            coarse.is_contiguous(memory_format=torch.channels_last) and _needs_grad(x, conv.weight, conv.bias, coarse))


class FusedConvUp2Function(torch.autograd.Function):
    """FPN's top-down step conv1x1(x) + bias + nearest-2x-upsample(coarse) with its backward on the own kernels: the forward
    is s2a_conv1x1_add_up2_f16 on the forward filter of s2a_conv_pack_weight_train (packed on every call, as in
    FusedConvFunction); backward: grad_x by s2a_conv_nhwc_f16 on the input-gradient filter, grad_weight by
    s2a_conv_backward_weight_f16, grad_bias by the prep pass, grad_coarse by s2a_sum_pool2x2_f16 (the four fine gradients of a
    coarse pixel summed over f32 in a fixed order, one rounding).  Only what needs_input_grad asks for is computed.  No host
    read, no float atomic, no memset node: capturable, and bit-equal from run to run."""

    @staticmethod
    def forward(ctx, x, weight, bias, coarse):
        O = weight.shape[0]
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        fwd, dgrad = _train_pack(weight, need_x, x.device)          # (a 1x1 filter: train_up2_ok)
        b = None if bias is None else bias.detach().to(torch.float16).contiguous()
        out = conv1x1_add_up2(x, fwd, b, coarse.detach(), O)
        ctx.save_for_backward(x if need_w else None, dgrad)
        ctx.geom = (tuple(x.shape), O, 1, weight.dtype, None if bias is None else bias.dtype)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, dgrad = ctx.saved_tensors
        (B, C, H, W), O = ctx.geom[:2]
        need_x, need_w, _, need_c = ctx.needs_input_grad[:4]
        L, dev = _lib.lib(), grad_out.device
        gx = gw = gc = None
        with torch.cuda.device(dev):
            g, gb = _train_prep(ctx, grad_out, None, B * H * W)          # (no ReLU: g is grad_out, dense f16 channels-last)
            if need_x:
                gx = conv_f16(g, dgrad, None, C, 1, 1, False)
            if need_w:
                gw = _train_wgrad(x, g, ctx.geom)
            if need_c:
                gc = torch.empty((B, O, H // 2, W // 2), dtype=torch.float16, device=dev, memory_format=torch.channels_last)
                _lib.check(L.s2a_sum_pool2x2_f16(_lib.ptr(g), _lib.ptr(gc), B, H, W, O, _lib.stream_ptr(dev)))
        return gx, gw, gb, gc


class FusedConv2d(nn.Conv2d):
    """nn.Conv2d + (bias, optional residual, optional ReLU) epilogue in one pass"""
    own_grad_entry = False      # train_kernels(entry=True): the stem conv trains from the uint8 batch (StemU8Function), FPN's
    #                             laterals run their top-down step as FusedConvUp2Function
    own_grad = False        # train_kernels(): grad-enabled forwards of eligible layers (train_conv_ok) run FusedConvFunction
    own_grad_strided = False    # train_kernels(strided=True): those of the stride-2 layers (train_conv_strided_ok) run
    #                             FusedConvS2Function

    def __init__(self, *args, relu=False, **kw):
        super().__init__(*args, **kw)
        self.fuse_relu = relu

    @classmethod
    def from_conv(cls, conv, relu=False):
        m = cls(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding,
                conv.dilation, conv.groups, bias=conv.bias is not None, relu=relu)
        m = m.to(conv.weight.device, conv.weight.dtype)
        m.weight = conv.weight
        m.bias = conv.bias
        return m

    def packed_args(self):
        """(fragment-order filter, f16 bias, physical out channels) for the pyramid-packed launches"""
        if not hasattr(self, "_packed"):
            self._packed = PackedWeightCache()
        width = max(64, self.out_channels)
        return self._packed.get(self.weight), self._packed.get_bias(self.bias, width), width

    def fp8_ok(self):
        """a layer the e4m3 kernel serves: 3x3 / stride 1 / pad 1 with bias, O a multiple of 64, C a multiple of 128"""
        return (tuple(self.kernel_size) == (3, 3) and tuple(self.stride) == (1, 1) and tuple(self.padding) == (1, 1) and
                tuple(self.dilation) == (1, 1) and self.groups == 1 and self.bias is not None and
                self.out_channels % 64 == 0 and self.in_channels % 128 == 0)

    def packed_args_fp8(self, in_scale):
        """(e4m3 filter, scale f32[O], bias f32[O], out channels) for s2a_conv3x3_pyramid_fp8 on an input quantised with
        in_scale (x = in_scale * x_q)"""
        if not hasattr(self, "_packed"):
            self._packed = PackedWeightCache()
        w, sc = self._packed.get_fp8(self.weight, in_scale)
        return w, sc, self._packed.get_bias_f32(self.bias), self.out_channels

    def wino_ok(self):
        """a layer the Winograd kernel serves: 3x3 / stride 1 / pad 1, O a multiple of 64, C a multiple of 32"""
        return (tuple(self.kernel_size) == (3, 3) and tuple(self.stride) == (1, 1) and tuple(self.padding) == (1, 1) and
                tuple(self.dilation) == (1, 1) and self.groups == 1 and self.out_channels % 64 == 0 and
                self.in_channels % 32 == 0)

    def packed_args_wino(self):
        """(transformed filter, f16 bias, out channels) for s2a_conv3x3_wino_pyramid_f16"""
        if not hasattr(self, "_packed"):
            self._packed = PackedWeightCache()
        return self._packed.get_wino(self.weight), self._packed.get_bias(self.bias, self.out_channels), self.out_channels

    def forward(self, x, residual=None, out=None, chain=None):
        """out: dense NHWC buffer for the result (library path only; the own kernel is called with out= directly);
        chain: a Conv3Chain, honoured on the own-kernel path only (conv_f16)"""
        if out is None and self.own_grad and _needs_grad(x, self.weight, self.bias, residual) and \
                train_conv_ok(x, self, residual):
            return FusedConvFunction.apply(x, self.weight, self.bias, residual, self.fuse_relu)   # (chain= is ignored, as under grad)
        if out is None and self.own_grad_strided and _needs_grad(x, self.weight, self.bias, residual) and \
                train_conv_strided_ok(x, self, residual):
            return FusedConvS2Function.apply(x, self.weight, self.bias, residual, self.fuse_relu)
        if out is None and residual is None and self.own_grad and _lib.deterministic() and _needs_grad(x, self.weight, self.bias):
            pad = train_pad_widths(x, self)
            if pad is not None:     # deterministic mode: the library's weight gradient is not reproducible, the padded own route is
                return padded_train_conv(x, self.weight, self.bias, self.fuse_relu, *pad)
        if out is not None:
            assert x.is_cuda and self.bias is not None and not torch.is_grad_enabled() and not own_conv_ok(
                x, self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation, self.groups)
            y = F.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation, self.groups)
            return bias_act_(y, self.bias, residual, self.fuse_relu, out=out)
        if not torch.is_grad_enabled() and own_conv_ok(
                x, self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding,
                self.dilation, self.groups) and (residual is None or (
                    residual.dtype == torch.float16 and residual.is_contiguous(memory_format=torch.channels_last))):
            if not hasattr(self, "_packed"):
                self._packed = PackedWeightCache()
            kw = {} if chain is None else {"chain": chain}
            return conv_f16(x, self._packed.get(self.weight), self._packed.get_bias(self.bias, max(64, self.out_channels)),
                            self.out_channels, self.kernel_size[0], self.stride[0], self.fuse_relu, residual, **kw)
        if (not x.is_cuda) or self.bias is None:
            y = super().forward(x)
            if residual is not None:
                y = y + residual
            return F.relu(y) if self.fuse_relu else y
        # library convolution + epilogue: the raw one-pass epilogue when no gradient is wanted, stock (differentiable) ops
        # when grad is enabled and x, the filter, the bias or the residual requires grad (bias_act_ decides)
        y = F.conv2d(x, self.weight, None, self.stride, self.padding, self.dilation, self.groups)
        return bias_act_(y, self.bias, residual, self.fuse_relu)


def stem_pack_weight(weight):
    """[64,3,7,7] -> the fragment order of the fused stem kernel (s2a_stem_pack_weight_f16)"""
    w = weight.detach().to(torch.float16).contiguous()
    assert tuple(w.shape) == (64, 3, 7, 7)
    L = _lib.lib()
    out = torch.empty((L.s2a_stem_packed_elems(),), dtype=torch.float16, device=w.device)
    with torch.cuda.device(w.device):
        _lib.check(L.s2a_stem_pack_weight_f16(_lib.ptr(w), _lib.ptr(out), _lib.stream_ptr(w.device)))
    return out


def stem_u8(imgs_u8, packed_weight, bias, divisor=255.0):
    """uint8 image [B,3,H,W] (channels-last storage) -> relu(conv7x7/2(img / divisor) + bias) -> maxpool 3x3/2:
    [B,64,H/4,W/4] f16 channels-last, one kernel (s2a_stem_u8_f16)"""
    _lib.require_cuda(imgs_u8)
    B, C, H, W = imgs_u8.shape
    assert C == 3 and imgs_u8.dtype == torch.uint8 and imgs_u8.permute(0, 2, 3, 1).is_contiguous()
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hp, Wp = (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1
    out = torch.empty((B, 64, Hp, Wp), dtype=torch.float16, device=imgs_u8.device, memory_format=torch.channels_last)
    b = None if bias is None else bias.to(torch.float16).contiguous()
    with torch.cuda.device(imgs_u8.device):
        _lib.check(_lib.lib().s2a_stem_u8_f16(_lib.ptr(imgs_u8), _lib.ptr(packed_weight), _lib.ptr(b), _lib.ptr(out),
                                              B, H, W, float(divisor), _lib.stream_ptr(imgs_u8.device)))
    return out


STEM_GRAD_COLS = 64 * 147 + 64      # floats per slice of s2a_stem_backward_f16: the filter gradient, then the bias sums


def stem_out_hw(H, W):
    """pooled size of the stem: 7x7 / 2 / pad 3, then 3x3 / 2 / pad 1"""
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


class StemU8Function(torch.autograd.Function):
    """StemU8Function.apply(imgs_u8, weight, bias, divisor): relu(conv7x7/2(img / divisor) + bias) -> maxpool 3x3/2 from the
    uint8 batch [B,3,H,W] (channels-last storage), [B,64,H/4,W/4] f16 channels-last, with the backward on the own kernels.
    weight [64,3,7,7] / bias [64] or None: f16 parameters or f32 masters (rounded to f16 on the way in, gradients in the
    master dtype straight from the f32 sums).  The filter is packed on every call, never cached (as FusedConvFunction).
    Forward s2a_stem_u8_f16_train: the inference kernel's bits for finite parameters, torch's ReLU and pool for non-finite
    ones, plus one byte per output naming the pooled tap.  Saved: imgs_u8, out and those bytes -- no normalised image, no
    [B,64,H/2,W/2] activation, no int64 indices.  Backward s2a_stem_backward_f16 + s2a_conv_backward_weight_s2_reduce: the
    filter and bias gradient (an image gets none), per-slice f32 sums added in slice order.  No host read, no float atomic,
    no memset node, geometry from shapes only: capturable, and bit-equal from run to run."""

    @staticmethod
    def forward(ctx, imgs_u8, weight, bias, divisor):
        _lib.require_cuda(imgs_u8, weight, bias)
        B, C, H, W = imgs_u8.shape
        assert C == 3 and imgs_u8.dtype == torch.uint8 and imgs_u8.permute(0, 2, 3, 1).is_contiguous()
        assert tuple(weight.shape) == (64, 3, 7, 7) and weight.dtype in (torch.float16, torch.float32)
        assert bias is None or (bias.dtype == weight.dtype and tuple(bias.shape) == (64,))
        dev = imgs_u8.device
        Hp, Wp = stem_out_hw(H, W)
        packed = stem_pack_weight(weight)
        b = None if bias is None else bias.detach().to(torch.float16).contiguous()
        out = torch.empty((B, 64, Hp, Wp), dtype=torch.float16, device=dev, memory_format=torch.channels_last)
        sel = torch.empty((B, Hp, Wp, 64), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().s2a_stem_u8_f16_train(_lib.ptr(imgs_u8), _lib.ptr(packed), _lib.ptr(b), _lib.ptr(out), _lib.ptr(sel),
                                                        B, H, W, float(divisor), _lib.stream_ptr(dev)))
        ctx.save_for_backward(imgs_u8, out, sel)
        ctx.geom = (B, H, W, float(divisor), weight.dtype, bias is not None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        imgs_u8, out, sel = ctx.saved_tensors
        B, H, W, divisor, wdtype, has_bias = ctx.geom
        need_w, need_b = ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2]
        if not (need_w or need_b):
            return None, None, None, None
        L, dev = _lib.lib(), grad_out.device
        go = grad_out if grad_out.dtype == torch.float16 else grad_out.to(torch.float16)
        go = go.contiguous(memory_format=torch.channels_last)
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            slices = L.s2a_stem_backward_slices(B, H, W)
            partial = torch.empty((slices, STEM_GRAD_COLS), dtype=torch.float32, device=dev)
            _lib.check(L.s2a_stem_backward_f16(_lib.ptr(imgs_u8), _lib.ptr(out), _lib.ptr(sel), _lib.ptr(go), _lib.ptr(partial), slices,
                                               B, H, W, divisor, st))
            grads = torch.empty((STEM_GRAD_COLS,), dtype=wdtype, device=dev)
            _lib.check(L.s2a_conv_backward_weight_s2_reduce(_lib.ptr(partial), slices, STEM_GRAD_COLS, _lib.ptr(grads),
                                                            _lib.dtype_code(grads), st))
        gw = grads[:64 * 147].view(64, 3, 7, 7) if need_w else None
        gb = grads[64 * 147:] if need_b else None
        return None, gw, gb, None
