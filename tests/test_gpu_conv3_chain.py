"""GPU: a bottleneck's conv3 with the next block's conv1 chained into the same launch (s2a_conv1x1_chain_f16).

Per shape class (K, O, O3) the entry point is called directly on a ragged map (270 positions: a partial last tile, an
image boundary inside a tile) and on one smaller than a tile, with and without a residual:
  * `out` equals the stand-alone 1x1 launch bit for bit, `chain_out` the stand-alone conv1 launch on it;
  * a second launch into NaN-filled buffers gives the same bits (every element written, deterministically);
  * both stay within the elementwise float64 bounds of oracle/conv64.py (tau below: the formulas of
    tests/test_gpu_forward_shapes.py);
  * the stand-alone launches give these bits with S2A_CONV1_HALF forced either way.
Trunk level: DetectorBackbone on one 3 x 160 x 192 chip gives the same C3, C4, C5 with the chain on and off, the chain
removes exactly its conv1 launches, and backbone.backbone.4.1.conv1 still runs as a launch of its own."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY = 2.0 ** -25                 # half an f16 subnormal step: the absolute floor of an underflowed result

SHAPES = [(128, 512, 128), (128, 512, 256), (256, 1024, 256)]
SIZES = [(2, 9, 15), (1, 5, 7)]


def tau(kind, K):
    """elementwise bound / S (u = 2^-11, v = 2^-24, K products per output):
    conv      exact f16 products summed in f32 (K v), + bias in f32, one f16 rounding  -> u + (K + 17) v
    conv_res  rnd16(rnd16(acc + b) + r): the residual epilogue rounds twice           -> 2u + (K + 17) v"""
    return {"conv": U16 + (K + 17) * U32, "conv_res": 2 * U16 + (K + 17) * U32}[kind]


def within(got, y, S, kind, K):
    err = (got.double() - y).abs()
    return int((~(err <= tau(kind, K) * S + TINY)).sum()) == 0


def chain_launch(x, w3, b3, res, wc, bc, O, O3):
    """the entry point itself, into NaN-filled outputs -> (out, chain_out)"""
    from s2anet_amd import _lib
    B, K, H, W = x.shape
    out = torch.full((B, O, H, W), float("nan"), dtype=torch.float16, device=x.device).contiguous(memory_format=torch.channels_last)
    nxt = torch.full((B, O3, H, W), float("nan"), dtype=torch.float16, device=x.device).contiguous(memory_format=torch.channels_last)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().s2a_conv1x1_chain_f16(_lib.ptr(x), _lib.ptr(w3), _lib.ptr(b3), _lib.ptr(res), _lib.ptr(out),
                                                    _lib.ptr(wc), _lib.ptr(bc), _lib.ptr(nxt), O3, B, K, O, H, W,
                                                    _lib.stream_ptr(x.device)))
    return out, nxt


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("B,H,W", SIZES)
@pytest.mark.parametrize("K,O,O3", SHAPES)
def test_chained_launch_equals_the_two_launches(K, O, O3, B, H, W, with_res, monkeypatch):
    from oracle.conv64 import conv64
    from s2anet_amd.fused import conv_f16, conv_pack_weight
    g = torch.Generator().manual_seed(1000 * K + O3 + 7 * H + int(with_res))
    cl = dict(memory_format=torch.channels_last)
    x = torch.randn(B, K, H, W, generator=g).to(DEV).half().contiguous(**cl)
    w3 = (torch.randn(O, K, 1, 1, generator=g) * 0.1).to(DEV).half()
    b3 = (torch.randn(O, generator=g) * 0.1).to(DEV).half()
    wc = (torch.randn(O3, O, 1, 1, generator=g) * 0.05).to(DEV).half()
    bc = (torch.randn(O3, generator=g) * 0.1).to(DEV).half()
    res = torch.randn(B, O, H, W, generator=g).to(DEV).half().contiguous(**cl) if with_res else None
    p3, pc = conv_pack_weight(w3), conv_pack_weight(wc)

    out, nxt = chain_launch(x, p3, b3, res, pc, bc, O, O3)
    out0 = conv_f16(x, p3, b3, O, 1, 1, True, res)
    nxt0 = conv_f16(out0, pc, bc, O3, 1, 1, True)
    assert torch.equal(out, out0), (out.float() - out0.float()).abs().max().item()
    assert torch.equal(nxt, nxt0), (nxt.float() - nxt0.float()).abs().max().item()
    # (torch.equal on NaN is False: every element was written)
    out2, nxt2 = chain_launch(x, p3, b3, res, pc, bc, O, O3)
    assert torch.equal(out2, out) and torch.equal(nxt2, nxt)
    y, S = conv64(x, w3, b3, 1, 1, residual=res, relu=True)
    assert within(out, y, S, "conv_res" if with_res else "conv", K)
    y, S = conv64(out, wc, bc, 1, 1, relu=True)
    assert within(nxt, y, S, "conv", O)
    assert (out != 0).float().mean().item() > 0.2 and (nxt != 0).float().mean().item() > 0.2
    for half in ("0", "1"):
        monkeypatch.setenv("S2A_CONV1_HALF", half)
        o = conv_f16(x, p3, b3, O, 1, 1, True, res)
        assert torch.equal(o, out), half
        assert torch.equal(conv_f16(o, pc, bc, O3, 1, 1, True), nxt), half


class _CountingLib:
    def __init__(self, real):
        self._real, self.counts = real, {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("s2a_"):
            return fn

        def call(*a):
            self.counts[name] = self.counts.get(name, 0) + 1
            return fn(*a)
        return call


def test_trunk_same_bits_fewer_launches(monkeypatch):
    from s2anet_amd import _lib
    from s2anet_amd.detector import BottleNeck, build_synthetic_detector
    from s2anet_amd.fused import conv3_chain_ok
    monkeypatch.setenv("S2A_OWN_CONV_ALWAYS", "1")
    monkeypatch.delenv("S2A_NO_CONV3_CHAIN", raising=False)
    bb = build_synthetic_detector(device=DEV).backbone
    imgs = torch.randint(0, 256, (1, 3, 160, 192), dtype=torch.uint8, device=DEV,
                         generator=torch.Generator(DEV).manual_seed(5)).contiguous(memory_format=torch.channels_last)
    l4c1 = bb.backbone[4][1].conv1
    # the conv1 layers the chain takes over: every block that follows a chainable conv3
    blocks = [b for i in range(2, 5) for b in bb.backbone[i]]
    with torch.no_grad():
        chained = sum(1 for a, b in zip(blocks, blocks[1:]) if isinstance(b, BottleNeck) and conv3_chain_ok(a.conv3, b.conv1))
    assert chained == 9, chained          # 3 in layer2, layer2 -> layer3.0, 5 in layer3 (layer3 -> layer4.0 is not built)
    assert not conv3_chain_ok(bb.backbone[4][0].conv3, l4c1)

    def run():
        real = _lib.lib()
        proxy = _CountingLib(real)
        own = []
        h0 = l4c1.register_forward_pre_hook(lambda m, a: own.append(-proxy.counts.get("s2a_conv_nhwc_f16", 0)))
        h1 = l4c1.register_forward_hook(lambda m, a, r: own.append(proxy.counts.get("s2a_conv_nhwc_f16", 0)))
        _lib._lib = proxy
        try:
            with torch.no_grad():
                C = bb.forward_u8(imgs, 255.0)
            torch.cuda.synchronize()
        finally:
            _lib._lib = real
            h0.remove()
            h1.remove()
        return C, proxy.counts, own

    C_on, n_on, own_on = run()
    monkeypatch.setenv("S2A_NO_CONV3_CHAIN", "1")
    C_off, n_off, own_off = run()
    assert len(C_on) == 3 and all(torch.equal(a, b) for a, b in zip(C_on, C_off))
    assert all(bool((c != 0).any()) for c in C_on)
    assert n_off.get("s2a_conv1x1_chain_f16", 0) == 0 and n_on.get("s2a_conv1x1_chain_f16", 0) == chained
    # a chained launch stands for two s2a_conv_nhwc_f16 calls (the conv3 and the next conv1): the trunk's convolution
    # launches drop by exactly the number of chained conv1 layers
    assert n_off["s2a_conv_nhwc_f16"] - n_on["s2a_conv_nhwc_f16"] == 2 * chained
    assert n_off["s2a_conv_nhwc_f16"] - (n_on["s2a_conv_nhwc_f16"] + n_on["s2a_conv1x1_chain_f16"]) == chained
    # backbone.backbone.4.1.conv1: one call, one launch of its own, either way
    assert len(own_on) == 2 and sum(own_on) == 1, own_on
    assert len(own_off) == 2 and sum(own_off) == 1, own_off
