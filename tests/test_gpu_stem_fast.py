"""GPU: the fused stem kernel (s2a_stem_u8_f16) after its issue-rate rebuild gives the bits it gave before.

The rebuild changes how k_stem issues its work (fragments fetched one step ahead, scalar tile skip, packed max in the
pooling, packed convert / ReLU in the epilogue, hoisted index arithmetic, wider LDS stores of the converted patch); the
MFMA instruction, the K layout and step order, the table value f16(u8 / divisor) and the f32 sum + f16 bias -> ReLU ->
3x3/2 max are what decide the output bits and stay.  So every output must hash to what the kernel of the parent commit
produced.  HASHES below were recorded from a build of PARENT on an MI355X, before the kernel was touched, with
`record()` of this file; they are never taken from the kernel under test.

Shapes: (1,3,8,8) one partial tile; (2,3,72,100) ragged in both directions (pooled 18 x 25: partial tiles on both
edges, two images); (1,3,800,800) 625 tiles on the 512 persistent workgroups, so the next-tile prefetch and the
second trip of the tile loop run.  Each with bias None / random and divisor 255 / 1.
Per case: the hash, equal bits from a second call into a NaN-filled buffer (every element written, deterministically),
and the elementwise float64 bound of tests/test_gpu_forward_shapes.py (Meter("stem", 147)) against oracle.conv64.stem64."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY = 2.0 ** -25                 # half an f16 subnormal step: the absolute floor of an underflowed result
TAU_STEM = U16 + (147 + 17) * U32  # tests/test_gpu_forward_shapes.py tau("stem", 147)
L2_CONV = 2 * U16                  # tests/test_gpu_forward_shapes.py L2_CONV, the Meter's relative-L2 bound

PARENT = "7fae941"                 # the commit whose k_stem produced HASHES
SHAPES = [(1, 3, 8, 8), (2, 3, 72, 100), (1, 3, 800, 800)]
CASES = [(s, wb, d) for s in SHAPES for wb in (False, True) for d in (255.0, 1.0)]
HASHES = {
    "1x3x8x8|bias=0|div=255": "e4f119a7ced0ac9bd979c6a3c1ab39cc8f939e4e9f9b66b466d34b7cbc8ca23c",
    "1x3x8x8|bias=0|div=1": "c9acaf2d76c50ba957f92c396c30ea7e15af9aaaeec413d1f67db0dc66d582e0",
    "1x3x8x8|bias=1|div=255": "7b961a4ae7bcf159450aebfc56f37e1a8cab1caebf27b40191aec39321f3fa34",
    "1x3x8x8|bias=1|div=1": "7a71ff38f88662c4ef65c643cd2d7f5062e2cef47cc1ed85072b3de9cdbb2312",
    "2x3x72x100|bias=0|div=255": "ed8f990b1ce2f12dd73d1e9276061ae3fe1353b7ae8e9c44289fb4323a94b602",
    "2x3x72x100|bias=0|div=1": "bc14264566399c50be994317d8e28e2bbaf04d9f29f61cbfc0aa9f492e1b202f",
    "2x3x72x100|bias=1|div=255": "32ada40c103bb5cbdd259d9dd72c3e7b70f8004dba23656e34ec10f974247ae4",
    "2x3x72x100|bias=1|div=1": "6a8c2e894e9b5c584b8b95bb762fba149254f67d060c7f188160197341dc5902",
    "1x3x800x800|bias=0|div=255": "c9c2913faea611abfe810f130a083e2084595cfe895b0b38085a8fa54207d42d",
    "1x3x800x800|bias=0|div=1": "503528ba5aefe817923f686a45d7f76b73357c298670513b73865c0276cea1e8",
    "1x3x800x800|bias=1|div=255": "d5fa9adc2c6de97e11c4b39a242be1d5e58d2f5c8a67979d2152edae569b2e14",
    "1x3x800x800|bias=1|div=1": "d5580227f3e585b2b8c21b080f3f161d39c150ad5933dfcdd69ee09471caa23d",
}


def key(shape, with_bias, divisor):
    return "%s|bias=%d|div=%g" % ("x".join(map(str, shape)), int(with_bias), divisor)


def inputs(shape, with_bias):
    """seeded by the shape alone (numpy's PCG64 stream is the same everywhere): image, filter, bias"""
    B, C, H, W = shape
    rng = np.random.default_rng(9000 + 7 * H + W + int(with_bias))
    img = torch.from_numpy(rng.integers(0, 256, (B, H, W, C), dtype=np.uint8)).to(DEV).permute(0, 3, 1, 2)
    w = torch.from_numpy((rng.standard_normal((64, 3, 7, 7)) * 0.05).astype(np.float16)).to(DEV)
    b = torch.from_numpy((rng.standard_normal(64) * 0.1).astype(np.float16)).to(DEV) if with_bias else None
    return img, w, b


def digest(out):
    """SHA-256 of the output in its storage order [B,Hp,Wp,64]"""
    return hashlib.sha256(out.permute(0, 2, 3, 1).contiguous().cpu().numpy().tobytes()).hexdigest()


def run(shape, with_bias, divisor):
    from s2anet_amd.fused import stem_pack_weight, stem_u8
    img, w, b = inputs(shape, with_bias)
    wp = stem_pack_weight(w)
    return img, w, b, wp, stem_u8(img, wp, b, divisor)


def record():
    """print the HASHES table of the library that is loaded (run on the parent build only)"""
    for shape, wb, d in CASES:
        print('    "%s": "%s",' % (key(shape, wb, d), digest(run(shape, wb, d)[4])))


@pytest.mark.parametrize("shape,with_bias,divisor", CASES, ids=[key(*c) for c in CASES])
def test_stem_reproduces_the_parent_kernel(shape, with_bias, divisor):
    from oracle.conv64 import stem64
    from s2anet_amd import _lib
    img, w, b, wp, out = run(shape, with_bias, divisor)
    B, _, H, W = shape
    assert out.shape == (B, 64, ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1)
    assert digest(out) == HASHES[key(shape, with_bias, divisor)], "k_stem no longer gives the bits of " + PARENT

    again = torch.full_like(out, float("nan"))
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().s2a_stem_u8_f16(_lib.ptr(img), _lib.ptr(wp), _lib.ptr(b), _lib.ptr(again), B, H, W,
                                              float(divisor), _lib.stream_ptr(img.device)))
    assert torch.equal(again, out), "a second launch into a NaN-filled buffer gives other bits"

    y, S = stem64(img, w, b, divisor)
    err = (out.double() - y).abs()
    assert int((~(err <= TAU_STEM * S + TINY)).sum()) == 0, (err / S.clamp_min(1e-300)).max().item() / TAU_STEM
    l2 = err.square().sum().sqrt().item() / max(y.square().sum().sqrt().item(), 1e-300)
    assert l2 <= L2_CONV, l2
    assert int((out != 0).sum()) > 0
