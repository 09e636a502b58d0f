"""CPU: s2a_conv1x1_chain_f16 refuses bad arguments with S2A_EINVAL and a message before any HIP call."""
import ctypes


def test_conv1x1_chain_argument_checks_without_touching_the_gpu():
    from s2anet_amd import _lib
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)          # never dereferenced: the checks fail first
    odd = ctypes.c_void_p(18)          # misaligned

    def msg():
        return L.s2a_last_error().decode()

    def call(x=one, w=one, b=one, r=z, out=one, cw=one, cb=one, cout=one, O3=128, B=1, K=128, O=512, H=8, W=8):
        return L.s2a_conv1x1_chain_f16(x, w, b, r, out, cw, cb, cout, O3, B, K, O, H, W, z)
    # shapes outside the list the kernel is built for
    for K, O, O3 in ((64, 256, 64), (128, 512, 64), (256, 1024, 128), (256, 1024, 512), (512, 2048, 512), (128, 1024, 256)):
        assert call(K=K, O=O, O3=O3) == _lib.EINVAL and "built for" in msg(), (K, O, O3)
    # chain filter, bias and output go together
    assert call(cout=z) == _lib.EINVAL and "go together" in msg()
    assert call(cb=z) == _lib.EINVAL and "go together" in msg()
    assert call(cw=z, cb=z, cout=z) == _lib.EINVAL and "NULL" in msg()
    # NULL tensors, alignment, size, empty batch
    assert call(x=z) == _lib.EINVAL and "NULL" in msg()
    assert call(b=z) == _lib.EINVAL and "NULL" in msg()
    for kw in (dict(x=odd), dict(out=odd), dict(r=odd), dict(cw=odd), dict(cout=odd), dict(w=odd)):
        assert call(**kw) == _lib.EINVAL and "aligned" in msg(), kw
    assert call(B=1 << 12, H=1 << 10, W=1 << 10) == _lib.EINVAL and "32-bit" in msg()
    assert call(B=-1) == _lib.EINVAL and "bad shape" in msg()
    assert call(B=0) == _lib.OK
