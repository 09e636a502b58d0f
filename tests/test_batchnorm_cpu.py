"""The own training-mode BatchNorm (s2anet_amd/norm.py, csrc/bn_ops.hip, csrc/bn_plan.hpp) without a GPU:

  * tests/bn_plan_walk.cpp, a stand-alone program under AddressSanitizer and UBSan, walks the slice plan through the very
    functions the kernels call: every (P, C) of the GPU grid (tests/test_gpu_train_bn.py) is covered exactly once, empty
    slices merge as identities, the merge of the plan's partials equals the float64 mean / variance on the offset case;
  * the backward identity the two backward kernels are built on, in float64 against autograd of
    F.batch_norm(training=True), with and without residual and ReLU;
  * the truth table of train_bn_ok on CPU tensors: all False, each row for its stated reason;
  * train_batchnorm: 53 on S2ANet(), sets own_grad_norm on the bottlenecks and nothing else;
  * every argument check of the five C entry points: S2A_EINVAL with its message before any HIP call, and the slices
    query; no new *_workspace_bytes symbol and no opaque workspace argument."""
import ctypes
import os
import re
import subprocess

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import ROOT

F64 = torch.float64

# the GPU grid: name -> (B, C, H, W).  The first six are the issue's; the last is there because at 64 channels the plan has
# 256 slices, more than the 180 tiles of 40 x 72: "more tiles than slices" needs 2 x 96 x 96 (576 tiles).  The eighth is the
# only one whose lanes own five rows or more, so that k_bn_stats runs its four-rows-in-flight loop: 3 x 117 x 117 = 41067 rows,
# 192 per slice, the last used slice ragged (tests/test_bn_geometry_cpu.py asserts this from the plan)
SHAPES = {
    "smallest": (2, 64, 1, 1), "ragged": (3, 320, 7, 9), "wide_rows": (2, 2048, 4, 4), "tiles_40x72": (2, 64, 40, 72),
    "offset": (2, 64, 16, 16), "constant_channel": (2, 64, 5, 5), "more_tiles_than_slices": (2, 64, 96, 96),
    "unrolled_ragged": (3, 64, 117, 117),
}
# the trunk's batch-8 shapes of scripts/bench_train_bn.py, covered by the plan walk as well
BENCH_SHAPES = [(8, 64, 256, 256), (8, 256, 256, 256), (8, 128, 128, 128), (8, 512, 128, 128), (8, 1024, 64, 64), (8, 2048, 32, 32)]


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bn_plan_walk") / "bn_plan_walk")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "s2anet_amd", "csrc"), os.path.join(ROOT, "tests", "bn_plan_walk.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, (args, r.stdout[-1000:], r.stderr[-3000:])
        return r.stdout
    return run


def _pc(shape):
    B, C, H, W = shape
    return B * H * W, C


def test_plan_covers_every_shape_of_the_gpu_grid_exactly_once(walk):
    from s2anet_amd import _lib
    L = _lib.lib()
    shapes = list(SHAPES.values()) + BENCH_SHAPES[2:]          # (the two 256 x 256 maps: 5e5 rows, seconds under ASan)
    out = walk("cover", *[v for s in shapes for v in _pc(s)])
    rows = re.findall(r"cover P (\d+) C (\d+): groups (\d+) slices (\d+) rows_per_slice (\d+) tiles (\d+) empty_slices (\d+)", out)
    assert len(rows) == len(shapes), out
    seen = {}
    for s, row in zip(shapes, rows):
        P, C, groups, slices, per, tiles, empty = map(int, row)
        assert (P, C) == _pc(s) and groups == C // 64 and slices == L.s2a_bn_slices(P, C)        # the library's plan is this one
        seen[s] = (slices, tiles, empty)
    assert seen[SHAPES["wide_rows"]][2] == seen[SHAPES["wide_rows"]][0] - 1                     # one tile: every other slice is empty
    assert seen[SHAPES["more_tiles_than_slices"]][1] > seen[SHAPES["more_tiles_than_slices"]][0]
    assert seen[SHAPES["smallest"]][1] == 1 and seen[SHAPES["ragged"]][1] * 32 > 189 > (seen[SHAPES["ragged"]][1] - 1) * 32


def test_empty_slices_merge_as_identities(walk):
    assert "identity ok" in walk("identity")


def test_merged_partials_equal_float64_on_the_offset_case(walk):
    for name in ("offset", "more_tiles_than_slices"):          # (the second: several rows per lane, slices of three tiles)
        out = walk("offset", *_pc(SHAPES[name]))
        m = re.search(r"mean rel err (\S+), variance rel err (\S+) \(plain f32 E\[x\^2\] - mean\^2: (\S+)\)", out)
        assert m, out
        print(out)
        assert float(m.group(1)) <= 2.0 ** -23 and float(m.group(2)) <= 2.0 ** -20


# ----------------------------------------------------------------------------- the backward identity
def own_backward(x, gamma, go, out, relu, eps):
    """what s2a_bn_backward_reduce_f16 + s2a_bn_backward_input_f16 compute, in x's dtype: -> (dx, dgamma, dbeta, g)"""
    dims = (0, 2, 3)
    P = x.numel() // x.shape[1]
    mean = x.mean(dims, keepdim=True)
    invstd = 1 / torch.sqrt(x.var(dims, unbiased=False, keepdim=True) + eps)
    xh = (x - mean) * invstd
    g = torch.where(out <= 0, torch.zeros_like(go), go) if relu else go
    sg, sgx = g.sum(dims, keepdim=True), (g * xh).sum(dims, keepdim=True)
    dx = gamma.view(1, -1, 1, 1) * invstd * (g - sg / P - xh * sgx / P)
    return dx, sgx.flatten(), sg.flatten(), g


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("shape", [(2, 3, 1, 1), (3, 5, 7, 9), (2, 4, 5, 5)], ids=lambda s: "x".join(map(str, s)))
def test_backward_identity_is_autograds(shape, res, relu):
    gen = torch.Generator().manual_seed(sum(shape) + 2 * res + relu)
    x = torch.randn(shape, generator=gen, dtype=F64) * 0.7 + 3.0
    if shape == (2, 4, 5, 5):
        x[:, 1] = 2.5                                           # one channel constant: var = 0, invstd = eps^-1/2
    x.requires_grad_(True)
    gamma = (torch.rand(shape[1], generator=gen, dtype=F64) + 0.5).requires_grad_(True)
    beta = torch.randn(shape[1], generator=gen, dtype=F64).requires_grad_(True)
    r = torch.randn(shape, generator=gen, dtype=F64).requires_grad_(True) if res else None
    eps = 1e-5
    y = F.batch_norm(x, None, None, gamma, beta, True, 0.1, eps)
    if res:
        y = y + r
    out = F.relu(y) if relu else y
    go = torch.randn(shape, generator=gen, dtype=F64)
    out.backward(go)
    dx, dg, db, g = own_backward(x.detach(), gamma.detach(), go, out.detach(), relu, eps)
    assert torch.isfinite(dx).all()
    for name, got, want in (("dx", dx, x.grad), ("dgamma", dg, gamma.grad), ("dbeta", db, beta.grad)) + \
            ((("dres", g, r.grad),) if res else ()):
        assert torch.allclose(got, want, rtol=1e-9, atol=1e-9 * float(want.abs().max() + 1)), (name, float((got - want).abs().max()))


# ----------------------------------------------------------------------------- train_bn_ok
def _cl(shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype).contiguous(memory_format=torch.channels_last)


def _truth_table():
    """(name, x, bn, residual, the words of the reason with the device left out; None: only the device stands in the way)"""
    def bn(c=64, dtype=torch.float32, stats=None, **kw):
        m = nn.BatchNorm2d(c, **kw).to(dtype)
        if stats is not None and m.running_mean is not None:
            m.running_mean, m.running_var = m.running_mean.to(stats), m.running_var.to(stats)
        return m
    x = _cl((2, 64, 3, 5))
    odd_var = bn()
    odd_var.running_var = odd_var.running_var.half()
    mixed = bn()
    mixed.bias.data = mixed.bias.data.half()
    return [
        ("inside_but_cpu", x, bn(), None, None),
        ("inside_f16_params_but_cpu", x, bn(dtype=torch.float16), None, None),
        ("inside_f16_params_f32_stats_but_cpu", x, bn(dtype=torch.float16, stats=torch.float32), None, None),
        ("inside_with_residual_but_cpu", x, bn(), _cl((2, 64, 3, 5)), None),
        ("f32_input", _cl((2, 64, 3, 5), torch.float32), bn(), None, "not float16"),
        ("nchw", torch.zeros((2, 64, 3, 5), dtype=torch.float16), bn(), None, "channels-last"),
        ("3d", torch.zeros((2, 64, 15), dtype=torch.float16), bn(), None, "channels-last"),
        ("channels_differ", x, bn(128), None, "num_features"),
        ("channels_96", _cl((2, 96, 3, 5)), bn(96), None, "multiple of 64"),
        ("one_value", _cl((1, 64, 1, 1)), bn(), None, "fewer than 2"),
        ("not_affine", x, bn(affine=False), None, "not affine"),
        ("no_running_stats", x, bn(track_running_stats=False), None, "running statistics"),
        ("momentum_none", x, bn(momentum=None), None, "momentum"),
        ("f64_params", x, bn(dtype=torch.float64), None, "float16 or both float32"),
        ("weight_f32_bias_f16", x, mixed, None, "float16 or both float32"),
        ("f16_stats_under_f32_params", x, bn(stats=torch.float16), None, "running statistics"),
        ("stats_differ", x, odd_var, None, "running statistics"),
        ("residual_shape", x, bn(), _cl((2, 64, 3, 4)), "residual"),
        ("residual_f32", x, bn(), _cl((2, 64, 3, 5), torch.float32), "residual"),
        ("residual_nchw", x, bn(), torch.zeros((2, 64, 3, 5), dtype=torch.float16), "residual"),
        ("not_a_batchnorm", x, nn.GroupNorm(1, 64), None, "BatchNorm2d"),
    ]


@pytest.mark.parametrize("row", _truth_table(), ids=lambda r: r[0])
def test_train_bn_ok_truth_table(row):
    import s2anet_amd as S
    from s2anet_amd.norm import _bn_problem
    name, x, bn, residual, words = row
    assert S.train_bn_ok(x, bn, residual) is False                       # CPU tensors: every row is outside
    why = _bn_problem(x, bn, residual, need_cuda=False)
    if words is None:
        assert why is None and "GPU" in _bn_problem(x, bn, residual), why
    else:
        assert why is not None and words in why, (name, why)


def test_size_limit_is_stated_without_allocating():
    """2^31 bytes: an f16 meta tensor of 2^30 elements is outside, one row less is inside"""
    from s2anet_amd.norm import _bn_problem
    bn = nn.BatchNorm2d(64)
    big = torch.empty((1, 64, 4096, 4096), dtype=torch.float16, device="meta").contiguous(memory_format=torch.channels_last)
    assert "2^31" in _bn_problem(big, bn, None, need_cuda=False)
    ok = torch.empty((1, 64, 4096, 4095), dtype=torch.float16, device="meta").contiguous(memory_format=torch.channels_last)
    assert _bn_problem(ok, bn, None, need_cuda=False) is None


def test_batch_norm_train_refuses_cpu_tensors():
    import s2anet_amd as S
    with pytest.raises(NotImplementedError):
        S.batch_norm_train(_cl((2, 64, 3, 5)), nn.BatchNorm2d(64))


# ----------------------------------------------------------------------------- the switch
def test_train_batchnorm_counts_53_and_sets_nothing_else():
    import s2anet_amd as S
    from s2anet_amd.detector import BottleNeck, S2ANet, fuse_epilogues
    from s2anet_amd.fused import FusedConv2d
    assert BottleNeck.own_grad_norm is False
    model = fuse_epilogues(S2ANet())
    before = {id(m): dict(m.__dict__) for m in model.modules()}
    keys = list(model.state_dict())
    assert S.train_batchnorm(model) == 53
    blocks = [m for m in model.modules() if isinstance(m, BottleNeck)]
    assert len(blocks) == 16 and all(m.own_grad_norm is True for m in blocks)
    for m in model.modules():
        added = set(m.__dict__) - set(before[id(m)])
        assert added == ({"own_grad_norm"} if isinstance(m, BottleNeck) else set()), (type(m), added)
    convs = [m for m in model.modules() if isinstance(m, FusedConv2d)]
    assert convs and not any(m.own_grad or m.own_grad_strided or m.own_grad_entry for m in convs)
    assert all(type(m) is nn.BatchNorm2d for m in model.modules() if isinstance(m, nn.BatchNorm2d)) and list(model.state_dict()) == keys
    assert S.train_kernels(model, True, strided=True, entry=True) == len(convs)          # its count does not move
    assert all(m.own_grad_norm is True for m in blocks)
    assert S.train_batchnorm(model, False) == 53 and not any(m.own_grad_norm for m in blocks)


def test_cpu_training_forward_keeps_the_stock_route():
    """the flag on a CPU block: the predicates refuse, the block runs what it runs today, bit for bit"""
    import copy
    import s2anet_amd as S
    from s2anet_amd.detector import BottleNeck
    torch.manual_seed(0)
    blk = BottleNeck(256, 64).train()
    twin = copy.deepcopy(blk)
    assert S.train_batchnorm(blk) == 3 and blk.own_grad_norm and not twin.own_grad_norm
    x = torch.randn((2, 256, 5, 6))
    assert not blk._own_norm_ok(x) and not blk._own_norm_ok(x.half().contiguous(memory_format=torch.channels_last))
    assert torch.equal(blk(x), twin(x)) and torch.equal(blk.bn3.running_var, twin.bn3.running_var)
    assert int(blk.bn1.num_batches_tracked) == 1


# ----------------------------------------------------------------------------- the C ABI
def _err():
    from s2anet_amd import _lib
    return _lib.lib().s2a_last_error().decode()


PTR, ODD, ODD2 = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10008), ctypes.c_void_p(0x10002)   # never dereferenced
NULL = ctypes.c_void_p(0)
P_OK, C_OK = 189, 320


def _calls(L, P, C, slices, f32=0):
    """the four entry points on fake pointers -> {name: (function, argument list, indices of (16-byte, 4-byte) pointers)}"""
    return {
        "bn_train_stats": (L.s2a_bn_train_stats_f16, [PTR, P, C, 1e-5, 0.1, PTR, slices, PTR, PTR, PTR, PTR, f32, NULL],
                           (0, 5), (7, 8, 9, 10)),
        "bn_train_apply": (L.s2a_bn_train_apply_f16, [PTR, PTR, PTR, PTR, PTR, f32, PTR, PTR, P, C, 1, NULL], (0, 6, 7), (1, 2, 3, 4)),
        "bn_backward_reduce": (L.s2a_bn_backward_reduce_f16, [PTR, PTR, PTR, PTR, PTR, PTR, PTR, slices, PTR, PTR, f32, PTR, P, C, NULL],
                               (0, 1, 2, 5, 6), (3, 4, 8, 9, 11)),
        "bn_backward_input": (L.s2a_bn_backward_input_f16, [PTR, PTR, PTR, PTR, PTR, PTR, f32, PTR, PTR, P, C, NULL],
                              (0, 1, 2, 8), (3, 4, 5, 7)),
    }


BAD_PC = [((189, 96), "multiple of 64"), ((189, 0), "multiple of 64"), ((189, -64), "multiple of 64"), ((1, 64), "at least 2"),
          ((0, 64), "at least 2"), ((-5, 64), "at least 2"), ((1 << 24, 64), "too large"), ((2, 1 << 29), "too large"),
          (((1 << 31) + 2, 64), "too large")]


@pytest.mark.parametrize("pc,words", BAD_PC, ids=["%dx%d" % pc for pc, _ in BAD_PC])
def test_bad_shapes_are_refused_by_the_query_and_all_four(pc, words):
    from s2anet_amd import _lib
    L = _lib.lib()
    assert L.s2a_bn_slices(*pc) == 0
    for name, (fn, args, _, _) in _calls(L, pc[0], pc[1], 1).items():
        assert fn(*args) == _lib.EINVAL and name in _err() and words in _err(), (name, _err())


def test_slices_query():
    from s2anet_amd import _lib
    L = _lib.lib()
    for shape in list(SHAPES.values()) + BENCH_SHAPES:
        P, C = _pc(shape)
        n = L.s2a_bn_slices(P, C)
        assert 0 < n <= 256 and L.s2a_bn_slices(P, C) == n and n * 2 * C * 4 <= 1 << 20, (shape, n)     # partial: at most 1 MiB
        assert L.s2a_bn_slices(P + 1, C) == n                       # the channel count alone moves it
    assert L.s2a_bn_slices(1 << 23, 64) == 256 and L.s2a_bn_slices((1 << 24) - 1, 64) == 256 and L.s2a_bn_slices(1 << 24, 64) == 0


def test_null_and_misaligned_pointers_are_refused():
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_bn_slices(P_OK, C_OK)
    optional = {"bn_train_stats": (9, 10), "bn_train_apply": (6,), "bn_backward_reduce": (1, 2, 3, 4, 5, 6, 8, 9, 11),
                "bn_backward_input": (2,)}
    for name, (fn, args, wide, narrow) in _calls(L, P_OK, C_OK, n).items():
        for i in wide + narrow:
            if i not in optional[name]:
                bad = list(args)
                bad[i] = NULL
                assert fn(*bad) == _lib.EINVAL and name in _err() and "NULL" in _err(), (name, i, _err())
            for odd in ((ODD, ODD2) if i in wide else (ODD2,)):
                bad = list(args)
                bad[i] = odd
                assert fn(*bad) == _lib.EINVAL and name in _err() and "aligned" in _err(), (name, i, _err())
    # pointers that go together
    stats, args = L.s2a_bn_train_stats_f16, _calls(L, P_OK, C_OK, n)["bn_train_stats"][1]
    assert stats(*(args[:9] + [NULL, PTR] + args[11:])) == _lib.EINVAL and "go together" in _err()
    assert stats(*(args[:11] + [2] + args[12:])) == _lib.EINVAL and "f32 or f16" in _err()
    red, args = L.s2a_bn_backward_reduce_f16, _calls(L, P_OK, C_OK, n)["bn_backward_reduce"][1]
    assert red(*(args[:2] + [NULL] + args[3:])) == _lib.EINVAL and "needs the forward output" in _err()       # g without out
    assert red(*(args[:5] + [NULL, NULL] + args[7:])) == _lib.EINVAL and "nothing to write" in _err()
    assert red(*(args[:6] + [NULL] + args[7:])) == _lib.EINVAL and "need partial" in _err()                  # gradients, no sums
    assert red(*(args[:11] + [NULL] + args[12:])) == _lib.EINVAL and "NULL" in _err()                        # sums without coef
    assert red(*(args[:10] + [2] + args[11:])) == _lib.EINVAL and "f32 or f16" in _err()
    for name in ("bn_train_apply", "bn_backward_input"):
        fn, args = _calls(L, P_OK, C_OK, n, f32=2)[name][:2]
        assert fn(*args) == _lib.EINVAL and "f32 or f16" in _err(), name


def test_a_slice_count_other_than_the_querys_is_refused():
    from s2anet_amd import _lib
    L = _lib.lib()
    n = L.s2a_bn_slices(P_OK, C_OK)
    for s in (0, -1, n - 1, n + 1):
        for name in ("bn_train_stats", "bn_backward_reduce"):
            fn, args = _calls(L, P_OK, C_OK, s)[name][:2]
            assert fn(*args) == _lib.EINVAL and "slices is %d" % s in _err() and "answers %d" % n in _err(), (name, _err())


def test_no_new_workspace_query_and_no_opaque_workspace():
    from s2anet_amd import _lib
    _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert len(set(re.findall(r"\b(s2a_\w+_workspace_bytes)\b", out))) == 20
    new = sorted(n for n in _lib.SYMBOLS if n.startswith("s2a_bn_"))
    assert new == ["s2a_bn_backward_input_f16", "s2a_bn_backward_reduce_f16", "s2a_bn_slices", "s2a_bn_train_apply_f16",
                   "s2a_bn_train_stats_f16"]
    hdr = open(os.path.join(ROOT, "include", "s2anet_hip.h")).read()
    for n in new:
        assert re.search(r"\b%s\b" % n, out) and re.search(r"\b%s\(" % n, hdr), n
        assert ctypes.c_size_t not in _lib.SYMBOLS[n][1]
    assert "torch.nn.BatchNorm2d" in hdr and "models/backbone.py:54-83" in hdr
