"""CPU: the float64 deformable-conv reference (oracle/dcn64.py) that checks the fused backward at production shapes is
pinned here: against the reference's recorded gradients (tests/golden/dcn_backward_small.npz), the float64 forward
restatement, the float32 C++ oracle, its own error scales and autograd's numerical gradient."""
import numpy as np
import torch

import oracle
from conftest import golden
from oracle.dcn64 import deform_conv64, deform_conv_backward64

F64 = torch.float64


def edge_offsets(rng, B, H, W):
    """offsets whose samples hit every case the sampling rules tell apart: exact integers (one-sided coordinate
    gradient), the bands (-1, 0) and (H-1, H) where only two corners count, the band's edges -1 and H themselves
    (excluded), far outside the image, and ordinary fractional points"""
    off = rng.uniform(-2.5, 2.5, (B, 18, H, W))
    kind = rng.integers(0, 6, (B, 9, H, W))
    ys = np.arange(H).reshape(1, 1, H, 1) - 1 + (np.arange(9) // 3).reshape(1, 9, 1, 1)
    xs = np.arange(W).reshape(1, 1, 1, W) - 1 + (np.arange(9) % 3).reshape(1, 9, 1, 1)
    dy, dx = off[:, 0::2], off[:, 1::2]
    ty = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                   [rng.integers(-1, H + 1, kind.shape).astype(np.float64),           # exact integers, -1 and H included
                    -rng.uniform(0.05, 0.95, kind.shape),                              # (-1, 0)
                    H - 1 + rng.uniform(0.05, 0.95, kind.shape),                       # (H-1, H)
                    rng.choice([-40.0, H + 40.0], kind.shape),                         # far outside
                    rng.integers(0, H, kind.shape) + 0.5], ys + dy)
    tx = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                   [rng.integers(-1, W + 1, kind.shape).astype(np.float64), -rng.uniform(0.05, 0.95, kind.shape),
                    W - 1 + rng.uniform(0.05, 0.95, kind.shape), rng.choice([-40.0, W + 40.0], kind.shape),
                    rng.integers(0, W, kind.shape).astype(np.float64)], xs + dx)
    off[:, 0::2], off[:, 1::2] = ty - ys, tx - xs
    return off.astype(np.float32)             # the points stay exact: integers and f32 offsets of small magnitude


def test_matches_reference_recorded_gradients():
    g = golden("dcn_backward_small.npz")
    t = {k: torch.from_numpy(g[k]) for k in ("x", "offset", "weight", "grad_out")}
    r = deform_conv_backward64(t["x"], t["offset"], t["weight"], t["grad_out"], pos_dtype=torch.float32)
    for k in ("input", "offset", "weight"):
        ref = torch.from_numpy(g["grad_" + k]).to(F64)
        err = (r["grad_" + k] - ref).abs()
        # the recording is the reference's float32 build: within a few float32 roundings per product of S
        assert (err <= 2e-6 * r["S_" + k] + 1e-12).all(), k
        assert err.max() < 1e-5 * max(1.0, ref.abs().max().item()), k


def test_forward_matches_float64_restatement():
    rng = np.random.default_rng(7)
    B, C, H, W, O = 2, 5, 9, 7, 4
    x = rng.standard_normal((B, C, H, W))
    w = rng.standard_normal((O, C, 3, 3))
    off = edge_offsets(rng, B, H, W).astype(np.float64)
    ref = oracle.deform_conv_forward_f64(x, off, w)
    got = deform_conv64(torch.from_numpy(x), torch.from_numpy(off), torch.from_numpy(w)).numpy()
    assert np.abs(got - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


def test_gradients_match_float32_oracle_with_edge_samples():
    rng = np.random.default_rng(11)
    for (B, C, H, W, O) in ((2, 6, 8, 10, 5), (1, 3, 3, 13, 2), (3, 4, 11, 3, 3)):
        x = rng.standard_normal((B, C, H, W)).astype(np.float32)
        w = (rng.standard_normal((O, C, 3, 3)) * 0.3).astype(np.float32)
        off = edge_offsets(rng, B, H, W)
        go = rng.standard_normal((B, O, H, W)).astype(np.float32)
        go[rng.random(go.shape) < 0.4] = 0
        ref = oracle.deform_conv_backward(x, off, w, go)
        r = deform_conv_backward64(*(torch.from_numpy(a) for a in (x, off, w, go)), pos_dtype=torch.float32)
        for k, o in zip(("input", "offset", "weight"), ref):
            got = r["grad_" + k]
            err = (got - torch.from_numpy(o).to(F64)).abs()
            assert (err <= 4e-6 * r["S_" + k] + 1e-12).all(), (k, B, C, H, W, O)
            # S bounds every entry; where S is 0 the gradient is exactly 0 (no sample, no contribution)
            assert (got.abs() <= r["S_" + k] * (1 + 1e-12)).all(), k
            assert (got[r["S_" + k] == 0] == 0).all(), k


def test_scale_is_sum_of_absolute_products():
    """S of each gradient against a brute-force sum over the products that make up each entry (tiny shape)"""
    rng = np.random.default_rng(3)
    B, C, H, W, O = 1, 2, 4, 5, 3
    x = rng.standard_normal((B, C, H, W))
    w = rng.standard_normal((O, C, 3, 3))
    off = edge_offsets(rng, B, H, W).astype(np.float64)
    go = rng.standard_normal((B, O, H, W))
    r = deform_conv_backward64(*(torch.from_numpy(a) for a in (x, off, w, go)))
    s_in, s_off, s_w = np.zeros_like(x), np.zeros_like(off), np.zeros_like(w)
    for y in range(H):
        for xq in range(W):
            for t in range(9):
                h = y - 1 + t // 3 + off[0, 2 * t, y, xq]
                ww = xq - 1 + t % 3 + off[0, 2 * t + 1, y, xq]
                if not (-1 < h < H and -1 < ww < W):
                    continue
                hl, wl = int(np.floor(h)), int(np.floor(ww))
                lh, lw = h - hl, ww - wl
                for dy, dx, bw, ch, cw in ((0, 0, (1 - lh) * (1 - lw), 1 - lw, 1 - lh), (0, 1, (1 - lh) * lw, lw, 1 - lh),
                                           (1, 0, lh * (1 - lw), 1 - lw, lh), (1, 1, lh * lw, lw, lh)):
                    yy, xx = hl + dy, wl + dx
                    if not (0 <= yy < H and 0 <= xx < W):
                        continue
                    for c in range(C):
                        v = x[0, c, yy, xx]
                        for o in range(O):
                            p = abs(w[o, c, t // 3, t % 3] * go[0, o, y, xq])
                            s_in[0, c, yy, xx] += p * bw
                            s_w[o, c, t // 3, t % 3] += abs(go[0, o, y, xq] * bw * v)
                            s_off[0, 2 * t, y, xq] += p * ch * abs(v)
                            s_off[0, 2 * t + 1, y, xq] += p * cw * abs(v)
    for k, ref in (("input", s_in), ("offset", s_off), ("weight", s_w)):
        assert np.abs(r["S_" + k].numpy() - ref).max() < 1e-12 * max(1.0, ref.max()), k


def test_chunking_does_not_change_the_result():
    rng = np.random.default_rng(5)
    B, C, H, W, O = 2, 7, 6, 9, 3
    args = [torch.from_numpy(a) for a in (rng.standard_normal((B, C, H, W)), edge_offsets(rng, B, H, W),
                                          rng.standard_normal((O, C, 3, 3)), rng.standard_normal((B, O, H, W)))]
    whole = deform_conv_backward64(*args)
    split = deform_conv_backward64(*args, chunk_elems=2 * 9 * H * W)       # two channels per chunk
    for k in whole:
        assert torch.allclose(whole[k], split[k], rtol=1e-13, atol=1e-13), k


def test_autograd_gradcheck_at_non_integer_points():
    rng = np.random.default_rng(9)
    B, C, H, W, O = 1, 2, 4, 5, 2
    x = torch.from_numpy(rng.standard_normal((B, C, H, W))).requires_grad_(True)
    w = torch.from_numpy(rng.standard_normal((O, C, 3, 3))).requires_grad_(True)
    # fractional points (about 0.3 px from every integer: the central differences stay in one cell), some in the bands
    base = rng.integers(-1, 5, (B, 18, H, W)) + rng.choice([0.3, 0.5, 0.7], (B, 18, H, W))
    off = torch.from_numpy(base).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: deform_conv64(a, b, c), (x, off, w), eps=1e-6, atol=1e-7)
    # the chunked backward agrees with autograd of the plain forward
    go = torch.from_numpy(rng.standard_normal((B, O, H, W)))
    gx, goff, gw = torch.autograd.grad(deform_conv64(x, off, w), (x, off, w), go)
    r = deform_conv_backward64(x, off, w, go, scale=False)
    for a, k in ((gx, "grad_input"), (goff, "grad_offset"), (gw, "grad_weight")):
        assert torch.allclose(a, r[k], rtol=1e-12, atol=1e-12), k
