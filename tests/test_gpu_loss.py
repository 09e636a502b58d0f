"""GPU: the S2ANet training loss (s2anet_amd/loss.py, csrc/loss_ops.hip) against the reference's own compute_loss
(tests/golden/s2anet_loss*.npz, tests/golden/make_golden_loss.py) and against a float64 restatement of
models/head.py:353-646 written here; the two autograd links (fused AlignConv, rot_inv_pool) against their unfused /
torch counterparts; the head end to end."""
import math

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("fam_cls", "fam_bbox", "odm_cls", "odm_bbox")
CASE3 = dict(fl_gamma=1.5, fl_alpha=0.25, smoothL1_beta=0.5, FPN_balance=(1.0, 0.8, 1.2, 0.5, 2.0), reg_balance=2.0,
             odm_balance=0.5)
DEFAULTS = dict(fl_gamma=2.0, fl_alpha=0.5, smoothL1_beta=1.0 / 9.0, FPN_balance=(1.0,) * 5, reg_balance=1.0,
                odm_balance=1.0)


# ----------------------------------------------------------------------------- float64 restatement of the reference
def ref_loss64(p6, ids, ts, offsets, fl_gamma=2.0, fl_alpha=0.5, smoothL1_beta=1.0 / 9.0, FPN_balance=(1.0,) * 5,
               reg_balance=1.0, odm_balance=1.0):
    """compute_loss (head.py:383-436) + compute_loss_single_level (:581-646) + FocalLoss / SmoothL1Loss
    (utils/loss.py) + rboxes_encode (boxes.py:166-221) in float64, given the assignment.  -> (loss [1], items [4])"""
    B = p6[1][0].shape[0]
    C = p6[0][0].shape[1]
    ts = ts.double()
    offsets = offsets.long()
    items = []
    for m in range(2):
        cls_l, box_l, anc_l = p6[2 * m], p6[2 * m + 1], p6[4 + m]
        cls = torch.cat([c.double().permute(0, 2, 3, 1).reshape(B, -1, C) for c in cls_l], 1)
        box = torch.cat([b.double().permute(0, 2, 3, 1).reshape(B, -1, 5) for b in box_l], 1)
        anc = torch.cat([a.detach().double().reshape(-1, a.shape[-3] * a.shape[-2] if a.dim() == 4 else a.shape[0], 5)
                         .expand(B, -1, 5) for a in anc_l], 1)
        w = torch.cat([torch.full((c.shape[2] * c.shape[3],), float(FPN_balance[l]), dtype=torch.float64, device=DEV)
                       for l, c in enumerate(cls_l)])
        idm = ids[m]
        pos, valid = idm >= 0, idm != -2
        row = (offsets[:B, None] + idm.clamp(min=0)).clamp(max=max(ts.shape[0] - 1, 0))
        gt = ts[row] if ts.shape[0] else torch.zeros(B, idm.shape[1], 7, dtype=torch.float64, device=DEV)
        t = torch.zeros_like(cls)
        t.scatter_(2, gt[..., 1].long().clamp(0, C - 1)[..., None], 1.0)
        t = t * pos[..., None]
        p = torch.sigmoid(cls)
        bce = cls.clamp(min=0) - cls * t + torch.log1p(torch.exp(-cls.abs()))
        p_t = t * p + (1 - t) * (1 - p)
        focal = bce * (t * fl_alpha + (1 - t) * (1 - fl_alpha)) * (1.0 - p_t) ** fl_gamma
        cls_sum = (focal.sum(-1) * valid * w).sum()
        ox, oy = gt[..., 2] - anc[..., 0], gt[..., 3] - anc[..., 1]
        ca, sa = torch.cos(anc[..., 4]), torch.sin(anc[..., 4])
        da = torch.remainder(gt[..., 6] - anc[..., 4] + math.pi / 4, math.pi) - math.pi / 4
        tgt = torch.stack([(ca * ox + sa * oy) / anc[..., 2], (-sa * ox + ca * oy) / anc[..., 3],
                           torch.log(gt[..., 4].clamp(min=1e-30) / anc[..., 2]),
                           torch.log(gt[..., 5].clamp(min=1e-30) / anc[..., 3]), da / math.pi], -1)
        d = (box - tgt.detach()).abs()
        sl1 = torch.where(d < smoothL1_beta, 0.5 * d * d / smoothL1_beta, d - 0.5 * smoothL1_beta)
        reg_sum = torch.where(pos, sl1.sum(-1) * w, torch.zeros_like(w)).sum()
        n = max(int(pos.sum()), B)
        bal = odm_balance if m == 1 else 1.0
        items += [cls_sum / n * bal, reg_sum / n * reg_balance * bal]
    items = torch.stack(items)
    return items.sum().reshape(1), items


def grads_close(g, r, rel=1e-4, absm=1e-6):
    g, r = g.double().cpu(), r.double().cpu()
    tol = rel * r.abs() + absm * r.abs().max()
    bad = (g - r).abs() > tol
    assert not bad.any(), ("grad mismatch", int(bad.sum()), float((g - r).abs().max()), float(r.abs().max()))


def golden_p(dtype=torch.float32):
    g = golden("s2anet_loss.npz")
    n = golden("net_forward.npz")
    leaves = [[torch.from_numpy(n["%s_%d" % (k, l)]).to(DEV, dtype).requires_grad_(True) for l in range(5)] for k in NAMES]
    init = [torch.from_numpy(n["init_anchors_%d" % l]).to(DEV) for l in range(5)]
    refine = [torch.from_numpy(n["refine_anchors_%d" % l]).to(DEV) for l in range(5)]
    return g, leaves + [init, refine]


def make_head(**settings):
    from s2anet_amd.head import S2ANetHead
    h = S2ANetHead(15)
    h.imgs_size = (384, 384)
    for k, v in settings.items():
        setattr(h, k, v)
    return h


def all_grads(p):
    return [t.grad for lst in p[:4] for t in lst]


# ----------------------------------------------------------------------------- 1. golden
def test_golden_against_reference_compute_loss():
    g, p = golden_p()
    head = make_head()
    targets = torch.from_numpy(g["targets"]).to(DEV)
    ids, ts, off = head.assign_labels_fam_odm(p, targets)
    assert np.array_equal(ids.cpu().numpy(), g["assign_ids"])
    loss, items = head.compute_loss(p, targets)
    assert isinstance(items, np.ndarray) and items.dtype == np.float32 and loss.shape == (1,)
    np.testing.assert_allclose(items, g["case1_items"], rtol=2e-5, atol=0)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), g["case1_loss"], rtol=2e-5, atol=0)
    loss.backward()
    for k, name in enumerate(NAMES):
        for l in range(5):
            grads_close(p[k][l].grad, torch.from_numpy(g["grad_%s_%d" % (name, l)]))
    # this library's 5-list form (grid anchors generated by the head) gives the same result
    p5 = [[t.detach().clone().requires_grad_(True) for t in lst] for lst in p[:4]] + [p[5]]
    loss5, items5 = head.compute_loss(p5, targets)
    loss5.backward()
    assert np.array_equal(items5, items)
    for a, b in zip(all_grads(p5), all_grads(p)):
        assert torch.equal(a, b)
    # image 1 without gts; non-default settings
    _, p2 = golden_p()
    _, it2 = make_head().compute_loss(p2, torch.from_numpy(g["targets_case2"]).to(DEV))
    np.testing.assert_allclose(it2, g["case2_items"], rtol=2e-5, atol=0)
    _, it3 = make_head(**CASE3).compute_loss(p, targets)
    np.testing.assert_allclose(it3, g["case3_items"], rtol=2e-5, atol=0)


# ----------------------------------------------------------------------------- 2. full size
def full_size_batch(seed=0, B=8, size=1024, n_gt=30, dtype=torch.float32):
    from s2anet_amd.loss import grid_anchors
    gen = torch.Generator(device=DEV).manual_seed(seed)
    strides = (8, 16, 32, 64, 128)
    sizes = [(size // s, size // s) for s in strides]

    def logits(shape):
        x = -4.6 + torch.randn(shape, device=DEV, generator=gen)
        band = torch.rand(shape, device=DEV, generator=gen) < 0.03
        return torch.where(band, (torch.rand(shape, device=DEV, generator=gen) * 60 - 30), x).to(dtype)

    fam_cls = [logits((B, 15, h, w)) for h, w in sizes]
    odm_cls = [logits((B, 15, h, w)) for h, w in sizes]
    fam_box = [(0.5 * torch.randn((B, 5, h, w), device=DEV, generator=gen)).to(dtype) for h, w in sizes]
    odm_box = [(0.5 * torch.randn((B, 5, h, w), device=DEV, generator=gen)).to(dtype) for h, w in sizes]
    init = [grid_anchors(hw, s, 4.0, DEV) for hw, s in zip(sizes, strides)]
    refine = []
    for a, (h, w) in zip(init, sizes):
        r = a.view(1, h, w, 5).repeat(B, 1, 1, 1)
        r[..., :2] += torch.randn((B, h, w, 2), device=DEV, generator=gen) * a[0, 2] * 0.1
        r[..., 2:4] *= torch.exp(torch.randn((B, h, w, 2), device=DEV, generator=gen) * 0.2)
        r[..., 4] = (torch.rand((B, h, w), device=DEV, generator=gen) - 0.25) * math.pi
        refine.append(r)
    t = torch.empty((B * n_gt, 7), device=DEV)
    t[:, 0] = torch.arange(B, device=DEV).repeat_interleave(n_gt).float()
    t[:, 1] = torch.randint(0, 15, (B * n_gt,), device=DEV, generator=gen).float()
    t[:, 2:4] = torch.rand((B * n_gt, 2), device=DEV, generator=gen) * size
    t[:, 4:6] = 8 + torch.rand((B * n_gt, 2), device=DEV, generator=gen) * 200
    t[:, 6] = (torch.rand((B * n_gt,), device=DEV, generator=gen) - 0.25) * math.pi
    t[0, 1], t[1, 1] = 0, 14
    t = t[torch.randperm(B * n_gt, device=DEV, generator=gen)]          # unsorted: the head sorts by image
    p = [fam_cls, fam_box, odm_cls, odm_box, init, refine]
    for lst in p[:4]:
        for x in lst:
            x.requires_grad_(True)
    return p, t


def check_against_restatement(p, ids, ts, off, settings=DEFAULTS, grad_scale=1.0):
    from s2anet_amd import s2anet_loss
    for lst in p[:4]:
        for t in lst:
            t.grad = None
    loss, items = s2anet_loss(*p, ids, ts, off, **settings)
    (loss * 1.0).backward(torch.full_like(loss, grad_scale))
    got = [t.grad.clone() for lst in p[:4] for t in lst]
    for lst in p[:4]:
        for t in lst:
            t.grad = None
    rl, ritems = ref_loss64(p, ids, ts, off, **settings)
    (rl * grad_scale).sum().backward()
    np.testing.assert_allclose(items.cpu().numpy(), ritems.detach().cpu().numpy(), rtol=2e-5, atol=1e-7)
    for a, t in zip(got, [t for lst in p[:4] for t in lst]):
        assert a.dtype == t.dtype
        grads_close(a, t.grad)
    return loss, items, got


def test_full_size_against_float64_restatement():
    head = make_head()
    head.imgs_size = (1024, 1024)
    p, t = full_size_batch()
    ids, ts, off = head.assign_labels_fam_odm(p, t)
    assert int((ids[0] >= 0).sum()) > 100 and int((ids[1] >= 0).sum()) > 10
    check_against_restatement(p, ids, ts, off)
    check_against_restatement(p, ids, ts, off, dict(DEFAULTS, **CASE3))


# ----------------------------------------------------------------------------- 3. f16, 4. determinism
def test_f16_maps_and_determinism():
    from s2anet_amd import s2anet_loss
    head = make_head()
    head.imgs_size = (1024, 1024)
    p16, t = full_size_batch(seed=1, B=2, dtype=torch.float16)
    ids, ts, off = head.assign_labels_fam_odm(p16, t)
    p32 = [[x.detach().float().requires_grad_(True) for x in lst] for lst in p16[:4]] + p16[4:]
    res = []
    for p in (p16, p32, p16):
        loss, items = s2anet_loss(*p, ids, ts, off)
        loss.backward()
        res.append((loss.detach().clone(), items.clone(), [x.grad.clone() for lst in p[:4] for x in lst]))
        for lst in p[:4]:
            for x in lst:
                x.grad = None
    (l16, i16, g16), (l32, i32, g32), (l16b, i16b, g16b) = res
    assert torch.equal(l16, l32) and torch.equal(i16, i32)
    for a, b in zip(g16, g32):
        assert a.dtype == torch.float16 and torch.equal(a, b.half())
    assert torch.equal(l16, l16b) and torch.equal(i16, i16b)
    for a, b in zip(g16, g16b):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 5. edge cases
def test_edge_cases():
    head = make_head()
    _, p = golden_p()
    B = 2
    # a batch without gts: only the negative classification term, divided by B
    ids, ts, off = head.assign_labels_fam_odm(p, torch.zeros((0, 7), device=DEV))
    assert ts.shape == (0, 7) and bool((ids < 0).all())
    loss, items, got = check_against_restatement(p, ids, ts, off)
    assert items[1] == 0 and items[3] == 0 and items[0] > 0
    assert all(bool((g == 0).all()) for g in got[5:10] + got[15:20])           # no regression gradient
    # a level without positives: zero regression gradient there (the golden gts sit on levels 0-2)
    g = golden("s2anet_loss.npz")
    targets = torch.from_numpy(g["targets"]).to(DEV)
    ids, ts, off = head.assign_labels_fam_odm(p, targets)
    loss, items, got = check_against_restatement(p, ids, ts, off, grad_scale=3.5)      # grad_output != 1
    assert bool((got[5 + 4] == 0).all()) and bool((got[15 + 4] == 0).all())
    # every anchor of image 1 ignored: no loss and no gradient from it
    ids2 = ids.clone()
    ids2[:, 1] = -2
    loss2, items2, got2 = check_against_restatement(p, ids2, ts, off)
    for k in (0, 10):                                                           # fam_cls / odm_cls, all levels
        for l in range(5):
            assert bool((got2[k + l][1] == 0).all())
    # gts outside the image: their anchors are negatives or ignored, the loss stays finite
    far = targets.clone()
    far[:, 2:4] += 5000
    ids3, ts3, off3 = head.assign_labels_fam_odm(p, far)
    l3, _, _ = check_against_restatement(p, ids3, ts3, off3)
    assert torch.isfinite(l3).all()


# ----------------------------------------------------------------------------- 6. graph capture
def test_graph_capture_replays_bit_equal_to_eager():
    from s2anet_amd import s2anet_loss
    head = make_head()
    head.imgs_size = (1024, 1024)
    p, t = full_size_batch(seed=2, B=2)
    ids, ts, off = head.assign_labels_fam_odm(p, t)
    maps = [x for lst in p[:4] for x in lst]

    def step():
        loss, items = s2anet_loss(*p, ids, ts, off)
        return (loss, items, *torch.autograd.grad(loss, maps))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    gen = torch.Generator(device=DEV).manual_seed(7)
    for _ in range(2):
        with torch.no_grad():
            for x in maps:
                x.add_(torch.randn(x.shape, device=DEV, generator=gen, dtype=x.dtype) * 0.3)
        graph.replay()
        torch.cuda.synchronize()
        eager = step()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


# ----------------------------------------------------------------------------- 7. autograd links
@pytest.mark.parametrize("dtype,bound", [(torch.float32, 1e-4), (torch.float16, 2e-3)])
def test_fused_alignconv_gradients_match_unfused_route(dtype, bound):
    import s2anet_amd as S
    from s2anet_amd.alignconv import align_conv_forward, align_offsets
    torch.manual_seed(0)
    B, C, H, W, stride = 2, 64, 12, 16, 8
    ac = S.AlignConv(C, 64, 3).to(DEV, dtype)
    with torch.no_grad():
        ac.deform_conv.weight.normal_(0, 0.05)
    from s2anet_amd.loss import grid_anchors
    anc = grid_anchors((H, W), stride, 4.0, DEV).view(1, H, W, 5).repeat(B, 1, 1, 1)
    anc[..., :2] += torch.randn((B, H, W, 2), device=DEV) * 3
    anc[..., 4] = torch.rand((B, H, W), device=DEV) * 3.0 - 0.7
    x = torch.randn((B, C, H, W), device=DEV, dtype=dtype, requires_grad=True)
    assert ac.fused_ok(x)
    out = ac(x, anc, stride)
    assert out.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(out, align_conv_forward(x, anc, ac.deform_conv.weight, stride, relu=True))
        assert torch.equal(out, ac(x, anc, stride))
    go = torch.randn_like(out)
    out.backward(go)
    gx, gw = x.grad.clone(), ac.deform_conv.weight.grad.clone()
    x.grad = None
    ac.deform_conv.weight.grad = None
    offset = align_offsets(anc.reshape(B, H * W, 5), (H, W), stride)
    ref = torch.relu(S.deform_conv(x, offset, ac.deform_conv.weight, 1, 1))
    ref.backward(go)
    for a, r in ((gx, x.grad), (gw, ac.deform_conv.weight.grad)):
        assert a.dtype == r.dtype
        assert float((a.float() - r.float()).abs().max()) <= bound * float(r.float().abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("channels_last", [False, True])
def test_rot_inv_pool_gradient_equals_torch_max(dtype, channels_last):
    import s2anet_amd as S
    torch.manual_seed(1)
    N, c, h, w = 2, 32, 5, 7
    base = torch.randint(0, 3, (N, c, h, w), device=DEV).to(dtype)            # many ties
    base[0, :8] = 1                                                             # a whole group tied
    if channels_last:
        base = base.contiguous(memory_format=torch.channels_last)
    x1 = base.clone().requires_grad_(True)
    x2 = base.clone().requires_grad_(True)
    y1 = S.rot_inv_pool(x1, 8)
    assert y1.grad_fn is not None
    y2 = x2.view(N, c // 8, 8, h, w).max(2)[0] if not channels_last else x2.contiguous().view(N, c // 8, 8, h, w).max(2)[0]
    assert torch.equal(y1, y2)
    go = torch.randn(y1.shape, device=DEV).to(dtype)
    y1.backward(go)
    y2.backward(go)
    assert x1.grad.dtype == dtype and torch.equal(x1.grad, x2.grad)


# ----------------------------------------------------------------------------- 8. end to end
def test_head_end_to_end_trains():
    from s2anet_amd.head import S2ANetHead
    torch.manual_seed(3)
    head = S2ANetHead(15, in_channels=64, feat_channels=64).to(DEV).train()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.Conv2d) and m.weight.shape[-1] == 3:
                m.weight.normal_(0, 0.05)
        head.align_conv.deform_conv.weight.normal_(0, 0.05)
    B, size = 2, 256
    feats = [torch.randn((B, 64, size // s, size // s), device=DEV, requires_grad=True) for s in head.featmap_strides]
    assert head.align_conv.fused_ok(feats[0])
    t = torch.tensor([[0, 3, 0.30, 0.40, 0.20, 0.10, 0.3], [0, 14, 0.70, 0.60, 0.12, 0.25, 1.2],
                      [0, 0, 0.50, 0.20, 0.40, 0.30, -0.5], [1, 7, 0.25, 0.75, 0.15, 0.15, 0.0],
                      [1, 9, 0.55, 0.50, 0.50, 0.22, 2.0]], device=DEV)
    tn = t.clone()
    results = head(feats, tn, (size, size))
    assert torch.equal(tn[:, 2:6], t[:, 2:6] * size)                            # scaled in place
    assert results["pred"] is None and isinstance(results["loss_items"], np.ndarray)
    loss = results["loss"]
    assert loss.shape == (1,) and loss.grad_fn is not None
    loss.backward()
    got = {n: q.grad.clone() for n, q in head.named_parameters()}
    got_f = [f.grad.clone() for f in feats]
    assert got["align_conv.deform_conv.weight"].abs().max() > 0 and got["or_conv.weight"].abs().max() > 0
    # at 256^2 the anchors of strides 64 / 128 (256 / 512 px) are all invalid, so those levels get no gradient
    assert all(float(f.abs().max()) > 0 for f in got_f[:3])
    head.zero_grad(set_to_none=True)
    for f in feats:
        f.grad = None
    p = head(feats)["pred"]
    ids, ts, off = head.assign_labels_fam_odm(p, tn)
    p6 = list(p[:4]) + [head.init_grid_anchors([tuple(b.shape[2:]) for b in p[1]], DEV), p[4]]
    rl, _ = ref_loss64(p6, ids, ts, off)
    rl.sum().backward()
    for n, q in head.named_parameters():
        assert got[n] is not None and q.grad is not None, n
        assert float((got[n] - q.grad).abs().max()) <= 1e-4 * float(q.grad.abs().max()) + 1e-12, n
    for a, f in zip(got_f, feats):
        assert float((a - f.grad).abs().max()) <= 1e-4 * float(f.grad.abs().max())

