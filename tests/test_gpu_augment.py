"""GPU: the training augmentation (s2anet_amd/augment.py, csrc/augment_ops.hip) against the oracles of tests/augment_cases.py:
images bit for bit, labels within the rounding of one float64 -> float32 conversion, the draw against Philox on Python
integers, the whole of it replayed from a captured graph, and through the detector's training forward.

S2A_AUGMENT_REPORT=<path>: the label tests write their worst error ratios there (profiles/augment.json keeps them)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import augment_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -23                                                   # one f32 ulp at 1


def table_of_all_combos(seed):
    """all 16 (rot, flipud, fliplr), one per image, shuffled"""
    params = np.zeros((16, 4), np.int32)
    params[:, :3] = np.array(AC.COMBOS)[np.random.default_rng(seed).permutation(16)]
    return params


def run_images(aug, imgs, params, **kw):
    labels = torch.zeros((0, 10), device=DEV)
    out, _, _ = aug.apply(torch.from_numpy(imgs).to(DEV), labels, torch.from_numpy(params).to(DEV), **kw)
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def aug():
    import s2anet_amd as S
    return S.TrainAugment(seed=5)


# ---------------------------------------------------------------------------------------------------------- images
@pytest.mark.parametrize("S", [8, 12, 64, 68, 132])
def test_images_all_sixteen_elements_bit_exact(aug, S):
    rng = np.random.default_rng(S)
    imgs = AC.random_images(rng, 16, S)
    params = table_of_all_combos(S)
    want = AC.batch_oracle(imgs, params)
    assert (want == AC.BORDER).any()
    for fill in (7, 200):                                                       # every byte must be written: a byte that is
        out = torch.full((16, S, S, 3), fill, dtype=torch.uint8, device=DEV)    # left alone cannot equal the oracle both times
        got = run_images(aug, imgs, params, out_imgs=out)
        for b in range(16):
            assert np.array_equal(got[b], want[b]), (S, b, params[b], fill)


def test_images_single_image_slice_of_a_larger_allocation_and_nchw_view(aug):
    S = 68
    rng = np.random.default_rng(3)
    for combo in ((1, 0, 1), (2, 1, 0)):
        img = AC.random_images(rng, 1, S)
        params = np.array([combo + (0,)], np.int32)
        assert np.array_equal(run_images(aug, img, params), AC.batch_oracle(img, params))
    big = torch.from_numpy(AC.random_images(rng, 9, S)).to(DEV)
    big_out = torch.full((9, S, S, 3), 7, dtype=torch.uint8, device=DEV)
    params = table_of_all_combos(8)[:4]
    p = torch.from_numpy(params).to(DEV)
    src, dst = big[3:7], big_out[2:6]
    aug.apply(src, torch.zeros((0, 10), device=DEV), p, out_imgs=dst)
    assert np.array_equal(dst.cpu().numpy(), AC.batch_oracle(src.cpu().numpy(), params))
    assert bool((big_out[:2] == 7).all()) and bool((big_out[6:] == 7).all())      # and nothing outside the slice
    # the detector's layout: [B,3,S,S] in channels_last memory
    nchw = src.permute(0, 3, 1, 2)
    out, _, _ = aug.apply(nchw, torch.zeros((0, 10), device=DEV), p)
    assert out.shape == nchw.shape and out.permute(0, 2, 3, 1).is_contiguous()
    assert torch.equal(out.permute(0, 2, 3, 1), dst)


def test_images_refuse_overlap_and_bad_shapes(aug):
    buf = torch.zeros((5, 16, 16, 3), dtype=torch.uint8, device=DEV)
    p = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    none = torch.zeros((0, 10), device=DEV)
    for dst in (buf[:4], buf[1:5]):
        with pytest.raises(RuntimeError, match="overlap"):
            aug.apply(buf[:4], none, p, out_imgs=dst)
    with pytest.raises(RuntimeError, match="square"):
        aug.apply(torch.zeros((4, 16, 20, 3), dtype=torch.uint8, device=DEV), none, p)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        aug.apply(torch.zeros((4, 18, 18, 3), dtype=torch.uint8, device=DEV), none, p)
    with pytest.raises(ValueError):
        aug.apply(torch.zeros((4, 16, 16, 3), device=DEV), none, p)


# ---------------------------------------------------------------------------------------------------------- labels
def corner_sets(boxes):
    """rbox_to_poly of [n,5] float32 rows -> float64 [n,4,2]"""
    from s2anet_amd.formats import rbox_to_poly
    return rbox_to_poly(torch.from_numpy(np.ascontiguousarray(boxes, np.float32)).to(DEV)).cpu().numpy().astype(np.float64).reshape(-1, 4, 2)


def report(key, value):
    path = os.environ.get("S2A_AUGMENT_REPORT")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = value
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


@pytest.mark.parametrize("seed", AC.LABEL_SEEDS)
def test_labels_against_the_float64_oracle(aug, seed):
    S, B = 132, 16
    labels = AC.label_cases(seed, S, B)
    params = table_of_all_combos(seed)
    o = AC.label_oracle(labels, params, S)
    imgs = torch.zeros((B, S, S, 3), dtype=torch.uint8, device=DEV)
    lab_d, par_d = torch.from_numpy(labels).to(DEV), torch.from_numpy(params).to(DEV)
    _, t, status = aug.apply(imgs, lab_d, par_d)
    _, tn, status_n = aug.apply(imgs, lab_d, par_d, normalize=True)
    t, tn, status = t.cpu().numpy(), tn.cpu().numpy(), status.cpu().numpy()
    real = o["fate"] != AC.PADDING
    cmp_ = o["compare"] & real
    assert (~o["compare"][real]).mean() <= 0.05
    # padding rows stay padding; kept / dropped decisions and the counts match exactly on the compared rows
    assert (t[~real, 0] == -1).all() and (t[~real, 1:] == 0).all()
    kept_gpu = t[:, 0] >= 0
    assert np.array_equal(kept_gpu[cmp_], o["fate"][cmp_] == AC.KEPT)
    assert np.array_equal(t[kept_gpu, 0], labels[kept_gpu, 0]) and np.array_equal(t[kept_gpu, 1], labels[kept_gpu, 1])
    assert (t[~kept_gpu, 1:] == 0).all()
    left_out = real & ~o["compare"]
    assert status[0] == real.sum() and status[1] == kept_gpu.sum() and status[1] + status[2] + status[3] == status[0]
    want = AC.status_of(o["fate"], cmp_)
    lo, hi = want, want + np.array([0, left_out.sum(), left_out.sum(), left_out.sum()])
    assert (status[1:] >= lo[1:]).all() and (status[1:] <= hi[1:]).all(), (status, want)
    if not left_out.any():
        assert np.array_equal(status, want)
    assert np.array_equal(status_n.cpu().numpy(), status)

    rows = np.nonzero(cmp_ & (o["fate"] == AC.KEPT))[0]
    got, ref = t[rows, 2:].astype(np.float64), o["box"][rows]
    assert (got[:, 2] >= got[:, 3]).all()
    assert (t[rows, 6] >= np.float32(-math.pi / 4)).all() and (t[rows, 6] < np.float32(3 * math.pi / 4)).all()
    ulp2 = 2 * U32 * np.maximum(np.abs(ref[:, :4]), 1.0)                    # 2 f32 ulps of max(|v|, 1)
    # the centre has one description; sides and angle have two when the box is a square
    ratio_c = np.abs(got[:, :2] - ref[:, :2]) / ulp2[:, :2]
    square = np.abs(ref[:, 2] - ref[:, 3]) <= ulp2[:, 2]
    d_wh = np.abs(got[:, 2:4] - ref[:, 2:4]) / ulp2[:, 2:4]
    period = np.where(square, math.pi / 2, math.pi)
    d_th = np.mod(got[:, 4] - ref[:, 4], period)
    d_th = np.minimum(d_th, period - d_th)
    worst = dict(centre_ulp2=float(ratio_c.max()), sides_ulp2=float(d_wh.max()), theta_over_1e6=float(d_th.max() / 1e-6))
    print("label ratios (error / tolerance), seed", seed, worst, "compared", len(rows), "left out", int(left_out.sum()))
    report("labels_seed_%d" % seed, dict(worst, compared=int(len(rows)), left_out=int(left_out.sum()), rows=int(real.sum())))
    assert ratio_c.max() <= 1.0 and d_wh.max() <= 1.0 and d_th.max() <= 1e-6
    # corner sets (what rbox_to_poly makes of both): a corner is centre +- a e2 +- b e1 in f32.  It moves by the 2 ulps of the
    # centre, 3 for each product (2 of the side, the f32 roundings of the factor and of the product), 2 for the two sums:
    # 10 ulps of the largest coordinate; and by the diagonal times the angle's 1e-6 (twice what half a diagonal sweeps)
    cg, cr = corner_sets(t[rows, 2:]), corner_sets(o["box"][rows].astype(np.float32))
    tol = 10 * U32 * np.maximum(np.abs(cr).max(axis=(1, 2)), 1.0) + 1e-6 * (ref[:, 2] + ref[:, 3])
    dist = np.array([min(np.abs(cg[i] - np.roll(cr[i], k, 0)).max() for k in range(4)) for i in range(len(rows))])
    report("labels_seed_%d_corners" % seed, float((dist / tol).max()))
    assert (dist <= tol).all(), float((dist / tol).max())

    # normalize=True: xywhtheta2xywhtheta_n divides the float64 box, the result is rounded to f32 once
    refn = ref.copy()
    refn[:, :4] /= S
    gotn = tn[rows, 2:].astype(np.float64)
    assert np.array_equal(tn[:, :2], t[:, :2]) and np.array_equal(tn[:, 6], t[:, 6])
    assert (np.abs(gotn[:, :4] - refn[:, :4]) <= 2 * U32 * np.maximum(np.abs(refn[:, :4]), 2.0 ** -8)).all()
    # against the pixel form divided in float64: the pixel form's own rounding (half an ulp) and the quotient's
    assert (np.abs(gotn[:, :4] * S - got[:, :4]) <= 1.01 * U32 * np.maximum(np.abs(got[:, :4]), S * 2.0 ** -8)).all()


def test_label_targets_feed_the_batched_assignment(aug):
    import s2anet_amd as S
    size, B = 132, 16
    labels = AC.label_cases(AC.LABEL_SEEDS[0], size, B)
    params = table_of_all_combos(2)
    imgs = torch.zeros((B, size, size, 3), dtype=torch.uint8, device=DEV)
    _, t, status = aug.apply(imgs, torch.from_numpy(labels).to(DEV), torch.from_numpy(params).to(DEV))
    anchors = S.grid_anchors((17, 17), 8, device=DEV)
    ids, ts, offsets, st = S.assign_labels_batched([anchors], t, B, imgs_size=(size, size))
    torch.cuda.synchronize()
    assert int(st[0]) == 0 and int(st[2]) == int(status[1]) and int(offsets[-1]) == int(status[1])
    assert int((ids >= 0).sum()) > 0


# ------------------------------------------------------------------------------------------------------------ draw
@pytest.mark.parametrize("step", [0, (1 << 32) + 5])
def test_draw_equals_python_philox(step):
    import s2anet_amd as S
    B, seed = 4096, 0x1234567887654321
    a = S.TrainAugment(degrees=180.0, flipud=0.25, fliplr=0.5, seed=seed)
    a.step.fill_(step)
    got = a.draw(B).cpu().numpy()
    assert int(a.step) == step + 1
    want = AC.draw_table(B, step, seed, 180.0, 0.25, 0.5)
    assert np.array_equal(got, want)
    if step == 0:
        counts = np.bincount(got[:, 0], minlength=4)
        assert (np.abs(counts - 1024) <= 5 * 27.7).all(), counts                # binomial(4096, 1/4): sigma 27.7
        assert abs(int(got[:, 2].sum()) - 2048) <= 5 * 32                       # binomial(4096, 1/2): sigma 32
        again = a.draw(B).cpu().numpy()
        assert int(a.step) == 2 and np.array_equal(again, AC.draw_table(B, 1, seed, 180.0, 0.25, 0.5))
        assert not np.array_equal(again, got)


def test_draw_switches():
    import s2anet_amd as S
    B = 1000                                                                    # not a multiple of the wave
    t = S.TrainAugment(degrees=0.0, flipud=0.0, fliplr=1.0, seed=9).draw(B).cpu().numpy()
    assert (t[:, 0] == 0).all() and (t[:, 1] == 0).all() and (t[:, 2] == 1).all() and (t[:, 3] == 0).all()
    t = S.TrainAugment(degrees=180.0, flipud=1.0, fliplr=0.0, seed=9).draw(B).cpu().numpy()
    assert (t[:, 1] == 1).all() and (t[:, 2] == 0).all() and len(np.unique(t[:, 0])) == 4
    out = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    a = S.TrainAugment(seed=-3)
    assert a.draw(B, out=out) is out
    assert np.array_equal(out.cpu().numpy(), AC.draw_table(B, 0, -3, 180.0, 0.0, 0.5))


# --------------------------------------------------------------------------------------------------------- capture
def test_draw_images_and_labels_replay_from_one_graph():
    import s2anet_amd as S
    size, B, seed = 68, 4, 77
    rng = np.random.default_rng(4)
    a = S.TrainAugment(degrees=180.0, flipud=0.5, fliplr=0.5, seed=seed)
    imgs = torch.from_numpy(AC.random_images(rng, B, size)).to(DEV)
    lab = AC.label_cases(AC.LABEL_SEEDS[1], size, B, n=40)
    labels = torch.from_numpy(lab).to(DEV)
    params = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    out_i = torch.empty_like(imgs)
    out_t = torch.empty((labels.shape[0], 7), device=DEV)
    out_s = torch.empty(4, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a(imgs, labels, params=params, out_imgs=out_i, out_targets=out_t, out_status=out_s)      # warm-up off the graph
    torch.cuda.current_stream().wait_stream(side)
    a.step.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a(imgs, labels, params=params, out_imgs=out_i, out_targets=out_t, out_status=out_s)
    assert int(a.step) == 0                                                      # capturing runs nothing
    tables = []
    for step in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert int(a.step) == step + 1
        want = AC.draw_table(B, step, seed, 180.0, 0.5, 0.5)
        assert np.array_equal(params.cpu().numpy(), want)
        tables.append(want)
        e_i, e_t, e_s = a.apply(imgs, labels, torch.from_numpy(want).to(DEV))
        assert torch.equal(out_i, e_i) and torch.equal(out_s, e_s)
        assert torch.equal(out_t.view(torch.int32), e_t.view(torch.int32))
        assert np.array_equal(out_i.cpu().numpy(), AC.batch_oracle(imgs.cpu().numpy(), want))
    assert len({t.tobytes() for t in tables}) == 3


# ------------------------------------------------------------------------------------------------------ end to end
def test_augmented_batch_trains_the_detector():
    import s2anet_amd as S
    from s2anet_amd.detector import build_synthetic_detector
    size, B = 64, 2
    model = build_synthetic_detector().train()
    S.train_kernels(model, True, strided=True, entry=True)
    for p in model.parameters():
        p.requires_grad_(True)
    rng = np.random.default_rng(6)
    imgs = torch.from_numpy(AC.random_images(rng, B, size)).to(DEV).permute(0, 3, 1, 2)       # [B,3,S,S] channels_last
    # axis-aligned boxes with whole corners: their conversion is exact in f32, so both routes see the same bits
    quads = []
    for b, (x0, y0, w, h) in enumerate([(8, 10, 30, 16), (20, 24, 12, 28)]):
        quads.append([b, 3 + b, x0 + .5, y0 + .5, x0 + w + .5, y0 + .5, x0 + w + .5, y0 + h + .5, x0 + .5, y0 + h + .5])
    labels = torch.tensor(quads, dtype=torch.float32, device=DEV)
    a = S.TrainAugment(degrees=180.0, flipud=0.5, fliplr=0.5, seed=1)

    def loss_of(batch, targets):
        for p in model.parameters():
            p.grad = None
        with torch.enable_grad():
            loss = model(batch, targets.clone())["loss"]
            loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss).all())
        assert any(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
                   for p in model.parameters())
        return loss.detach().clone()

    out, targets, status = a(imgs, labels, normalize=True)
    assert status.tolist() == [2, 2, 0, 0]
    loss_of(out, targets)
    # the identity element: the batch comes back bit for bit, the loss is the unaugmented one
    ident = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    out0, targets0, _ = a.apply(imgs, labels, ident, normalize=True)
    assert torch.equal(out0, imgs)
    o = AC.label_oracle(labels.cpu().numpy(), ident.cpu().numpy(), size)
    plain = np.concatenate([labels.cpu().numpy()[:, :2].astype(np.float64), o["box"]], 1)
    plain[:, 2:6] /= size
    plain = torch.from_numpy(plain.astype(np.float32)).to(DEV)
    assert torch.equal(targets0, plain)
    l_aug, l_plain = loss_of(out0, targets0), loss_of(imgs, plain)
    # the same bits go in; only the order of the loss's float atomics may differ between two runs
    assert torch.allclose(l_aug, l_plain, rtol=1e-5, atol=0), (l_aug, l_plain)
