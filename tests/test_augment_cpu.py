"""CPU: the training augmentation's surface -- symbols exported and bound, Philox known answers, argument checks that answer
before any HIP call, from_hyp, and the self-checks of the oracles in tests/augment_cases.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import augment_cases as AC

AUGMENT_SYMBOLS = ("s2a_augment_draw", "s2a_augment_images_u8", "s2a_augment_labels")


def test_symbols_are_exported_and_bound_and_take_no_workspace():
    import s2anet_amd as S
    from s2anet_amd import _lib
    L = _lib.lib()
    for name in AUGMENT_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert "TrainAugment" in S.__all__ and callable(S.TrainAugment)
    assert not [n for n in _lib.SYMBOLS if "augment" in n and n.endswith("_workspace_bytes")]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(s2a_\w+_workspace_bytes)\b", out))
    assert len(exported) == 20 and not [n for n in exported if "augment" in n]


def test_philox_known_answers():
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((AC.M32,) * 4, (AC.M32,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for counter, key, want in cases:
        assert " ".join("%08x" % w for w in AC.philox4x32_10(counter, key)) == want


def test_argument_checks_return_codes_without_touching_the_gpu():
    from s2anet_amd import _lib
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    a, b = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)     # never dereferenced: the checks fail first

    def msg():
        return L.s2a_last_error().decode()

    def draw(step=a, seed=a, batch=4, p_ud=0.0, p_lr=0.5, params=a):
        return L.s2a_augment_draw(step, seed, batch, 1, p_ud, p_lr, params, z)

    def images(src=a, params=a, batch=2, h=64, w=64, dst=b):
        return L.s2a_augment_images_u8(src, params, batch, h, w, dst, z)

    def labels(lab=a, rows=5, params=a, batch=2, h=64, w=64, targets=b, status=a):
        return L.s2a_augment_labels(lab, rows, params, batch, h, w, 0, targets, status, z)

    for kw in (dict(step=z), dict(seed=z), dict(params=z)):
        assert draw(**kw) == _lib.EINVAL and "NULL" in msg(), kw
    for n in (0, -1):
        assert draw(batch=n) == _lib.EINVAL and "batch" in msg()
    for kw in (dict(p_ud=-0.1), dict(p_ud=1.5), dict(p_lr=-1.0), dict(p_lr=1.0001), dict(p_lr=math.nan)):
        assert draw(**kw) == _lib.EINVAL and "[0, 1]" in msg(), kw

    for kw in (dict(src=z), dict(params=z), dict(dst=z)):
        assert images(**kw) == _lib.EINVAL and "NULL" in msg(), kw
    for kw in (dict(batch=0), dict(batch=-2), dict(h=0, w=0), dict(h=-64, w=-64)):
        assert images(**kw) == _lib.EINVAL and "positive" in msg(), kw
    assert images(h=64, w=68) == _lib.EINVAL and "square" in msg()
    for s in (66, 63, 4):
        assert images(h=s, w=s) == _lib.EINVAL and "multiple of 4" in msg(), s
    nbytes = 2 * 64 * 64 * 3
    for dst in (a, ctypes.c_void_p((1 << 20) + nbytes - 4), ctypes.c_void_p((1 << 20) - nbytes + 4)):
        assert images(dst=dst) == _lib.EINVAL and "overlap" in msg()
    assert images(src=ctypes.c_void_p((1 << 20) + 2)) == _lib.EINVAL and "aligned" in msg()

    for kw in (dict(lab=z), dict(params=z), dict(targets=z), dict(status=z)):
        assert labels(**kw) == _lib.EINVAL and "NULL" in msg(), kw
    for kw in (dict(rows=0), dict(rows=-1), dict(batch=0), dict(h=0, w=0)):
        assert labels(**kw) == _lib.EINVAL and "positive" in msg(), kw
    assert labels(h=64, w=60) == _lib.EINVAL and "square" in msg()
    assert labels(h=66, w=66) == _lib.EINVAL and "multiple of 4" in msg()


# the augmentation entries of the reference's data/hyps/hyp.scratch.s2anet.yaml
HYP_S2ANET = dict(hsv_h=0.0, hsv_s=0.0, hsv_v=0.0, degrees=180.0, translate=0.0, scale=0.0, shear=0.0, perspective=0.0,
                  flipud=0.0, fliplr=0.5, mosaic=0.0, mixup=0.0, copy_paste=0.0)


def test_from_hyp_reads_the_recipe_and_refuses_what_is_not_built(monkeypatch):
    from s2anet_amd import augment
    made = {}

    def init(self, degrees=180.0, flipud=0.0, fliplr=0.5, seed=0, device="cuda"):
        made.update(degrees=degrees, flipud=flipud, fliplr=fliplr, seed=seed)

    monkeypatch.setattr(augment.TrainAugment, "__init__", init)             # no GPU here: only what from_hyp passes on
    augment.TrainAugment.from_hyp(dict(HYP_S2ANET, lr0=0.01, momentum=0.937), seed=7)
    assert made == dict(degrees=180.0, flipud=0.0, fliplr=0.5, seed=7)
    for key in augment.UNSUPPORTED_HYP:
        with pytest.raises(ValueError, match=key):
            augment.TrainAugment.from_hyp(dict(HYP_S2ANET, **{key: 0.015}))
    assert "hsv_h" in augment.UNSUPPORTED_HYP


def test_wrapper_refuses_cpu_tensors_and_a_cpu_device():
    import s2anet_amd as S
    with pytest.raises(NotImplementedError):
        S.TrainAugment(device="cpu")
    with pytest.raises(ValueError):
        S.TrainAugment(fliplr=1.5)
    aug = object.__new__(S.TrainAugment)
    with pytest.raises(NotImplementedError):
        aug.apply(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 10), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        aug(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 10))


# ----------------------------------------------------------------------------------------------- oracle self-checks
def test_reference_matrices_are_the_integer_maps():
    S = 1024
    want = {0: [[1, 0, 0], [0, 1, 0]], 1: [[0, 1, 0], [-1, 0, S]], 2: [[-1, 0, S], [0, -1, S]], 3: [[0, -1, S], [1, 0, 0]]}
    for rot in range(4):
        M = AC.reference_matrix(rot, S)
        assert np.abs(M[:2] - np.array(want[rot], np.float64)).max() < 1e-12 and (M[2] == [0, 0, 1]).all()
        pts = np.array([[3.25, 7.5], [1000.0, 12.0], [0.0, 0.0], [511.5, 512.5]])
        mapped = (np.concatenate([pts, np.ones((4, 1))], 1) @ M.T)[:, :2]
        assert np.abs(mapped - AC.turn_points(pts, rot, S)).max() < 1e-9
    assert (AC.reference_matrix(0, S) == np.eye(3)).all()


def test_image_oracle_border_lines():
    rng = np.random.default_rng(5)
    img = AC.random_images(rng, 1, 12)[0]
    assert (img != AC.BORDER).all()
    assert np.array_equal(AC.image_oracle(img, 0, 0, 0), img)
    o = AC.image_oracle(img, 1, 0, 0)
    assert (o[0] == AC.BORDER).all() and (o[1:] != AC.BORDER).all() and np.array_equal(o[1:, 3], img[3, ::-1][:-1])
    o = AC.image_oracle(img, 2, 0, 0)
    assert (o[0] == AC.BORDER).all() and (o[:, 0] == AC.BORDER).all() and (o[1:, 1:] != AC.BORDER).all()
    o = AC.image_oracle(img, 3, 0, 0)
    assert (o[:, 0] == AC.BORDER).all() and (o[:, 1:] != AC.BORDER).all()
    o = AC.image_oracle(img, 1, 1, 1)                                       # the border row moves with the flip
    assert (o[-1] == AC.BORDER).all() and (o[:-1] != AC.BORDER).all()


def boxpoints(box):
    """formats.rbox_to_poly (rotated_box_to_poly_single + cv2.boxPoints) in float64"""
    x, y, w, h, a = box
    if a < 0:
        a += math.pi
    a = a / math.pi * 180
    e1, e2 = w, h
    if a > 90:
        a, e1, e2 = a - 90, h, w
    b_, a_ = math.cos(a * math.pi / 180) * 0.5, math.sin(a * math.pi / 180) * 0.5
    p0 = (x - a_ * e2 - b_ * e1, y + b_ * e2 - a_ * e1)
    p1 = (x + a_ * e2 - b_ * e1, y - b_ * e2 - a_ * e1)
    return np.array([p0, p1, (2 * x - p0[0], 2 * y - p0[1]), (2 * x - p1[0], 2 * y - p1[1])])


def corner_distance(p, q):
    """largest corner distance under the best cyclic match of two quads given in the same winding"""
    return min(np.abs(p - np.roll(q, k, 0)).max() for k in range(4))


def test_label_oracle_inverts_rbox_to_poly_on_integer_rectangles():
    # rectangles with integer corners: axis-aligned ones and ones along (3, 4) / (5, 12) directions
    quads = [np.array([[10, 20], [50, 20], [50, 30], [10, 30]]), np.array([[5, 5], [9, 5], [9, 45], [5, 45]]),
             np.array([[30, 30], [54, 48], [48, 56], [24, 38]]),               # 30 x 10 along (4, 3)
             np.array([[60, 10], [72, 15], [62, 39], [50, 34]]),               # 13 x 26 along (12, 5) / (-5, 12)
             np.array([[40, 40], [60, 60], [50, 70], [30, 50]])]               # along the 45-degree seam
    for q in quads:
        for order in (q, q[::-1], np.roll(q, 2, 0)):
            r = AC.min_area_rect(order)
            assert r is not None
            box, gap = r
            assert box[2] >= box[3] and -math.pi / 4 <= box[4] < 3 * math.pi / 4 and gap == math.inf
            back = boxpoints(box)
            ref = q.astype(np.float64)
            assert min(corner_distance(back, ref), corner_distance(back[::-1], ref)) < 1e-9, (q, box)
    assert AC.min_area_rect(np.array([[1, 1], [1, 1], [1, 1], [1, 1]])) is None
    assert AC.min_area_rect(np.array([[1, 1], [3, 3], [5, 5], [2, 2]])) is None
    concave = AC.min_area_rect(np.array([[30, 30], [60, 45], [30, 60], [40, 45]]))     # the hull is the triangle
    assert concave is not None and abs(concave[0][2] * concave[0][3] - 900.0) < 1e-9


@pytest.mark.parametrize("seed", AC.LABEL_SEEDS)
def test_label_generator_keeps_the_margins_for_all_but_five_percent(seed):
    S, B = 132, 16
    labels = AC.label_cases(seed, S, B)
    assert 180 <= labels.shape[0] <= 230
    frac = labels[:, 2:] - np.floor(labels[:, 2:])
    assert frac.min() >= 0.049 and frac.max() <= 0.951
    rng = np.random.default_rng(seed)
    params = np.zeros((B, 4), np.int32)
    params[:, :3] = np.array(AC.COMBOS)[rng.permutation(16)]
    o = AC.label_oracle(labels, params, S)
    real = o["fate"] != AC.PADDING
    assert (~o["compare"][real]).mean() <= 0.05
    counts = AC.status_of(o["fate"])
    assert counts[1] > 100 and counts[2] > 3 and counts[3] > 10 and (~real).sum() > 10


# --------------------------------------------------------------------------------- the image kernel's tile arithmetic
def test_tile_arithmetic_of_the_image_kernel_on_the_host(tmp_path):
    """tests/augment_tile_walk.cpp walks every workgroup and thread of k_augment_images through the arithmetic the kernel
    takes from csrc/augment_geom.hpp, under AddressSanitizer and UBSan on exact-size heap buffers: no index leaves the source
    rows, the staging tile or the destination, no byte of the tile is read that the load phase did not write, and the
    result is the image oracle's, at sizes below, at and over one and several tiles"""
    from conftest import ROOT
    exe = str(tmp_path / "augment_tile_walk")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "s2anet_amd", "csrc"), os.path.join(ROOT, "tests", "augment_tile_walk.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for S in (8, 12, 64, 68, 132, 260):
        rng = np.random.default_rng(S)
        imgs = AC.random_images(rng, 16, S)
        params = np.zeros((16, 4), np.int32)
        params[:, :3] = np.array(AC.COMBOS)[rng.permutation(16)]
        imgs.tofile(tmp_path / "imgs.bin")
        params.tofile(tmp_path / "params.bin")
        r = subprocess.run([exe, str(S), "16", str(tmp_path / "imgs.bin"), str(tmp_path / "params.bin"), str(tmp_path / "out.bin")],
                           capture_output=True, text=True)
        assert r.returncode == 0, (S, r.stdout[-500:], r.stderr[-2000:])
        got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(16, S, S, 3)
        want = AC.batch_oracle(imgs, params)
        for b in range(16):
            assert np.array_equal(got[b], want[b]), (S, params[b])
