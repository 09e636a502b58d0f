"""CPU: the parallel TP/FP rule of the device evaluation (claim_tp_fp) against the reference's greedy loop (mark_tp_fp),
and the host bookkeeping of Task1Evaluator as far as it runs without a device."""
import numpy as np
import pytest
import torch


def random_case(rng, n, g, share):
    """n detections in confidence order against g ground truths: overlaps around the threshold, a part without any
    ground truth (argmax -1, ovmax -inf), `share` of them piled on two ground truths, 30 % difficult boxes"""
    argmax = rng.integers(0, g, n)
    hot = rng.random(n) < share
    argmax[hot] = rng.integers(0, min(2, g), hot.sum())
    ovmax = np.round(rng.uniform(0.2, 0.9, n), 2)                    # (rounded: values exactly at the threshold occur)
    none = rng.random(n) < 0.15
    argmax[none], ovmax[none] = -1, -np.inf
    return ovmax, argmax, rng.random(g) < 0.3


@pytest.mark.parametrize("filt", [True, False])
def test_claim_rule_equals_greedy_marking(filt):
    from s2anet_amd.evaluate import claim_tp_fp, mark_tp_fp
    rng = np.random.default_rng(5)
    seen = dict(shared=0, none=0, difficult_hit=0, tp=0, fp=0)
    for k in range(300):
        n, g = int(rng.integers(1, 200)), int(rng.integers(1, 12))
        ovmax, argmax, diff = random_case(rng, n, g, share=(0.0, 0.5, 0.9)[k % 3])
        thr = (0.5, 0.7)[k % 2]
        tp, fp = claim_tp_fp(ovmax, argmax, diff, thr, filt)
        wtp, wfp = mark_tp_fp(ovmax, argmax, diff, thr, filt)
        assert np.array_equal(tp, wtp) and np.array_equal(fp, wfp), (k, n, g)
        over = ovmax > thr
        seen["shared"] += int(np.bincount(argmax[over], minlength=g).max() > 3) if over.any() else 0
        seen["none"] += int((argmax == -1).any())
        seen["difficult_hit"] += int(diff[argmax[over]].any()) if over.any() else 0
        seen["tp"] += int(tp.sum())
        seen["fp"] += int(fp.sum())
    assert min(seen.values()) > 50, seen


def test_claim_rule_small_cases():
    from s2anet_amd.evaluate import claim_tp_fp
    # three detections on one ground truth: the first in the order takes it
    tp, fp = claim_tp_fp([0.9, 0.8, 0.6], [0, 0, 0], [0])
    assert tp.tolist() == [1, 0, 0] and fp.tolist() == [0, 1, 1]
    # a filtered difficult box: neither TP nor FP; unfiltered: an ordinary ground truth
    tp, fp = claim_tp_fp([0.9, 0.8], [0, 0], [1])
    assert tp.tolist() == [0, 0] and fp.tolist() == [0, 0]
    tp, fp = claim_tp_fp([0.9, 0.8], [0, 0], [1], is_filter_difficult=False)
    assert tp.tolist() == [1, 0] and fp.tolist() == [0, 1]
    # at the threshold, below it, no ground truth at all: FP; a low detection does not take the box from a later one
    tp, fp = claim_tp_fp([0.5, 0.3, -np.inf, 0.7], [0, 0, -1, 0], [0])
    assert tp.tolist() == [0, 0, 0, 1] and fp.tolist() == [1, 1, 1, 0]
    tp, fp = claim_tp_fp([], [], [])
    assert tp.size == 0 and fp.size == 0


def test_evaluator_host_bookkeeping():
    """offsets, capacities and argument checks are settled on the host, before the device is touched"""
    from s2anet_amd.evaluate import Task1Evaluator, evaluate_task1
    ev = Task1Evaluator(15, max_dets=1000, max_gts=100, max_images=8)
    assert (ev.num_dets, ev.num_gts) == (0, 0)
    assert ev._reserve("dets", 400) == 0 and ev._reserve("dets", 600) == 400 and ev.num_dets == 1000
    with pytest.raises(ValueError, match="do not fit"):
        ev._reserve("dets", 1)
    assert ev._reserve("gts", 99) == 0 and ev._reserve("gts", 0) == 99 and ev._reserve("gts", 1) == 99
    with pytest.raises(ValueError, match="do not fit"):
        ev._reserve("gts", 1)
    assert (ev.num_dets, ev.num_gts) == (1000, 100)
    ev.reset()
    assert (ev.num_dets, ev.num_gts) == (0, 0)
    # a block that does not fit is refused before anything else happens (CPU tensors: the device is never reached)
    dets, labels, counts = torch.zeros(2, 600, 6), torch.zeros(2, 600, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="do not fit"):
        ev.add_detections(dets, labels, counts, [0, 1])
    with pytest.raises(ValueError, match="do not fit"):
        ev.add_ground_truth(torch.zeros(101, 8), torch.zeros(101), 0)
    with pytest.raises(ValueError, match="do not fit"):
        ev.add_polygons(torch.zeros(1001, 8), torch.zeros(1001), torch.zeros(1001), 0)
    assert (ev.num_dets, ev.num_gts) == (0, 0)
    # shapes and image indices
    small = (torch.zeros(2, 10, 6), torch.zeros(2, 10, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"dets \[B,K,6\]"):
        ev.add_detections(torch.zeros(2, 10, 5), small[1], small[2], [0, 1])
    with pytest.raises(ValueError, match=r"dets \[B,K,6\]"):
        ev.add_detections(small[0], torch.zeros(2, 9), small[2], [0, 1])
    with pytest.raises(ValueError, match="one image index per block"):
        ev.add_detections(*small, [0, 1, 2])
    with pytest.raises(ValueError, match="image index outside"):
        ev.add_detections(*small, [0, 8])
    with pytest.raises(ValueError, match="image index outside"):
        ev.add_ground_truth(torch.zeros(3, 8), torch.zeros(3), -1)
    with pytest.raises(ValueError, match="polygons"):
        ev.add_ground_truth(torch.zeros(3, 6), torch.zeros(3), 0)
    with pytest.raises(ValueError, match="difficult"):
        ev.add_ground_truth(torch.zeros(3, 8), torch.zeros(3), 0, torch.zeros(2))
    with pytest.raises(ValueError, match="polys"):
        ev.add_polygons(torch.zeros(3, 8), torch.zeros(3), torch.zeros(4), 0)
    # well-formed CPU tensors: refused as every op of the package refuses them, and nothing was reserved
    with pytest.raises(NotImplementedError):
        ev.add_detections(*small, [0, 1])
    with pytest.raises(NotImplementedError):
        ev.add_ground_truth(torch.zeros(3, 8), torch.zeros(3), 0)
    assert (ev.num_dets, ev.num_gts) == (0, 0)
    # constructor and functional form
    for bad in (dict(num_classes=0), dict(num_classes=1025), dict(max_images=0), dict(max_dets=0), dict(max_gts=1 << 31),
                dict(num_classes=1000, max_images=1 << 22)):
        with pytest.raises(ValueError):
            Task1Evaluator(**dict(dict(num_classes=15, max_dets=10, max_gts=10, max_images=4), **bad))
    z = torch.zeros
    with pytest.raises(ValueError, match=r"det_polys \[D,8\]"):
        evaluate_task1(z(4, 7), z(4), z(4), z(4), z(2, 8), z(2), z(2), z(2), 15, 4)
    with pytest.raises(ValueError, match=r"gt_polys \[G,8\]"):
        evaluate_task1(z(4, 8), z(4), z(4), z(4), z(2, 8), z(2), z(3), z(2), 15, 4)
    with pytest.raises(NotImplementedError):
        evaluate_task1(z(4, 8), z(4), z(4), z(4), z(2, 8), z(2), z(2), z(2), 15, 4)


def test_c_abi_argument_checks():
    """s2a_eval_task1 refuses bad sizes and a short workspace with a return code, before any HIP call"""
    import ctypes
    from s2anet_amd import _lib
    L = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(1 << 20)
    t11 = (ctypes.c_double * 11)(*np.arange(0.0, 1.1, 0.1).tolist())

    def call(D=10, G=5, C=15, I=4, out=one, ws_bytes=1 << 40, det=one, t=t11):
        return L.s2a_eval_task1(det, one, one, one, D, one, one, one, one, G, C, I, 0.5, 1, 1, t, out, one, one, one, one, one, one,
                                one, one, None, one, ws_bytes, z)

    def msg():
        return L.s2a_last_error().decode()
    assert call(D=-1) == _lib.EINVAL and "negative" in msg()
    assert call(D=1 << 31) == _lib.EINVAL and "2^31" in msg()
    assert call(C=0) == _lib.EINVAL and call(C=1025) == _lib.EINVAL and "num_classes" in msg()
    assert call(I=0) == _lib.EINVAL and call(C=1000, I=1 << 22) == _lib.EINVAL and "num_images" in msg()
    assert call(out=z) == _lib.EINVAL and "NULL output" in msg()
    assert call(det=z) == _lib.EINVAL and "NULL detection" in msg()
    assert call(t=None) == _lib.EINVAL and "11" in msg()
    assert call(ws_bytes=16) == _lib.EWORKSPACE and "workspace too small" in msg()
    need = L.s2a_eval_task1_workspace_bytes
    # O(D + G + classes * images): linear in each, no D x G term
    assert need(1 << 20, 1 << 17, 15, 4096) < (1 << 20) * 160
    assert need(2 << 20, 1 << 17, 15, 4096) - need(1 << 20, 1 << 17, 15, 4096) < (1 << 20) * 120
    assert need(1 << 20, 2 << 17, 15, 4096) - need(1 << 20, 1 << 17, 15, 4096) < (1 << 17) * 64
