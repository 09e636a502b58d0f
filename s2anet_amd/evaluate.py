"""DOTA Task-1 evaluation with the polygon overlaps on the GPU.

``voc_eval_arrays`` is ``voc_eval`` of DOTA_devkit/dota_evaluation_task1.py:92-318 for ONE class on arrays
instead of files: the per-detection search for the best-overlapping ground truth (HBB prefilter + polyiou,
:204-263) is one kernel over all detections (s2a_polyiou_match); the greedy TP/FP marking in confidence order
(:265-290) and the AP integral (:58-89) are the reference's scalar bookkeeping on the host.

``evaluate_task1`` / ``Task1Evaluator`` score ALL classes in one call that never leaves the device (s2a_eval_task1): the
loop over the classes of val.py:332-399 with the max-F1 point of every curve (:357-386) and their means (:395-399).  The
greedy marking becomes the parallel rule that ``claim_tp_fp`` states in NumPy.
"""
import ctypes

import numpy as np
import torch

from . import _lib


def polyiou_match(det_polys, det_image, gt_polys, gt_offsets):
    """det_polys[D,8] f64, det_image[D] int32, gt_polys[G,8] f64 grouped by image, gt_offsets[I+1] int64
    -> ovmax[D] f64 (-inf: no overlapping gt), argmax[D] int64 (index into gt_polys or -1)"""
    _lib.require_cuda(det_polys, det_image, gt_polys, gt_offsets)
    d = det_polys.to(torch.float64).contiguous().reshape(-1, 8)
    g = gt_polys.to(torch.float64).contiguous().reshape(-1, 8)
    img = det_image.to(torch.int32).contiguous()
    off = gt_offsets.to(torch.int64).contiguous()
    D = d.shape[0]
    ov = torch.empty((D,), dtype=torch.float64, device=d.device)
    am = torch.empty((D,), dtype=torch.int64, device=d.device)
    with torch.cuda.device(d.device):
        _lib.check(_lib.lib().s2a_polyiou_match(_lib.ptr(d), _lib.ptr(img), D, _lib.ptr(g), _lib.ptr(off), off.numel() - 1,
                                                _lib.ptr(ov), _lib.ptr(am), _lib.stream_ptr(d.device)))
    return ov, am


def voc_ap(rec, prec, use_07_metric=False):
    """dota_evaluation_task1.py:58-89"""
    if use_07_metric:
        ap = 0.0
        for t in np.arange(0.0, 1.1, 0.1):
            p = 0 if np.sum(rec >= t) == 0 else np.max(prec[rec >= t])
            ap = ap + p / 11.0
        return ap
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def mark_tp_fp(ovmax, argmax, gt_difficult, ovthresh=0.5, is_filter_difficult=True):
    """:265-290 on detections already in descending-confidence order"""
    n = len(ovmax)
    tp, fp = np.zeros(n), np.zeros(n)
    taken = np.zeros(len(gt_difficult), bool)
    for k in range(n):
        if ovmax[k] > ovthresh:
            j = argmax[k]
            if is_filter_difficult and gt_difficult[j]:
                continue
            if not taken[j]:
                tp[k] = 1.0
                taken[j] = True
            else:
                fp[k] = 1.0
        else:
            fp[k] = 1.0
    return tp, fp


def voc_eval_arrays(det_polys, det_scores, det_image, gt_polys, gt_image, gt_difficult, num_images, ovthresh=0.5,
                    is_filter_difficult=True, use_07_metric=False, device="cuda"):
    """one class: detections (polygons[D,8], confidences[D], image index[D]) against ground truth
    (polygons[G,8], image index[G], difficult[G]) -> rec, prec, ap, sorted_scores as voc_eval returns them"""
    det_polys = np.asarray(det_polys, np.float64).reshape(-1, 8)
    det_scores = np.asarray(det_scores, np.float64)
    det_image = np.asarray(det_image, np.int64)
    gt_polys = np.asarray(gt_polys, np.float64).reshape(-1, 8)
    gt_image = np.asarray(gt_image, np.int64)
    gt_difficult = np.asarray(gt_difficult).astype(bool)
    num_gts = int((~gt_difficult).sum()) if is_filter_difficult else int(gt_difficult.shape[0])
    if det_polys.shape[0] == 0:
        return np.zeros(1), np.zeros(1), 0.0, np.zeros(1)
    go = np.argsort(gt_image, kind="stable")                      # group the ground truth by image (file order kept)
    gt_polys, gt_image, gt_difficult = gt_polys[go], gt_image[go], gt_difficult[go]
    offsets = np.zeros(num_images + 1, np.int64)
    np.add.at(offsets, gt_image + 1, 1)
    offsets = np.cumsum(offsets)
    order = np.argsort(-det_scores)                                # :183
    dev = torch.device(device)
    ov, am = polyiou_match(torch.from_numpy(det_polys[order]).to(dev), torch.from_numpy(det_image[order].astype(np.int32)).to(dev),
                           torch.from_numpy(gt_polys).to(dev), torch.from_numpy(offsets).to(dev))
    tp, fp = mark_tp_fp(ov.cpu().numpy(), am.cpu().numpy(), gt_difficult, ovthresh, is_filter_difficult)
    fp, tp = np.cumsum(fp), np.cumsum(tp)
    rec = tp / float(num_gts)
    prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
    return rec, prec, voc_ap(rec, prec, use_07_metric), det_scores[order]


# ---------------------------------------------------------------------------------------------------------------------
# all classes at once, on the device

def claim_tp_fp(ovmax, argmax, gt_difficult, ovthresh=0.5, is_filter_difficult=True):
    """``mark_tp_fp`` without the loop: the rule s2a_eval_task1 runs on the device.

    In voc_eval a detection's best ground truth (ovmax, argmax) does not depend on which ground truths are taken
    already, so the greedy pass in confidence order (:265-290) collapses: a detection QUALIFIES for ground truth j when
    ``ovmax > ovthresh``, ``argmax == j`` and j is not a filtered difficult box; of the detections that qualify for j
    the one with the smallest rank (they are in descending-confidence order) is the TP, all the others are FP.  A
    detection whose best ground truth is a filtered difficult box is neither; one at or below the threshold is FP."""
    ovmax = np.asarray(ovmax, np.float64)
    argmax = np.asarray(argmax, np.int64)
    gt_difficult = np.asarray(gt_difficult).astype(bool)
    n = ovmax.shape[0]
    rank = np.arange(n)
    over = ovmax > ovthresh
    ignored = np.zeros(n, bool)
    if is_filter_difficult and gt_difficult.size:
        ignored[over] = gt_difficult[argmax[over]]
    qualifies = over & ~ignored
    claim = np.full(gt_difficult.shape[0], n, np.int64)             # the device's atomicMin of the rank
    np.minimum.at(claim, argmax[qualifies], rank[qualifies])
    tp = np.zeros(n)
    tp[qualifies] = claim[argmax[qualifies]] == rank[qualifies]
    fp = np.where(ignored, 0.0, 1.0 - tp)
    return tp, fp


THRESHOLDS_11 = np.arange(0.0, 1.1, 0.1)                            # :65, the reference's own table
_T11 = (ctypes.c_double * 11)(*THRESHOLDS_11.tolist())
_CURVES = ("order", "ovmax", "argmax", "tp_cum", "fp_cum", "rec", "prec", "seg_start")


class Task1Result:
    """what ``evaluate_task1`` returns, all on the device.  Per class [num_classes]: ``ap``, ``precision``,
    ``recall``, ``f1``, ``conf`` (f64; P / R / F1 / confidence at the class's max-F1 point, val.py:374-385),
    ``num_det_at_f1``, ``npos``, ``ndet`` (int64), ``valid`` (uint8: 0 for a class without a countable ground truth,
    which reports zeros).  ``curves`` is None or a dict of the per-position arrays of s2a_eval_curves (in the order
    class-major, descending score; ``seg_start[c]:seg_start[c + 1]`` is class c).  ``map50``, ``mp``, ``mr``, ``mf1``,
    ``mconf``: 0-dim device tensors, means over ALL classes as val.py:395-399 takes them."""
    __slots__ = ("ap", "precision", "recall", "f1", "conf", "num_det_at_f1", "npos", "ndet", "valid", "curves")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    map50 = property(lambda self: self.ap.mean())
    mp = property(lambda self: self.precision.mean())
    mr = property(lambda self: self.recall.mean())
    mf1 = property(lambda self: self.f1.mean())
    mconf = property(lambda self: self.conf.mean())

    def summary(self):
        """the single host read: ``((mp, mr, map50, conf), classes_ap50s)`` as val.py:425 returns them (means by
        NumPy on the host, as the reference takes them)"""
        a = torch.stack([self.precision, self.recall, self.ap, self.conf]).cpu().numpy()
        return (a[0].mean().item(), a[1].mean().item(), a[2].mean().item(), a[3].mean().item()), a[2].copy()


def _launch_task1(dp, ds, dl, di, gp, gl, gi, gd, num_classes, num_images, ovthresh, is_filter_difficult, use_07_metric,
                  curves, ws=None, alloc=None):
    dev = dp.device
    D, G, C = dp.shape[0], gp.shape[0], int(num_classes)
    if alloc is None:
        def alloc(name, n, dtype):
            return torch.empty(n, dtype=dtype, device=dev)
    f64, i64 = torch.float64, torch.int64
    res = Task1Result(ap=alloc("ap", C, f64), precision=alloc("precision", C, f64), recall=alloc("recall", C, f64),
                      f1=alloc("f1", C, f64), conf=alloc("conf", C, f64), num_det_at_f1=alloc("num_det_at_f1", C, i64),
                      npos=alloc("npos", C, i64), ndet=alloc("ndet", C, i64), valid=alloc("valid", C, torch.uint8))
    cv = None
    if curves:
        res.curves = {k: alloc(k, C + 1 if k == "seg_start" else D, f64 if k in ("ovmax", "rec", "prec") else i64)
                      for k in _CURVES}
        cv = _lib.EvalCurves(**{k: t.data_ptr() for k, t in res.curves.items()})
    L = _lib.lib()
    with torch.cuda.device(dev):
        if ws is None:
            ws = _lib.workspace(L.s2a_eval_task1_workspace_bytes(D, G, C, int(num_images)), dev, "eval_task1")
        _lib.check(L.s2a_eval_task1(_lib.ptr(dp), _lib.ptr(ds), _lib.ptr(dl), _lib.ptr(di), D, _lib.ptr(gp), _lib.ptr(gl),
                                    _lib.ptr(gi), _lib.ptr(gd), G, C, int(num_images), float(ovthresh),
                                    int(bool(is_filter_difficult)), int(bool(use_07_metric)), _T11,
                                    _lib.ptr(res.ap), _lib.ptr(res.precision), _lib.ptr(res.recall), _lib.ptr(res.f1),
                                    _lib.ptr(res.conf), _lib.ptr(res.num_det_at_f1), _lib.ptr(res.npos), _lib.ptr(res.ndet),
                                    _lib.ptr(res.valid), ctypes.byref(cv) if cv is not None else None, _lib.ptr(ws),
                                    ws.numel(), _lib.stream_ptr(dev)))
    return res


def _check_sizes(num_classes, num_images):
    num_classes, num_images = int(num_classes), int(num_images)
    if not 1 <= num_classes <= 1024:
        raise ValueError("num_classes must be in [1, 1024]")
    if num_images < 1 or (num_classes + 1) * num_images >= 1 << 31:
        raise ValueError("num_images must be >= 1 and (num_classes + 1) * num_images < 2^31")
    return num_classes, num_images


def evaluate_task1(det_polys, det_scores, det_labels, det_image, gt_polys, gt_labels, gt_image, gt_difficult, num_classes,
                   num_images, ovthresh=0.5, is_filter_difficult=True, use_07_metric=True, curves=False, alloc=None):
    """DOTA Task-1 evaluation of all classes (s2a_eval_task1), the functional form.

    Device tensors: det_polys [D,8], det_scores [D], det_labels [D], det_image [D]; gt_polys [G,8], gt_labels [G],
    gt_image [G], gt_difficult [G].  A row whose label is outside [0, num_classes) or whose image is outside
    [0, num_images) is padding: ignored, its polygon and score never interpreted.  No host synchronisation; the call
    can be captured into a HIP graph.  Returns a ``Task1Result`` (``curves=True``: with the per-position arrays).
    ``alloc(name, numel, dtype)``: where every output goes (default: a fresh tensor each)."""
    num_classes, num_images = _check_sizes(num_classes, num_images)
    D, G = int(det_scores.shape[0]), int(gt_labels.shape[0])
    if tuple(det_polys.shape) != (D, 8) or tuple(det_labels.shape) != (D,) or tuple(det_image.shape) != (D,):
        raise ValueError("evaluate_task1: det_polys [D,8], det_scores [D], det_labels [D], det_image [D] expected")
    if tuple(gt_polys.shape) != (G, 8) or tuple(gt_image.shape) != (G,) or tuple(gt_difficult.shape) != (G,):
        raise ValueError("evaluate_task1: gt_polys [G,8], gt_labels [G], gt_image [G], gt_difficult [G] expected")
    if D >= 1 << 31 or G >= 1 << 31:
        raise ValueError("evaluate_task1: 2^31 rows or more are not supported")
    _lib.require_cuda(det_polys, det_scores, det_labels, det_image, gt_polys, gt_labels, gt_image, gt_difficult)
    return _launch_task1(det_polys.to(torch.float64).contiguous(), det_scores.to(torch.float64).contiguous(),
                         det_labels.to(torch.int32).contiguous(), det_image.to(torch.int32).contiguous(),
                         gt_polys.to(torch.float64).contiguous(), gt_labels.to(torch.int32).contiguous(),
                         gt_image.to(torch.int32).contiguous(), gt_difficult.to(torch.uint8).contiguous(), num_classes,
                         num_images, ovthresh, is_filter_difficult, use_07_metric, curves, alloc=alloc)


class Task1Evaluator:
    """a validation run accumulated in static device tables and scored in one call.

    ``max_dets`` / ``max_gts`` rows and ``max_images`` images are the capacities; the tables are allocated on the first
    ``add_*`` and never move.  Every ``add_*`` appends a whole block at an offset the HOST knows (padded rows included:
    they carry label -1), so nothing is ever read back; exceeding a capacity raises ``ValueError`` before any launch.
    ``compute`` always scores the whole tables (unused rows are padding): its launch sequence depends on the capacities
    only, so it can be captured into a HIP graph once and replayed after the tables have been refilled."""

    def __init__(self, num_classes, max_dets, max_gts, max_images, device="cuda"):
        self.num_classes, self.max_images = _check_sizes(num_classes, max_images)
        self.max_dets, self.max_gts = int(max_dets), int(max_gts)
        if not (0 < self.max_dets < 1 << 31 and 0 < self.max_gts < 1 << 31):
            raise ValueError("Task1Evaluator: max_dets and max_gts must be in [1, 2^31)")
        self.device = torch.device(device)
        self.num_dets = self.num_gts = 0                            # rows appended so far (host bookkeeping)
        self._t = None

    # ---- host bookkeeping (no device needed)
    def _check_fits(self, side, n):
        used, cap = (self.num_dets, self.max_dets) if side == "dets" else (self.num_gts, self.max_gts)
        if n < 0 or used + n > cap:
            raise ValueError(f"Task1Evaluator: {n} more {side} rows do not fit ({used} of {cap} used)")
        return used

    def _reserve(self, side, n):
        """offset of a block of n rows on ``side`` ('dets' / 'gts'); ValueError when it does not fit"""
        n = int(n)
        used = self._check_fits(side, n)
        if side == "dets":
            self.num_dets += n
        else:
            self.num_gts += n
        return used

    def _image_column(self, image, n_blocks):
        """image index per block -> host-checked when it is a host value; a device tensor is taken as it is (an index
        out of range makes the rows padding)"""
        if isinstance(image, torch.Tensor) and image.is_cuda:
            if image.numel() != n_blocks:
                raise ValueError("Task1Evaluator: one image index per block expected")
            return image.reshape(-1).to(torch.int32)
        idx = np.asarray(image.cpu() if isinstance(image, torch.Tensor) else image, np.int64).reshape(-1)
        if idx.size == 1 and n_blocks != 1:
            idx = np.repeat(idx, n_blocks)
        if idx.size != n_blocks:
            raise ValueError("Task1Evaluator: one image index per block expected")
        if idx.size and (idx.min() < 0 or idx.max() >= self.max_images):
            raise ValueError(f"Task1Evaluator: image index outside [0, {self.max_images})")
        return idx.astype(np.int32)

    def _tables(self):
        if self._t is None:
            dev, D, G = self.device, self.max_dets, self.max_gts
            with torch.cuda.device(dev):
                nbytes = _lib.lib().s2a_eval_task1_workspace_bytes(D, G, self.num_classes, self.max_images)
            self._t = dict(dp=torch.zeros((D, 8), dtype=torch.float64, device=dev), ds=torch.zeros(D, dtype=torch.float64, device=dev),
                           dl=torch.full((D,), -1, dtype=torch.int32, device=dev), di=torch.full((D,), -1, dtype=torch.int32, device=dev),
                           gp=torch.zeros((G, 8), dtype=torch.float64, device=dev), gl=torch.full((G,), -1, dtype=torch.int32, device=dev),
                           gi=torch.full((G,), -1, dtype=torch.int32, device=dev), gd=torch.zeros(G, dtype=torch.uint8, device=dev),
                           ws=torch.empty(int(nbytes), dtype=torch.uint8, device=dev))
        return self._t

    def _dev(self, x, dtype):
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype)
        return torch.from_numpy(np.ascontiguousarray(x)).to(device=self.device, dtype=dtype)

    @staticmethod
    def _polys64(boxes):
        """[n,8] polygons as they are, [n,5+] rotated boxes through rbox_to_poly (float32) widened to float64"""
        from .formats import rbox_to_poly
        if boxes.shape[1] == 8:
            return boxes.to(torch.float64)
        return rbox_to_poly(boxes.to(torch.float32).contiguous()).to(torch.float64)

    # ---- filling the tables
    def add_ground_truth(self, polys_or_rboxes, labels, image, difficult=None):
        """ground truth of one image (``image``: an int) or of several (``image``: one index per row): polygons [n,8] or
        rotated boxes [n,5] (x, y, w, h, theta), labels [n], difficult [n] (None: all 0)"""
        shape = tuple(polys_or_rboxes.shape)
        n = int(np.prod(tuple(labels.shape)))
        if len(shape) != 2 or shape[1] not in (5, 8) or shape[0] != n:
            raise ValueError("add_ground_truth: polygons [n,8] or rotated boxes [n,5] and labels [n] expected")
        if difficult is not None and int(np.prod(tuple(difficult.shape))) != n:
            raise ValueError("add_ground_truth: difficult [n] expected")
        per_row = not isinstance(image, (int, np.integer))
        img = self._image_column(image, n) if per_row else self._image_column([image], 1)
        self._check_fits("gts", n)                                  # (refused before the device is touched)
        if isinstance(polys_or_rboxes, torch.Tensor):
            _lib.require_cuda(polys_or_rboxes)
        t = self._tables()
        boxes = self._dev(polys_or_rboxes, torch.float32 if shape[1] == 5 else torch.float64)
        at = self._reserve("gts", n)
        if n == 0:
            return at
        t["gp"][at:at + n] = self._polys64(boxes)
        t["gl"][at:at + n] = self._dev(labels, torch.int32).reshape(-1)
        t["gi"][at:at + n] = self._dev(img, torch.int32) if per_row else self._dev(img, torch.int32).expand(n)
        t["gd"][at:at + n] = 0 if difficult is None else self._dev(difficult, torch.uint8).reshape(-1)
        return at

    def add_detections(self, dets, labels, counts, image_index):
        """exactly what ``S2ANet.detect`` returns for B chips: dets [B,K,6] f32 (x, y, w, h, theta, score), labels [B,K]
        (-1 padded), counts [B]; image_index [B]: the image of every chip.  Polygons through ``rbox_to_poly`` widened to
        float64 (as s2a_scene_merge takes them); rows at or behind a chip's count become padding.  All B*K rows are
        appended; returns their offset."""
        if dets.dim() != 3 or dets.shape[2] != 6 or tuple(labels.shape) != tuple(dets.shape[:2]) or counts.numel() != dets.shape[0]:
            raise ValueError("add_detections: dets [B,K,6], labels [B,K], counts [B] expected")
        B, K = int(dets.shape[0]), int(dets.shape[1])
        img = self._image_column(image_index, B)
        self._check_fits("dets", B * K)
        _lib.require_cuda(dets, labels, counts)
        t = self._tables()
        at = self._reserve("dets", B * K)
        if B * K == 0:
            return at
        d = dets.to(device=self.device, dtype=torch.float32).contiguous()
        live = torch.arange(K, device=self.device)[None, :] < counts.to(self.device).reshape(B, 1)
        lab = torch.where(live, labels.to(self.device, torch.int32), torch.full_like(labels, -1, dtype=torch.int32))
        n = B * K
        t["dp"][at:at + n] = self._polys64(d.reshape(n, 6))
        t["ds"][at:at + n] = d[..., 5].reshape(n).to(torch.float64)
        t["dl"][at:at + n] = lab.reshape(n)
        t["di"][at:at + n] = self._dev(img, torch.int32).reshape(B, 1).expand(B, K).reshape(n)
        return at

    def add_polygons(self, polys, scores, labels, image):
        """detections that are polygons already: polys [n,8], scores [n], labels [n] (outside [0, num_classes): padding);
        ``image``: an int for all rows, or one index per row"""
        n = int(scores.shape[0])
        if tuple(polys.shape) != (n, 8) or tuple(labels.shape) != (n,):
            raise ValueError("add_polygons: polys [n,8], scores [n], labels [n] expected")
        per_row = not isinstance(image, (int, np.integer))
        img = self._image_column(image, n) if per_row else self._image_column([image], 1)
        self._check_fits("dets", n)
        _lib.require_cuda(polys, scores, labels)
        t = self._tables()
        at = self._reserve("dets", n)
        if n == 0:
            return at
        t["dp"][at:at + n] = polys.to(self.device, torch.float64)
        t["ds"][at:at + n] = scores.to(self.device, torch.float64)
        t["dl"][at:at + n] = labels.to(self.device, torch.int32)
        t["di"][at:at + n] = self._dev(img, torch.int32) if per_row else self._dev(img, torch.int32).expand(n)
        return at

    def add_merged(self, scene_detections, image_index):
        """the merged detections of one scene (``merge_detections`` / ``detect_scene``), trimmed or at full capacity
        (cleared rows carry label -1: padding); image_index: the scene's image"""
        sd = scene_detections
        return self.add_polygons(sd.polys, sd.scores, sd.labels, int(image_index))

    def reset(self):
        """forget every row (the tables stay where they are: a captured ``compute`` keeps working)"""
        self.num_dets = self.num_gts = 0
        if self._t is not None:
            self._t["dl"].fill_(-1)
            self._t["gl"].fill_(-1)

    def compute(self, ovthresh=0.5, is_filter_difficult=True, use_07_metric=True, curves=False):
        """score what the tables hold -> ``Task1Result``.  No host synchronisation."""
        t = self._tables()
        return _launch_task1(t["dp"], t["ds"], t["dl"], t["di"], t["gp"], t["gl"], t["gi"], t["gd"], self.num_classes,
                             self.max_images, ovthresh, is_filter_difficult, use_07_metric, curves, ws=t["ws"])
