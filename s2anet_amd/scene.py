"""Whole-scene detection: tile grid, chip gather and per-class polygon merge on the device.

The reference cuts a scene into chips offline (DOTA_devkit/SplitOnlyImage_multi_process.py:51-85), writes every
detection as a text line (val.py:40-52) and merges the lines per class (DOTA_devkit/ResultMerge_multi_process.py:
159-245, ``py_cpu_nms_poly_fast`` :62-123).  Here the scene stays on the device: ``tile_grid`` gives the chip
origins of ``SplitSingle``, ``gather_chips`` copies all chips of a batch in one launch, ``S2ANet.detect`` runs them,
``merge_detections`` moves the padded per-chip output into scene coordinates and runs the per-class polygon NMS
as one greedy resolve -- no host synchronisation unless ``check=True`` asks for the one read-back of the status.
"""
import numpy as np
import torch

from . import _lib


def _axis_origins(extent, subsize, slide):
    """one axis of SplitSingle's loops (:68-85): step by ``slide``; the tile that reaches the end is pulled back to
    max(extent - subsize, 0) and is the last one"""
    out, pos = [], 0
    while pos < extent:
        if pos + subsize >= extent:
            pos = max(extent - subsize, 0)
        out.append(pos)
        if pos + subsize >= extent:
            break
        pos += slide
    return out


def tile_grid(height, width, subsize=1024, gap=200):
    """chip origins of ``splitbase.SplitSingle`` for a height x width scene -> int32 [N,2] rows (left, up);
    ``left`` is the outer loop, ``up`` the inner one.  A scene smaller than a chip gives one tile at 0."""
    height, width, subsize, gap = int(height), int(width), int(subsize), int(gap)
    if subsize <= 0 or not 0 <= gap < subsize:
        raise ValueError("tile_grid: need subsize > 0 and 0 <= gap < subsize")
    if height <= 0 or width <= 0:
        return np.zeros((0, 2), np.int32)
    ups = _axis_origins(height, subsize, subsize - gap)
    return np.asarray([(left, up) for left in _axis_origins(width, subsize, subsize - gap) for up in ups],
                      np.int32).reshape(-1, 2)


def chip_names(image_name, origins, rate=1):
    """chip names of SplitSingle (:60, :76): '<image>__<rate>__<left>___<up>' with str(rate) as the script formats it
    (1 -> '1', 0.5 -> '0.5'); ``merge.parse_chip_name`` inverts them"""
    return ["%s__%s__%d___%d" % (image_name, str(rate), int(left), int(up)) for left, up in np.asarray(origins).reshape(-1, 2)]


def _origins_dev(origins, device):
    if isinstance(origins, torch.Tensor):
        return origins.to(device=device, dtype=torch.int32).reshape(-1, 2).contiguous()
    return torch.from_numpy(np.ascontiguousarray(origins, np.int32).reshape(-1, 2)).to(device)


def gather_chips(scene_u8, origins, subsize=1024, out=None):
    """scene uint8 [H,W,3] (HWC) on the GPU + origins [n,2] (left, up; array or device tensor, any order) ->
    uint8 [n,3,subsize,subsize] channels-last (the storage ``S2ANet.detect`` wants; a view of [n,S,S,3]).
    Pixels outside the scene are 0.  One launch (s2a_scene_gather_u8).  ``out``: a contiguous uint8 [n,S,S,3] buffer of
    the caller to write into (every byte of it is written)."""
    _lib.require_cuda(scene_u8)
    if scene_u8.dtype != torch.uint8 or scene_u8.dim() != 3 or scene_u8.shape[2] != 3:
        raise ValueError("gather_chips: scene must be uint8 [H,W,3]")
    dev = scene_u8.device
    scene = scene_u8.contiguous()
    if scene.data_ptr() % 4:                                   # a row-offset view: the kernel reads aligned dwords
        scene = scene.clone()
    org = _origins_dev(origins, dev)
    n, S = org.shape[0], int(subsize)
    if out is None:
        chips = torch.empty((n, S, S, 3), dtype=torch.uint8, device=dev)
    else:
        if out.dtype != torch.uint8 or tuple(out.shape) != (n, S, S, 3) or not out.is_contiguous() or out.device != dev:
            raise ValueError("gather_chips: out must be a contiguous uint8 [n,subsize,subsize,3] tensor on the scene's device")
        chips = out
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().s2a_scene_gather_u8(_lib.ptr(scene), scene.shape[0], scene.shape[1], _lib.ptr(org), n, S,
                                                  _lib.ptr(chips), _lib.stream_ptr(dev)))
    return chips.permute(0, 3, 1, 2)


class SceneDetections:
    """merged detections of one scene, on the device: ``polys`` f64 [M,8], ``scores`` f64 [M], ``labels`` int64 [M],
    ``src`` int64 [M] (source row chip*K + k) -- class-major, descending score inside a class; ``class_counts`` int64
    [num_classes]; ``status`` int64 [4] (see s2a_scene_merge).  With ``check=False`` nobody has read the status: the
    four row tensors then have the full capacity n_chips*K (rows behind ``class_counts.sum()`` are cleared) and are
    only valid if ``status[0] == 0``."""
    __slots__ = ("polys", "scores", "labels", "src", "class_counts", "status", "chips", "per_chip")

    def __init__(self, polys, scores, labels, src, class_counts, status):
        self.polys, self.scores, self.labels, self.src = polys, scores, labels, src
        self.class_counts, self.status = class_counts, status
        self.chips = self.per_chip = None


def _merge_once(dets, labels, counts, org, rates, num_classes, thresh, cap):
    dev = dets.device
    n_chips, K = dets.shape[0], dets.shape[1]
    n = n_chips * K
    polys = torch.empty((n, 8), dtype=torch.float64, device=dev)
    scores = torch.empty((n,), dtype=torch.float64, device=dev)
    lab = torch.empty((n,), dtype=torch.int64, device=dev)
    src = torch.empty((n,), dtype=torch.int64, device=dev)
    class_counts = torch.empty((num_classes,), dtype=torch.int64, device=dev)
    status = torch.empty((4,), dtype=torch.int64, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        ws = _lib.workspace(L.s2a_scene_merge_workspace_bytes(n, cap), dev, "scene_merge")
        _lib.check(L.s2a_scene_merge(_lib.ptr(dets), _lib.ptr(labels), _lib.ptr(counts), _lib.ptr(org), _lib.ptr(rates),
                                     n_chips, K, num_classes, float(thresh), cap, _lib.ptr(polys), _lib.ptr(scores),
                                     _lib.ptr(lab), _lib.ptr(src), _lib.ptr(class_counts), _lib.ptr(status),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return SceneDetections(polys, scores, lab, src, class_counts, status)


def merge_workspace_bytes(n_rows, pair_capacity=None):
    """bytes of scratch ``merge_detections`` takes for n_rows = n_chips*K input rows (default capacity: None)"""
    return int(_lib.lib().s2a_scene_merge_workspace_bytes(int(n_rows), int(pair_capacity or 0)))


def merge_detections(dets, labels, counts, origins, rates=None, num_classes=15, thresh=0.5, pair_capacity=None,
                     check=True):
    """per-class polygon merge of the chips of one scene (s2a_scene_merge).

    dets [n_chips,K,6] f32 (x, y, w, h, theta, score), labels [n_chips,K] (-1 padded), counts [n_chips]: what
    ``S2ANet.detect`` returns for the chips; origins [n_chips,2] (left, up); rates: one float per chip (the
    ``/ rate`` of poly2origpoly), None = 1.0.  Returns a ``SceneDetections``.

    The candidate pair list has ``pair_capacity`` entries (None: derived from the row count).  ``check=True`` reads
    the status back once at the end, runs again with the reported pair count if the list overflowed, and trims the
    result to its kept rows.  ``check=False`` issues no host synchronisation at all (the call can be captured into a
    HIP graph); the caller has to look at ``status[0]`` before using the result."""
    _lib.require_cuda(dets, labels, counts)
    if dets.dim() != 3 or dets.shape[2] != 6 or tuple(labels.shape) != tuple(dets.shape[:2]) or counts.numel() != dets.shape[0]:
        raise ValueError("merge_detections: dets [n,K,6], labels [n,K], counts [n] expected")
    dev = dets.device
    n_chips = dets.shape[0]
    d = dets.to(torch.float32).contiguous()
    lb = labels.to(torch.int32).contiguous()
    ct = counts.to(torch.int32).contiguous()
    org = _origins_dev(origins, dev)
    if org.shape[0] != n_chips:
        raise ValueError("merge_detections: one origin per chip expected")
    rt = None
    if rates is not None:
        rt = (rates.to(device=dev, dtype=torch.float64) if isinstance(rates, torch.Tensor)
              else torch.from_numpy(np.ascontiguousarray(rates, np.float64)).to(dev)).reshape(-1).contiguous()
        if rt.numel() != n_chips:
            raise ValueError("merge_detections: one rate per chip expected")
    cap = int(pair_capacity or 0)
    res = _merge_once(d, lb, ct, org, rt, int(num_classes), thresh, cap)
    if not check:
        return res
    st = res.status.tolist()                                   # the one read-back
    if st[0] != 0:
        res = _merge_once(d, lb, ct, org, rt, int(num_classes), thresh, max(int(st[1]), 1))
        st = res.status.tolist()
        if st[0] != 0:
            raise RuntimeError(f"merge_detections: pair list overflowed again ({st[1]} pairs)")
    m = int(res.class_counts.sum())
    res.polys, res.scores, res.labels, res.src = res.polys[:m], res.scores[:m], res.labels[:m], res.src[:m]
    return res


@torch.no_grad()
def detect_scene(model, scene_u8, batch=8, subsize=1024, gap=200, rate=1.0, thresh=0.5, return_chips=False, check=True,
                 **detect_kw):
    """``S2ANet.detect_scene``: tile, gather, detect in fixed batches, merge.

    scene_u8: uint8 [H,W,3] on the GPU, or a list of (scene, rate) pairs (the caller resized them) that are merged
    together as the reference merges every rate of an image in one file.  Chips run through ``detect()`` in batches
    of exactly ``batch`` (one set of shapes, workspaces and packed layouts); the last batch is padded with all-zero
    chips whose counts are forced to 0 before the merge.  ``return_chips=True``: the result also carries ``chips``
    (uint8 [n,3,S,S], the padding included) and ``per_chip`` = (dets, labels, counts, origins, rates) as merged."""
    scenes = [(scene_u8, rate)] if isinstance(scene_u8, torch.Tensor) else [(s, r) for s, r in scene_u8]
    if not scenes:
        raise ValueError("detect_scene: no scene")
    batch = int(batch)
    if batch < 1:
        raise ValueError("detect_scene: batch must be >= 1")
    dev = scenes[0][0].device
    all_chips, all_org, all_rate, all_real = [], [], [], []
    outs = []
    for sc, r in scenes:
        _lib.require_cuda(sc)
        org = tile_grid(sc.shape[0], sc.shape[1], subsize, gap)
        n = org.shape[0]
        pad = (-n) % batch
        # padded chips: an origin beyond the scene gathers zeros
        org_p = np.concatenate([org, np.tile(np.asarray([[sc.shape[1], sc.shape[0]]], np.int32), (pad, 1))]) if pad else org
        org_dev = _origins_dev(org_p, dev)
        for b0 in range(0, n + pad, batch):
            chips = gather_chips(sc, org_dev[b0:b0 + batch], subsize)
            outs.append(model.detect(chips, **detect_kw)[:3])
            if return_chips:
                all_chips.append(chips)
        if pad:
            org_p = org_p.copy()
            org_p[n:] = 0
        all_org.append(org_p)
        all_rate.append(np.full(n + pad, float(r), np.float64))
        all_real.append(np.arange(n + pad) < n)
    dets = torch.cat([o[0] for o in outs])
    labels = torch.cat([o[1] for o in outs])
    counts = torch.cat([o[2] for o in outs])
    real = torch.from_numpy(np.concatenate(all_real)).to(dev)
    counts = torch.where(real, counts, torch.zeros_like(counts))
    origins = np.concatenate(all_org)
    rates = np.concatenate(all_rate)
    res = merge_detections(dets, labels, counts, origins, rates, num_classes=model.head.num_classes, thresh=thresh, check=check)
    if return_chips:
        res.chips = torch.cat(all_chips)
        res.per_chip = (dets, labels, counts, origins, rates)
    return res
