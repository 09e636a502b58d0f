"""GPU: the workspace contract of the C ABI (include/s2anet_hip.h, "Workspaces"), entry point by entry point, on guarded
buffers (tests/workspace_guard.py).  For every entry point that takes (workspace, workspace_bytes), at the smallest shapes at
which the carving can go wrong:

  a. exactly *_workspace_bytes() bytes of NON-ZERO scratch (0xA5, then 0xFF) give the result of the op's own oracle at the
     tolerance of the op's existing test; where the op is bit-reproducible the two fills also equal each other and a run on a
     generous zero-filled workspace (4 x the bytes + 1 MiB) bit for bit;
  b. nothing in front of or behind the declared bytes is written (canaries);
  c. the 64 guard elements behind every output keep their bits, and outputs the header calls fully written hold no fill;
  d. one byte less, and a NULL workspace, return exactly S2A_EWORKSPACE with the entry point named in s2a_last_error(),
     and neither the outputs nor the workspace change: no kernel was launched.

Nothing but the scratch contents (and, in d, the declared size) is abnormal: all inputs are finite and valid.

AUDIT below is the reading of every host function: the sub-buffers it carves, what writes each one FIRST within the same
call, and which results are bit-reproducible between two calls.  tests/test_workspace_queries_cpu.py holds its keys against
the *_workspace_bytes symbols the built library exports, so an entry point added without a row fails the suite.

s2a_nms_rotated / s2a_ml_nms_rotated carve their lists for one segment of n rows: their declaration is (n, n).  The segmented
NMS entry points are not told which max_segment_rows the caller sized for, so the bound they can enforce is the smallest
declaration, s2a_nms_rotated_workspace_bytes(n, 1): they run at (n, n) and (n, 1), and (d) at (n, 1) -- at (n, n) one byte
less is still a valid (n, m < n) declaration and is accepted by design (header: a list that fills up finishes on the direct
kernel).
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import oracle
from conftest import distinct_scores, golden, rand_rboxes
from workspace_guard import GuardedWorkspaces

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ------------------------------------------------------------------------------------------------ the audit
# query -> ops: the entry points it sizes; buffers: (sub-buffer, first writer within the call); reproducible: True (every
# result), or the names of the results that are (the others are summed with float atomics, DESIGN.md / the ops' own tests)
AUDIT = {
    "s2a_box_iou_rotated_workspace_bytes": dict(
        ops=("s2a_box_iou_rotated",), reproducible=True,
        buffers=(("P1 PreBox[n], P2 PreBox[m]", "k_prep_boxes2"),
                 ("counters u64[512]", "k_prep_boxes2 zeroes all 512"),
                 ("gq uint2[cap] (the rest of the workspace)", "k_iou_cull*: entries below the chunk's counter only"),
                 ("vals f32[cap]", "k_iou_heavy: one per listed pair"))),
    "s2a_assign_labels_workspace_bytes": dict(
        ops=("s2a_assign_labels",), reproducible=True,
        buffers=(("list form: gt_pre[N], gt_key[N], gt_arg[N], rowbest[M], nbad[M], r3[M], count", "k_assign_list_init"),
                 ("list form: pair uint2[M*N], val f32[M*N]", "k_assign_cull / k_assign_exact below *count"),
                 ("matrix form: ious f32[M*N]", "s2a_box_iou_rotated (k_iou_cull<true> zero-fills, k_iou_scatter)"),
                 ("matrix form: gt_key[N], gt_arg[N]", "fill_u32"),
                 ("matrix form: the IoU's own workspace", "see s2a_box_iou_rotated_workspace_bytes"))),
    "s2a_assign_labels_batched_workspace_bytes": dict(
        ops=("s2a_assign_labels_batched",), reproducible=True,
        buffers=(("sets[4], img_count[B], gt_key / gt_arg [S*G], rowbest / nbad / r3 [S*B*A], count", "k_ab_init"),
                 ("img[G]", "k_ab_prep_count"), ("gt_img[G], gt_pre[G]", "k_ab_prep_scatter"),
                 ("pair uint2[P], val f32[P]", "k_ab_cull / k_ab_exact below min(*count, P)"))),
    "s2a_nms_poly_workspace_bytes": dict(
        ops=("s2a_nms_poly",), reproducible=True,
        buffers=(("key_a[n], idx_a[n]", "k_poly_keys"), ("key_b[n], order[n], sort scratch", "rocprim::radix_sort_pairs"),
                 ("sorted PolyBox[n], small[0..12)", "k_poly_prep (small[64] u64 is cleared by hipMemsetAsync first)"),
                 ("keep_orig[n], small[64]: pair / edge counters, status", "hipMemsetAsync"),
                 ("mask u64[n * nb] (mask form only)", "hipMemsetAsync (thresh >= 0) / k_poly_mask: every word the scan reads"),
                 ("pairs / edges / alive uint2[cap]", "k_poly_cull / k_poly_edges / k_nms_round below their counters"),
                 ("edge rounds: EdgeRoundsWs, state[n], blocked[2n]", "k_edge_rounds_init"),
                 ("cnt_scratch u32[blocks]", "k_nms_keep_count"), ("flags[n] (mask form)", "k_poly_flags"))),
    "s2a_nms_rotated_workspace_bytes": dict(
        ops=("s2a_nms_rotated", "s2a_ml_nms_rotated", "s2a_nms_rotated_segmented", "s2a_nms_rotated_segmented_dets"),
        reproducible=True,
        buffers=(("small path (k_nms_small): u64[n] + 1 KiB at the start of the workspace", "k_nms_small itself"),
                 ("keyA[n], keyC[n], idx[n], bbox_part, C (all counters), blocked[2n+4], seg_cnt[n+2], lo / hi, htab, hist, spb_ctr",
                  "k_nms_prep (by kernel, never a memset node)"),
                 ("keyA_s, perm_seg, rp_temp[0]", "rocprim::radix_sort_pairs / k_seg_sort"),
                 ("cnt, segidx1, seg_start, num_seg, sorted, state, state_fb (seg_start_a, num_seg_a)", "k_nms_seg_count / k_nms_pos_meta / k_seg_sort"),
                 ("keyB, keyB_s, perm_sp, rank, bucket, cnt2, lasthead, sp_box, rankkey (spatial order only)", "k_nms_spkeys / k_spb_* / k_nms_sp_meta"),
                 ("keyC_s, perm_glob, rp_temp[2]", "rocprim::radix_sort_pairs (output order)"),
                 ("tiles / gq / edges (the three lists)", "k_nms_tile_filter / k_nms_cull / k_nms_heavy below their counters in C"),
                 ("keep_orig[n]", "k_nms_finish"), ("cnt3", "k_nms_keep_count"), ("seg_cur", "k_nms_finish_segments"))),
    "s2a_nms_rotated_f64_workspace_bytes": dict(
        ops=("s2a_nms_rotated_f64",), reproducible=True,
        buffers=(("key_a[n], idx_a[n]", "k_rot64_keys"), ("key_b[n], order[n], sort scratch", "rocprim::radix_sort_pairs"),
                 ("small[64] u64, keep_orig[n]", "hipMemsetAsync"), ("sorted RBox6[n], small[0..12)", "k_rot64_prep"),
                 ("mask u64[n * nb]", "k_rot64_mask: the words of column blocks >= the row's block, the only ones k_nms_scan reads"),
                 ("flags[n]", "k_poly_flags"))),
    "s2a_multiclass_candidates_workspace_bytes": dict(
        ops=("s2a_multiclass_candidates",), reproducible=True,
        buffers=(("blk u32[blocks + 1]", "k_cand_count"), ("sel i32[total]", "k_cand_scatter: the first *count entries, all that are read"))),
    "s2a_deform_conv_workspace_bytes": dict(
        ops=("s2a_deform_conv_forward",), reproducible=True,
        buffers=(("wp: packed filter, two layouts (fast path)", "k_pack_weight + k_pack_weight_frag16 / k_pack_weight_x3"),
                 ("xn: NHWC copy of an NCHW input (fast path)", "k_nchw_to_nhwc"), ("generic path", "uses no scratch"))),
    "s2a_align_conv_workspace_bytes": dict(
        ops=("s2a_align_conv_forward",), reproducible=True,
        buffers=(("wp: packed filter (unless weight_packed)", "k_pack_weight + k_pack_weight_frag16 / k_pack_weight_x3"),
                 ("xn: NHWC copy of an NCHW input", "k_nchw_to_nhwc"))),
    "s2a_scene_merge_workspace_bytes": dict(
        ops=("s2a_scene_merge",), reproducible=True,
        buffers=(("key_a[n], idx_a[n], ctl (pair / edge counters)", "k_scene_keys"),
                 ("key_s[n], order[n], sort scratch", "rocprim::radix_sort_pairs"), ("polys32 f32[n*8]", "s2a_rbox_to_poly"),
                 ("sorted PolyBox[n], seg_start[classes + 2]", "k_scene_prep"),
                 ("pairs / edges / alive uint2[cap]", "k_scene_cull / k_poly_edges / k_nms_round below their counters"),
                 ("edge rounds: EdgeRoundsWs, state[n], blocked[2n]", "k_edge_rounds_init"),
                 ("keep_orig[n]", "k_nms_finish"), ("cnt u32[blocks]", "k_scene_count"))),
    "s2a_eval_task1_workspace_bytes": dict(
        ops=("s2a_eval_task1",), reproducible=True,
        buffers=(("key_a, idx_a [D]", "k_eval_det_keys"), ("key_s, ord1, ckey_s, order, gkey_s, grp_rank, gtkey_s, gt_order, sort scratch", "rocprim::radix_sort_pairs"),
                 ("ckey_a[D]", "k_eval_class_keys"), ("gkey_a, rank_a [D]", "k_eval_group_keys"), ("gtkey_a, gtidx_a [G]", "k_eval_gt_keys"),
                 ("gt_off[groups + 1], seg_start[classes + 1], claim[G]", "k_eval_tables"),
                 ("ov_ws[D], slot_ws[D] (= idx_a, dead after the first sort)", "k_eval_match"),
                 ("flag[D], tile_tot[tiles]", "k_eval_mark"), ("cum uint2[D]", "k_eval_cum"), ("acc ClassAcc[classes]", "k_eval_class"))),
    "s2a_conv_backward_prep_f16_workspace_bytes": dict(
        ops=("s2a_conv_backward_prep_f16",), reproducible=True,
        buffers=(("partial f32[blocks][O]", "k_conv_bwd_prep: every workgroup its whole row"),)),
    "s2a_conv_backward_weight_f16_workspace_bytes": dict(
        ops=("s2a_conv_backward_weight_f16",), reproducible=True,
        buffers=(("partial f32[slice][owner][ostride][k][64]", "k_conv_bwd_weight: every workgroup the rows of its out channels "
                  "(a slice without a tile writes zeros); k_conv_bwd_weight_reduce reads those rows only"),)),
    "s2a_deform_conv_backward_input_workspace_bytes": dict(
        ops=("s2a_deform_conv_backward_input_f16",), reproducible=("grad_offset",),
        buffers=(("xn, gn: NHWC copies", "k_bwd_nchw_to_nhwc(_h8)"), ("wp: packed filter", "k_pack_weight_bwd"),
                 ("gacc f32[S,H,W,C]", "k_bwd_zero4, then the tiles' float atomics"))),
    "s2a_deform_conv_backward_input_f32_workspace_bytes": dict(
        ops=("s2a_deform_conv_backward_input_f32",), reproducible=("grad_offset",),
        buffers=(("xn, gn: NHWC copies", "k_bwd_nchw_to_nhwc"), ("wp: packed filter", "k_pack_weight_bwd_f32"))),
    "s2a_deform_conv_backward_weight_workspace_bytes": dict(
        ops=("s2a_deform_conv_backward_weight_f16",), reproducible=True,
        buffers=(("xn, gn: NHWC copies", "k_bwd_nchw_to_nhwc(_h8)"),
                 ("partial f32[320][O][192]", "k_dcn_bwd_weight: blocks [0, owners * ksplit), all k_dcn_bwd_weight_reduce reads"))),
    "s2a_deform_conv_backward_weight_f32_workspace_bytes": dict(
        ops=("s2a_deform_conv_backward_weight_f32",), reproducible=True,
        buffers=(("xn, gn: NHWC copies", "k_bwd_nchw_to_nhwc"),
                 ("partial f32[320][O][192]", "k_dcn_bwd_weight_x3: blocks [0, owners * ksplit)"))),
    "s2a_deform_conv_backward_workspace_bytes": dict(
        ops=("s2a_deform_conv_backward", "s2a_deform_conv_backward_typed"), reproducible=("grad_offset", "grad_weight"),
        buffers=(("xn, gn, wp, gacc (f16), partial", "as the four queries above, in that order"),)),
    "s2a_s2anet_loss_workspace_bytes": dict(
        ops=("s2a_s2anet_loss_forward",), reproducible=True,          # (s2a_s2anet_loss_backward takes no workspace)
        buffers=(("partial f64[2 * B * blocks][3]", "k_loss_main: every workgroup its triple"),)),
    "s2a_train_update_workspace_bytes": dict(
        ops=("s2a_train_update",), reproducible=True,
        buffers=(("ctrl (inv_scale, clip, d, 1 - d, skip, pad)", "k_optim_finalise: every field"),
                 ("partial f32[chunks], flags u32[chunks]", "k_optim_partials: every trained chunk (not launched, and not read, "
                  "without clipping and scaling)"))),
}

ENTRY_QUERY = {op: q for q, row in AUDIT.items() for op in row["ops"]}


# ------------------------------------------------------------------------------------------------ guarded outputs
GUARD = 64
PATTERN = {torch.float32: 12345.0, torch.float16: 12344.0, torch.float64: 12345.678, torch.int64: 0x5a5a5a5a,
           torch.int32: 0x5a5a5a5a, torch.uint8: 0x5a}


def cu(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).to(DEV)          # (a copy: the shared inputs are read-only arrays)
    return t if dtype is None else t.to(dtype)


class Out:
    """an output of `shape` with GUARD elements behind it, everything pre-filled with PATTERN[dtype].  init: the caller's
    initial value of an ACCUMULATED output (then, as for partly written outputs, written=False: no no-fill check)"""

    def __init__(self, shape, dtype, written=True, init=None):
        self.shape, self.n, self.written, self.pat = tuple(shape), int(np.prod(shape)), written, PATTERN[dtype]
        self.buf = torch.full((self.n + GUARD,), self.pat, dtype=dtype, device=DEV)
        if init is not None:
            self.buf[:self.n] = init.reshape(-1).to(dtype)
        self.before = self.buf.clone()

    def data_ptr(self):
        return self.buf.data_ptr()

    def value(self):
        return self.buf[:self.n].view(self.shape)

    def numpy(self):
        return self.value().cpu().numpy()

    def guard_ok(self):
        return torch.equal(self.buf[self.n:], self.before[self.n:])

    def untouched(self):
        return torch.equal(self.buf, self.before)

    def holds_fill(self):
        return bool((self.buf[:self.n] == self.pat).any())


class NullWorkspace:
    """workspace = NULL with a plausible size"""

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def data_ptr(self):
        return 0

    def numel(self):
        return self.nbytes


class Case:
    """one entry point at one shape.  outputs() -> {name: Out}; call(outs, ws) -> rc (ws: data_ptr() / numel());
    results(outs) -> {name: ndarray} what the op's contract defines; verify(res): the oracle comparison"""

    def __init__(self, entry, tag, need, outputs, call, results, verify, short=True, env=None):
        self.entry, self.tag, self.need, self.short, self.env = entry, tag, int(need), short, env or {}
        self.outputs, self.call, self.results, self.verify = outputs, call, results, verify
        self.query = ENTRY_QUERY[entry]


def lib():
    from s2anet_amd import _lib
    return _lib, _lib.lib()


def stream():
    from s2anet_amd import _lib
    return _lib.stream_ptr(torch.device(DEV))


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def last_error():
    return lib()[1].s2a_last_error().decode("utf-8", "replace")


def generous(nbytes):
    return 3 * nbytes + (1 << 20)                     # handed out: 4 x the declaration + 1 MiB


def run_contract(case, monkeypatch):
    _lib, L = lib()
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    assert case.need > 0, "the query refuses a valid problem"
    reproducible = AUDIT[case.query]["reproducible"]
    runs = []
    # (a) - (c): 0x00 generous, then 0xA5 and 0xFF at exactly the declared size; a case stops at the first failing fill
    for fill, slack in ((0x00, generous), (0xA5, None), (0xFF, None)):
        what = "%s %s fill %#04x" % (case.entry, case.tag, fill)
        gw = GuardedWorkspaces(fill, slack)
        ws = gw(case.need, torch.device(DEV), case.entry)
        assert slack is not None or ws.numel() == case.need
        outs = case.outputs()
        rc = case.call(outs, ws)
        torch.cuda.synchronize()
        assert rc == _lib.OK, (what, rc, last_error())
        gw.check()                                                                   # (b)
        for name, o in outs.items():                                                 # (c)
            if isinstance(o, Out):
                assert o.guard_ok(), (what, name, "wrote behind the output")
                assert not (o.written and o.holds_fill()), (what, name, "a fully written output still holds its fill pattern")
        res = case.results(outs)
        case.verify(res)                                                             # (a): the oracle
        runs.append(res)
    names = list(runs[0]) if reproducible is True else [n for n in runs[0] if n in (reproducible or ())]
    assert reproducible is False or names, "nothing to compare"
    for name in names:                                                               # (a): invariance
        for other, fill in ((runs[1], 0xA5), (runs[2], 0xFF)):
            a, b = np.ascontiguousarray(runs[0][name]), np.ascontiguousarray(other[name])
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
                "%s %s: %s depends on the scratch contents (fill %#04x against a zeroed workspace)" % (case.entry, case.tag, name, fill)
    if not case.short:
        return
    # (d): one byte short on the same kind of guarded buffer, then NULL: S2A_EWORKSPACE, nothing launched
    gw = GuardedWorkspaces(0xA5)
    ws = gw(case.need, torch.device(DEV), case.entry)
    for what, w in (("one byte short", ws[:case.need - 1]), ("NULL workspace", NullWorkspace(case.need))):
        outs = case.outputs()
        rc = case.call(outs, w)
        torch.cuda.synchronize()
        msg = last_error()
        assert rc == _lib.EWORKSPACE, (case.entry, case.tag, what, rc, msg)
        assert case.entry[len("s2a_"):] in msg and "workspace" in msg, (case.entry, what, msg)
        for name, o in outs.items():
            if isinstance(o, Out):
                assert o.untouched(), (case.entry, case.tag, what, name, "a refused call wrote an output")
        assert gw.untouched(), (case.entry, case.tag, what, "a refused call wrote the workspace")
    gw.check()


CASES = []


def case_id(c):
    return "%s-%s" % (c.entry[len("s2a_"):], c.tag)


def register(fn):
    """a builder yields Case factories lazily: inputs and oracles are made when the test runs, not at collection"""
    for entry, tag, make in fn():
        CASES.append(pytest.param(make, id="%s-%s" % (entry[len("s2a_"):], tag)))
    return fn


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ rotated IoU
@register
def iou_cases():
    for n, m in ((1, 1), (3, 257)):
        def make(n=n, m=m):
            _lib, L = lib()
            rng = np.random.default_rng(100 + n)
            b1, b2 = rand_rboxes(rng, n, span=120), rand_rboxes(rng, m, span=120)
            if n == 1:
                b2[0, :2] = b1[0, :2] + 3.0                                          # the one pair overlaps
            ref = oracle.box_iou_rotated(b1, b2, sort_mode=oracle.SORT_GPU, cull=True)
            t1, t2 = cu(b1), cu(b2)

            def call(outs, ws):
                return L.s2a_box_iou_rotated(vp(t1), n, vp(t2), m, vp(outs["ious"]), vp(ws), ws.numel(), stream())

            def verify(res):
                assert (bits32(res["ious"]) != bits32(ref)).sum() == 0 and (ref > 0).any()
            return Case("s2a_box_iou_rotated", "%dx%d" % (n, m), L.s2a_box_iou_rotated_workspace_bytes(n, m),
                        lambda: {"ious": Out((n, m), torch.float32)}, call, lambda o: {"ious": o["ious"].numpy()}, verify)
        yield "s2a_box_iou_rotated", "%dx%d" % (n, m), make


# ------------------------------------------------------------------------------------------------ label assignment
def _assign_inputs(A, G):
    from test_gpu_assign_batched import SIZE, pyramid
    rng = np.random.default_rng(7 * A + G)
    grid, _ = pyramid()
    a = grid[:A].copy() if A > 1 else np.array([[100.0, 90.0, 32.0, 32.0, 0.2]], np.float32)
    g = rand_rboxes(rng, G, span=SIZE, lo=8, hi=80)
    g[0] = a[0] * np.array([1, 1, 1.1, 0.9, 1], np.float32)                           # at least one positive
    if G >= 3:
        g[2] = g[1]                                                                  # two identical gts
    return a.astype(np.float32), g.astype(np.float32), (SIZE, SIZE)


@register
def assign_cases():
    for A, G in ((1, 1), (1364, 3), (1364, 129)):
        for form in ("list", "matrix"):
            def make(A=A, G=G, form=form):
                _lib, L = lib()
                a, g, size = _assign_inputs(A, G)
                ref = oracle.assign_labels(a, g, imgs_size=size)
                ta, tg = cu(a), cu(g)

                def call(outs, ws):
                    return L.s2a_assign_labels(vp(ta), A, vp(tg), G, float(size[0]), float(size[1]), 0.5, 0.4, 0.0, 1, 1, 1,
                                               vp(outs["ids"]), vp(ws), ws.numel(), stream())

                def verify(res):
                    assert np.array_equal(res["ids"], ref) and (ref >= 0).any()
                return Case("s2a_assign_labels", "%s-%dx%d" % (form, A, G), L.s2a_assign_labels_workspace_bytes(A, G),
                            lambda: {"ids": Out((A,), torch.int64)}, call, lambda o: {"ids": o["ids"].numpy()}, verify,
                            env={"S2A_ASSIGN_LIST": "1" if form == "list" else "0"})
            yield "s2a_assign_labels", "%s-%dx%d" % (form, A, G), make


@register
def assign_batched_cases():
    # (S, B, A, counts per image, pair capacity): the smallest problem; two sets, a ragged table across the LDS chunk of 128
    for S, B, A, counts, P in ((1, 1, 1, (1,), 1), (2, 2, 1364, (129, 3), 2 * 1364 * 132)):
        def make(S=S, B=B, A=A, counts=counts, P=P):
            from test_gpu_assign_batched import SIZE, make_targets, oracle_ids, pyramid, sort_reference
            _lib, L = lib()
            grid, ref = pyramid()
            if A == 1:
                sets_np = [np.array([[100.0, 90.0, 32.0, 32.0, 0.2]], np.float32)]
                t = np.array([[0, 3, 100.0, 90.0, 35.0, 30.0, 0.2]], np.float32)
            else:
                sets_np = [grid, ref[:B]]
                t = make_targets(counts, 41)
            G = t.shape[0]
            ts, off = sort_reference(t, B)
            want = oracle_ids(sets_np, ts, off, (SIZE, SIZE))
            sets = [cu(s) for s in sets_np]
            table = (_lib.AnchorSet * S)()
            for e, s in zip(table, sets):
                e.anchors, e.batch_stride = s.data_ptr(), (A * 5 if s.dim() == 3 else 0)
            tt = cu(t)

            def outputs():
                return {"ids": Out((S, B, A), torch.int64), "sorted": Out((G, 7), torch.float32), "offsets": Out((B + 1,), torch.int64),
                        "status": Out((4,), torch.int64), "_keep": (sets, table, tt)}

            def call(outs, ws):
                return L.s2a_assign_labels_batched(table, S, B, A, vp(tt), G, None, float(SIZE), float(SIZE), 0.5, 0.4, 0.0, 1, 1, 1,
                                                   vp(outs["ids"]), vp(outs["sorted"]), vp(outs["offsets"]), vp(outs["status"]), P,
                                                   vp(ws), ws.numel(), stream())

            def verify(res):
                st = res["status"]
                assert st[0] == 0 and st[2] == G and st[3] == 0 and 0 < st[1] <= P, st
                assert np.array_equal(res["sorted"].view(np.uint32), ts.view(np.uint32)) and np.array_equal(res["offsets"], off)
                assert np.array_equal(res["ids"], want) and (want >= 0).any()
            return Case("s2a_assign_labels_batched", "S%dB%dA%dG%d" % (S, B, A, G),
                        L.s2a_assign_labels_batched_workspace_bytes(S, B, A, G, P), outputs, call,
                        lambda o: {k: o[k].numpy() for k in ("ids", "sorted", "offsets", "status")}, verify)
        yield "s2a_assign_labels_batched", "S%dB%dA%d" % (S, B, A), make


# ------------------------------------------------------------------------------------------------ multiclass candidates
@register
def candidate_cases():
    for n in (1, 257):
        def make(n=n):
            _lib, L = lib()
            B, C, thr = 1, 15, 0.3
            total = cap = B * n * C
            rng = np.random.default_rng(n)
            boxes = rand_rboxes(rng, B * n, span=300)
            scores = rng.random(total).astype(np.float32)
            scores[3] = 0.9
            flat = np.nonzero(scores > np.float32(thr))[0]                           # row-major == the reference's mask order
            k = flat.size
            want = dict(boxes=np.zeros((cap, 5), np.float32), scores=np.full(cap, -1, np.float32), seg=np.full(cap, -1, np.int32),
                        grp=np.full(cap, -1, np.int32), cls=np.full(cap, -1, np.int32), count=np.array([k], np.int64))
            want["boxes"][:k], want["scores"][:k] = boxes[flat // C], scores[flat]
            want["cls"][:k], want["grp"][:k] = flat % C, flat // C // n
            want["seg"][:k] = want["grp"][:k] * C + want["cls"][:k]
            tb, tsc = cu(boxes), cu(scores)

            def outputs():
                return {"boxes": Out((cap, 5), torch.float32), "scores": Out((cap,), torch.float32), "seg": Out((cap,), torch.int32),
                        "grp": Out((cap,), torch.int32), "cls": Out((cap,), torch.int32), "count": Out((1,), torch.int64)}

            def call(outs, ws):
                return L.s2a_multiclass_candidates(vp(tb), vp(tsc), B, n, C, thr, cap, vp(outs["boxes"]), vp(outs["scores"]),
                                                   vp(outs["seg"]), vp(outs["grp"]), vp(outs["cls"]), vp(outs["count"]), vp(ws),
                                                   ws.numel(), stream())

            def verify(res):
                assert 0 < k < total
                for name, w in want.items():
                    assert np.array_equal(res[name].view(np.uint8), w.view(np.uint8)), name
            return Case("s2a_multiclass_candidates", "total%d" % total, L.s2a_multiclass_candidates_workspace_bytes(total), outputs,
                        call, lambda o: {k_: v.numpy() for k_, v in o.items()}, verify)
        yield "s2a_multiclass_candidates", "total%d" % (15 * n), make


# ------------------------------------------------------------------------------------------------ rotated NMS, drop-in forms
def _nms_inputs(n, labels, dtype=np.float32):
    rng = np.random.default_rng(1000 * labels + n)
    d = rand_rboxes(rng, n, span=max(40.0, 9.0 * math.sqrt(n)), lo=8, hi=40)          # sparse: a few overlaps per row
    s = distinct_scores(rng, n)
    lab = rng.integers(0, labels, n).astype(np.float32)
    return d.astype(dtype), s.astype(dtype), lab.astype(dtype)


def _keep_outputs(n):
    return {"keep": Out((n,), torch.int64, written=False), "count": Out((1,), torch.int64), "host": ctypes.c_int64(-1)}


def _keep_results(sync):
    def results(o):
        k = int(o["count"].numpy()[0])
        if sync:
            assert o["host"].value == k, (o["host"].value, k)
        return {"keep": o["keep"].numpy()[:k].copy(), "count": np.array([k])}
    return results


@register
def nms_dropin_cases():
    for n in (1, 65, 257):
        for labels in (1, 3):
            for msr in ("n",):                         # (the drop-in forms take (n, n): see the module docstring)
                for sync in (True, False):
                    entry = "s2a_nms_rotated" if labels == 1 else "s2a_ml_nms_rotated"
                    tag = "n%d-ws(n,%s)-%s" % (n, msr, "sync" if sync else "async")

                    def make(n=n, labels=labels, msr=msr, sync=sync, entry=entry, tag=tag):
                        _lib, L = lib()
                        d, s, lab = _nms_inputs(n, labels)
                        thr = 0.3
                        ref = oracle.nms_rotated(d, s, thr, labels=lab if labels > 1 else None)
                        td, ts, tl = cu(d), cu(s), cu(lab)

                        def call(outs, ws):
                            host = ctypes.byref(outs["host"]) if sync else None
                            if labels == 1:
                                return L.s2a_nms_rotated(vp(td), vp(ts), n, thr, vp(outs["keep"]), vp(outs["count"]), host, vp(ws),
                                                         ws.numel(), stream())
                            return L.s2a_ml_nms_rotated(vp(td), vp(ts), vp(tl), n, thr, vp(outs["keep"]), vp(outs["count"]), host,
                                                        vp(ws), ws.numel(), stream())

                        def verify(res):
                            assert np.array_equal(res["keep"], ref), (res["keep"][:8], ref[:8])
                            assert n < 65 or 0 < len(ref) < n
                        return Case(entry, tag, L.s2a_nms_rotated_workspace_bytes(n, n if msr == "n" else 1), lambda: _keep_outputs(n),
                                    call, _keep_results(sync), verify)
                    yield entry, tag, make


@register
def nms_f64_cases():
    for n in (1, 65, 257):
        for labels in (1, 3):
            tag = "n%d-labels%d" % (n, labels)

            def make(n=n, labels=labels, tag=tag):
                _lib, L = lib()
                d, s, lab = _nms_inputs(n, labels, np.float64)
                thr = 0.3
                ref = oracle.nms_rotated_f64(d, s, thr, labels=lab if labels > 1 else None)
                td, ts, tl = cu(d), cu(s), (cu(lab) if labels > 1 else None)

                def call(outs, ws):
                    return L.s2a_nms_rotated_f64(vp(td), vp(ts), vp(tl), n, thr, vp(outs["keep"]), vp(outs["count"]),
                                                 ctypes.byref(outs["host"]), vp(ws), ws.numel(), stream())

                def verify(res):
                    assert np.array_equal(res["keep"], ref) and (n < 65 or 0 < len(ref) < n)
                return Case("s2a_nms_rotated_f64", tag, L.s2a_nms_rotated_f64_workspace_bytes(n), lambda: _keep_outputs(n), call,
                            _keep_results(True), verify)
            yield "s2a_nms_rotated_f64", tag, make


@register
def nms_poly_cases():
    for n in (1, 65):
        for form in ("list", "mask"):
            tag = "%s-n%d" % (form, n)

            def make(n=n, form=form, tag=tag):
                _lib, L = lib()
                rng = np.random.default_rng(n)
                polys = oracle.rboxes_to_polys(rand_rboxes(rng, n, span=max(40.0, 9.0 * math.sqrt(n)), lo=8, hi=40))
                dets = np.concatenate([polys, ((rng.permutation(n) + 1.0) / (n + 1.0))[:, None]], 1)
                thr = 0.3
                ref = oracle.nms_poly(dets, thr)
                td = cu(dets)

                def call(outs, ws):
                    return L.s2a_nms_poly(vp(td), n, thr, vp(outs["keep"]), vp(outs["count"]), ctypes.byref(outs["host"]), vp(ws),
                                          ws.numel(), stream())

                def verify(res):
                    assert np.array_equal(res["keep"], ref) and (n < 65 or 0 < len(ref) < n)
                return Case("s2a_nms_poly", tag, L.s2a_nms_poly_workspace_bytes(n), lambda: _keep_outputs(n), call, _keep_results(True),
                            verify, env={"S2A_POLY_NMS_LIST": "1" if form == "list" else "0"})
            yield "s2a_nms_poly", tag, make


# ------------------------------------------------------------------------------------------------ rotated NMS, segmented forms
def _segmented_inputs(n, nseg):
    rng = np.random.default_rng(50 * nseg + n)
    d, s, _ = _nms_inputs(n, 1)
    seg = rng.integers(0, nseg, n).astype(np.int32)
    if n >= 65:
        seg[rng.integers(0, n, 5)] = -1                                              # padding rows
    ngrp = 2 if nseg > 1 else 1
    per = (nseg + ngrp - 1) // ngrp
    grp = np.where(seg >= 0, seg // per, -1).astype(np.int32)
    cls = np.where(seg >= 0, seg % per, -1).astype(np.int32)
    keep = np.zeros(n, bool)
    for c in range(nseg):
        idx = np.nonzero(seg == c)[0]
        if len(idx):
            keep[idx[oracle.nms_rotated(d[idx], s[idx], 0.3)]] = True
    lists = []
    for g in range(ngrp):
        idx = np.nonzero(keep & (grp == g))[0]
        lists.append(idx[np.lexsort((idx, -s[idx].astype(np.float64)))])
    return d, s, seg, grp, cls, ngrp, keep, lists


@register
def nms_segmented_cases():
    for n in (1, 65, 257):
        for nseg in (1, 3):
            for msr in ("n", "1"):
                for entry in ("s2a_nms_rotated_segmented", "s2a_nms_rotated_segmented_dets"):
                    tag = "n%d-seg%d-ws(n,%s)" % (n, nseg, msr)

                    def make(n=n, nseg=nseg, msr=msr, entry=entry, tag=tag):
                        _lib, L = lib()
                        d, s, seg, grp, cls, ngrp, keep, lists = _segmented_inputs(n, nseg)
                        K = max(1, n // 3)                                           # cuts the longer lists
                        D, Sc, Sg, Gr, Cl = cu(d), cu(s), cu(seg), cu(grp), cu(cls)
                        need = L.s2a_nms_rotated_workspace_bytes(n, n if msr == "n" else 1)
                        if entry == "s2a_nms_rotated_segmented":
                            def outputs():
                                return {"flags": Out((n,), torch.uint8), "keep": Out((ngrp, K), torch.int32), "counts": Out((ngrp,), torch.int32)}

                            def call(outs, ws):
                                return L.s2a_nms_rotated_segmented(vp(D), vp(Sc), vp(Sg), vp(Gr), n, nseg, ngrp, 0.3, vp(outs["flags"]),
                                                                   vp(outs["keep"]), vp(outs["counts"]), K, vp(ws), ws.numel(), stream())

                            def verify(res):
                                assert np.array_equal(res["flags"].astype(bool), keep)
                                for g, idx in enumerate(lists):
                                    m = min(len(idx), K)
                                    assert res["counts"][g] == m and np.array_equal(res["keep"][g, :m], idx[:m]) and (res["keep"][g, m:] == -1).all()
                        else:
                            def outputs():
                                return {"wire": Out((ngrp, K * 7 + 1), torch.float32), "labels": Out((ngrp, K), torch.int32),
                                        "counts": Out((ngrp,), torch.int32)}

                            def call(outs, ws):
                                return L.s2a_nms_rotated_segmented_dets(vp(D), vp(Sc), vp(Sg), vp(Gr), vp(Cl), n, nseg, ngrp, 0.3, K,
                                                                        vp(outs["wire"]), vp(outs["labels"]), vp(outs["counts"]), None, None,
                                                                        None, vp(ws), ws.numel(), stream())

                            def verify(res):
                                for g, idx in enumerate(lists):
                                    idx = idx[:K]
                                    m = len(idx)
                                    rows = res["wire"][g, :K * 7].reshape(K, 7)
                                    assert res["counts"][g] == m and res["wire"][g, K * 7] == m
                                    assert np.array_equal(rows[:m, :5], d[idx]) and np.array_equal(rows[:m, 5], s[idx])
                                    assert np.array_equal(rows[:m, 6], cls[idx].astype(np.float32)) and (rows[m:, 6] == -1).all()
                                    assert not rows[m:, :6].any()
                                    assert np.array_equal(res["labels"][g, :m], cls[idx]) and (res["labels"][g, m:] == -1).all()
                        return Case(entry, tag, need, outputs, call, lambda o: {k: v.numpy() for k, v in o.items()}, verify,
                                    short=msr == "1")
                    yield entry, tag, make


# ------------------------------------------------------------------------------------------------ deformable convolution, AlignConv
SMALL = (1, 32, 3, 3, 16)
RAGGED = (2, 64, 5, 7, 64)


def _dcn_inputs(shape, seed):
    B, C, H, W, O = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, C, H, W)).astype(np.float32)
    w = (rng.standard_normal((O, C, 3, 3)) * 0.05).astype(np.float32)
    off = (rng.standard_normal((B, 18, H, W)) * 1.5).astype(np.float32)
    return x, w, off


@register
def dcn_forward_cases():
    for shape in (SMALL, RAGGED, "golden"):
        for dt in ("f32", "f16"):
            if shape == "golden" and dt == "f16":
                continue
            tag = "%s-%s" % ("dcn_small.npz" if shape == "golden" else "x".join(map(str, shape)), dt)

            def make(shape=shape, dt=dt, tag=tag):
                _lib, L = lib()
                if shape == "golden":                                                # C = 16: the generic kernel, the reference's own output
                    g = golden("dcn_small.npz")
                    x, w, off, ref = g["x"], g["weight"], g["offset"], g["out_torch"]
                else:
                    x, w, off = _dcn_inputs(shape, 3)
                td = torch.float32 if dt == "f32" else torch.float16
                tx, tw, toff = cu(x, td), cu(w, td), cu(off)
                if shape != "golden":
                    ref = oracle.deform_conv_forward(tx.float().cpu().numpy(), off, tw.float().cpu().numpy(), f16_cols=dt == "f16")
                B, C, H, W = x.shape
                O = w.shape[0]
                p = _lib.DcnParams(B, C, H, W, O, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, _lib.dtype_code(tx), _lib.DTYPE_F32, _lib.LAYOUT_NCHW, 0)

                def call(outs, ws):
                    return L.s2a_deform_conv_forward(vp(tx), vp(tw), vp(toff), vp(outs["out"]), p, vp(ws), ws.numel(), stream())

                def verify(res):
                    err = np.abs(res["out"].astype(np.float32) - ref)
                    if shape == "golden":
                        assert np.allclose(res["out"], ref, rtol=1e-4, atol=1e-4)   # test_dcn_generic_path_golden
                    elif dt == "f32":
                        assert err.max() < 1e-4, err.max()                           # test_dcn_mfma_f32_vs_oracle
                    else:
                        assert err.max() < 2e-2 and err.mean() < 2e-3, (err.max(), err.mean())   # test_dcn_f16_vs_oracle
                    assert np.abs(ref).max() > 0.1
                return Case("s2a_deform_conv_forward", tag, L.s2a_deform_conv_workspace_bytes(p), lambda: {"out": Out(ref.shape, td)},
                            call, lambda o: {"out": o["out"].numpy()}, verify)
            yield "s2a_deform_conv_forward", tag, make


@register
def align_conv_cases():
    # (O = 16 is not an AlignConv shape: channels % 32 (f32) / 64 (f16), out_channels % 64; the smallest valid one instead)
    for shape in ((1, 64, 3, 3, 64), RAGGED):
        for dt in ("f32", "f16"):
            tag = "%s-%s" % ("x".join(map(str, shape)), dt)

            def make(shape=shape, dt=dt, tag=tag):
                _lib, L = lib()
                B, C, H, W, O = shape
                stride = 8
                rng = np.random.default_rng(5)
                x, w, _ = _dcn_inputs(shape, 5)
                anchors = np.stack([oracle.grid_anchors(H, W, stride) for _ in range(B)])
                anchors[..., 0:2] += rng.normal(0, 4, anchors[..., 0:2].shape)
                anchors[..., 2:4] = 32 * np.exp(rng.normal(0, 0.5, anchors[..., 2:4].shape))
                anchors[..., 4] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, anchors[..., 4].shape)
                anchors = anchors.astype(np.float32)
                td = torch.float32 if dt == "f32" else torch.float16
                tx, tw, ta = cu(x, td), cu(w, td), cu(anchors)
                offs = np.stack([oracle.align_offsets(anchors[b], H, W, stride) for b in range(B)])
                ref = oracle.deform_conv_forward(tx.float().cpu().numpy(), offs, tw.float().cpu().numpy(), relu=True, f16_cols=dt == "f16")
                p = _lib.AlignParams(B, C, H, W, O, float(stride), _lib.dtype_code(tx), _lib.LAYOUT_NCHW, 1, 0)

                def call(outs, ws):
                    return L.s2a_align_conv_forward(vp(tx), vp(ta), vp(tw), vp(outs["out"]), p, vp(ws), ws.numel(), stream())

                def verify(res):
                    err = np.abs(res["out"].astype(np.float32) - ref)
                    if dt == "f32":
                        assert err.max() < 1e-4, err.max()                           # test_alignconv_fused_vs_oracle
                    else:
                        assert err.max() < 2e-2 and err.mean() < 2e-3, (err.max(), err.mean())
                    assert (ref > 0).any() and (ref == 0).any()
                return Case("s2a_align_conv_forward", tag, L.s2a_align_conv_workspace_bytes(p), lambda: {"out": Out((B, O, H, W), td)},
                            call, lambda o: {"out": o["out"].numpy()}, verify)
            yield "s2a_align_conv_forward", tag, make


# ------------------------------------------------------------------------------------------------ fused deformable backward
@functools.lru_cache(maxsize=None)
def _bwd_inputs(shape, dt):
    """inputs rounded to the dtype and the oracle's three gradients: computed once per (shape, dtype), never modified"""
    B, C, H, W, O = shape
    rng = np.random.default_rng(17)
    nd = np.float32 if dt == "f32" else np.float16
    x = rng.standard_normal((B, C, H, W)).astype(nd).astype(np.float32)
    w = (rng.standard_normal((O, C, 3, 3)) * 0.1).astype(nd).astype(np.float32)
    off = (rng.standard_normal((B, 18, H, W)) * 1.5).astype(nd).astype(np.float32)
    go = rng.standard_normal((B, O, H, W)).astype(nd).astype(np.float32)
    gx, goff, gw = oracle.deform_conv_backward(x, off, w, go)
    for a in (x, w, off, go, gx, goff, gw):
        a.setflags(write=False)
    return x, w, off, go, gx, goff, gw


def _bwd_close(got, ref, tol, what):
    err = np.abs(got.astype(np.float32) - ref).max()
    assert err < tol * max(1.0, np.abs(ref).max()), (what, err, np.abs(ref).max())
    assert np.abs(ref).max() > 0.5, what


@register
def dcn_backward_cases():
    # the weight gradient and the one-call forms need channels % 64 == 0 and out_channels % 32 == 0: RAGGED only
    plan = [("s2a_deform_conv_backward_input_f16", "f16", (SMALL, RAGGED)), ("s2a_deform_conv_backward_input_f32", "f32", (SMALL, RAGGED)),
            ("s2a_deform_conv_backward_weight_f16", "f16", (RAGGED,)), ("s2a_deform_conv_backward_weight_f32", "f32", (RAGGED,)),
            ("s2a_deform_conv_backward", "f16", (RAGGED,)), ("s2a_deform_conv_backward", "f32", (RAGGED,)),
            ("s2a_deform_conv_backward_typed", "f16", (RAGGED,)), ("s2a_deform_conv_backward_typed", "f32", (RAGGED,))]
    for entry, dt, shapes in plan:
        for shape in shapes:
            tag = "%s-%s" % ("x".join(map(str, shape)), dt)

            def make(entry=entry, dt=dt, shape=shape, tag=tag):
                _lib, L = lib()
                B, C, H, W, O = shape
                x, w, off, go, gx, goff, gw = _bwd_inputs(shape, dt)
                td = torch.float32 if dt == "f32" else torch.float16
                code = _lib.DTYPE_F32 if dt == "f32" else _lib.DTYPE_F16
                tx, tw, toff, tgo = cu(x, td), cu(w, td), cu(off, td), cu(go, td)
                # the tolerances of test_dcn_backward_{input,weight}_fused_{f16,f32}_vs_oracle
                tol_in, tol_w = (1e-4, 1e-4) if dt == "f32" else (4e-3, 6e-3)
                scale = 0.5
                kind = entry[len("s2a_deform_conv_backward"):]
                zeros = lambda *s: torch.zeros(s, device=DEV)                        # noqa: E731 (accumulated outputs: the caller zeroes them)

                def outputs():
                    o = {}
                    if kind != "_weight_f16" and kind != "_weight_f32":
                        typed = kind == "_typed"
                        o["grad_input"] = Out((B, C, H, W), td if typed else torch.float32, written=typed,
                                              init=None if typed else zeros(B, C, H, W))
                        o["grad_offset"] = Out((B, 18, H, W), td)
                    if kind not in ("_input_f16", "_input_f32"):
                        o["grad_weight"] = Out((O, C, 3, 3), torch.float32, written=False, init=zeros(O, C, 3, 3))
                    return o

                def call(outs, ws):
                    tail = (B, C, H, W, O, vp(ws), ws.numel(), stream())
                    if kind in ("_input_f16", "_input_f32"):
                        fn = L.s2a_deform_conv_backward_input_f16 if dt == "f16" else L.s2a_deform_conv_backward_input_f32
                        return fn(vp(tx), vp(toff), vp(tgo), vp(tw), vp(outs["grad_input"]), vp(outs["grad_offset"]), *tail)
                    if kind == "_weight_f16":
                        return L.s2a_deform_conv_backward_weight_f16(vp(tx), vp(toff), vp(tgo), vp(outs["grad_weight"]), *tail)
                    if kind == "_weight_f32":
                        return L.s2a_deform_conv_backward_weight_f32(vp(tx), vp(toff), vp(tgo), vp(outs["grad_weight"]), scale, *tail)
                    fn = L.s2a_deform_conv_backward_typed if kind == "_typed" else L.s2a_deform_conv_backward
                    return fn(code, vp(tx), vp(toff), vp(tgo), vp(tw), vp(outs["grad_input"]), vp(outs["grad_offset"]),
                              vp(outs["grad_weight"]), scale, *tail)

                def verify(res):
                    if "grad_input" in res:
                        _bwd_close(res["grad_input"], gx, tol_in, "grad_input")
                        _bwd_close(res["grad_offset"], goff, tol_in, "grad_offset")
                    if "grad_weight" in res:
                        _bwd_close(res["grad_weight"], gw * (1.0 if kind == "_weight_f16" else scale), tol_w, "grad_weight")
                q = getattr(L, ENTRY_QUERY[entry])
                need = q(code, B, C, H, W, O) if ENTRY_QUERY[entry] == "s2a_deform_conv_backward_workspace_bytes" else q(B, C, H, W, O)
                return Case(entry, tag, need, outputs, call, lambda o: {k: v.numpy() for k, v in o.items()}, verify)
            yield entry, tag, make


# ------------------------------------------------------------------------------------------------ training convolution
@register
def conv_backward_prep_cases():
    for P, O in ((15, 64), (189, 320)):
        tag = "%dx%d" % (P, O)

        def make(P=P, O=O, tag=tag):
            _lib, L = lib()
            rng = np.random.default_rng(P)
            go = rng.standard_normal((P, O)).astype(np.float16)
            out = np.maximum(rng.standard_normal((P, O)), 0).astype(np.float16)     # a ReLU output: about half zeros
            g_ref = np.where(out <= 0, np.float16(0), go)
            b_ref = g_ref.astype(np.float64).sum(0)
            # f32 sums of P exactly converted halfs in a fixed order: each addition rounds once, |error| <= P * 2^-24 * sum |g|;
            # one more rounding for the stored f32
            b_tol = P * 2.0 ** -24 * np.abs(g_ref.astype(np.float64)).sum(0) + 2.0 ** -24 * np.abs(b_ref)
            tgo, tout = cu(go), cu(out)

            def call(outs, ws):
                return L.s2a_conv_backward_prep_f16(vp(tgo), vp(tout), vp(outs["g"]), vp(outs["grad_bias"]), _lib.DTYPE_F32, P, O, vp(ws),
                                                    ws.numel(), stream())

            def verify(res):
                assert np.array_equal(res["g"].view(np.uint16), g_ref.view(np.uint16)) and (g_ref == 0).any() and (g_ref != 0).any()
                assert (np.abs(res["grad_bias"].astype(np.float64) - b_ref) <= b_tol).all()
            return Case("s2a_conv_backward_prep_f16", tag, L.s2a_conv_backward_prep_f16_workspace_bytes(P, O),
                        lambda: {"g": Out((P, O), torch.float16), "grad_bias": Out((O,), torch.float32)}, call,
                        lambda o: {k: v.numpy() for k, v in o.items()}, verify)
        yield "s2a_conv_backward_prep_f16", tag, make


@register
def conv_backward_weight_cases():
    for name in ("3x3_1x128x320_3x5", "1x1_nobias_2x64x320_5x5"):
        def make(name=name):
            from test_gpu_train_conv import CASES as TRAIN_CASES
            _lib, L = lib()
            k, B, C, O, H, W = TRAIN_CASES[name][:6]
            rng = np.random.default_rng(k)
            x = rng.standard_normal((B, H, W, C)).astype(np.float16)                 # NHWC, as the kernels read them
            g = rng.standard_normal((B, H, W, O)).astype(np.float16)
            x64 = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
            g64 = torch.from_numpy(g.astype(np.float64)).permute(0, 3, 1, 2)

            def wgrad(a, b):                                                         # float64: d/dw of sum(conv2d(a, w) * b)
                w = torch.zeros((O, C, k, k), dtype=torch.float64, requires_grad=True)
                (torch.nn.functional.conv2d(a, w, None, 1, k // 2) * b).sum().backward()
                return w.grad.numpy()
            ref = wgrad(x64, g64)
            # products of two halfs are exact in f32; an entry is a sum of at most B*H*W of them in f32, each addition rounding
            # once: |error| <= B*H*W * 2^-24 * sum |g| |x|, one more rounding for the stored f32
            tol = B * H * W * 2.0 ** -24 * wgrad(x64.abs(), g64.abs()) + 2.0 ** -24 * np.abs(ref)
            tx, tg = cu(x), cu(g)

            def call(outs, ws):
                return L.s2a_conv_backward_weight_f16(vp(tx), vp(tg), vp(outs["grad_weight"]), _lib.DTYPE_F32, B, C, H, W, O, k, vp(ws),
                                                      ws.numel(), stream())

            def verify(res):
                assert (np.abs(res["grad_weight"].astype(np.float64) - ref) <= tol).all() and np.abs(ref).max() > 1.0
            return Case("s2a_conv_backward_weight_f16", name, L.s2a_conv_backward_weight_f16_workspace_bytes(B, C, H, W, O, k),
                        lambda: {"grad_weight": Out((O, C, k, k), torch.float32)}, call, lambda o: {"grad_weight": o["grad_weight"].numpy()},
                        verify)
        yield "s2a_conv_backward_weight_f16", name, make


# ------------------------------------------------------------------------------------------------ training loss
@register
def loss_cases():
    # (B, level sizes): A = 31 anchors on two levels; A = 1364 on five (more than one workgroup per image, a ragged last one)
    for B, sizes in ((1, ((5, 5), (3, 2))), (2, ((32, 32), (16, 16), (8, 8), (4, 4), (2, 2)))):
        A = sum(h * w for h, w in sizes)
        tag = "B%dA%d" % (B, A)

        def make(B=B, sizes=sizes, A=A, tag=tag):
            from s2anet_amd.loss import grid_anchors
            from test_gpu_loss import DEFAULTS, grads_close, ref_loss64
            _lib, L = lib()
            C, n_gt, nl = 15, 6, len(sizes)
            gen = torch.Generator(device=DEV).manual_seed(A)
            strides = [8 * 2 ** l for l in range(nl)]
            rnd = lambda shape, s=1.0: torch.randn(shape, device=DEV, generator=gen) * s   # noqa: E731
            maps = [[rnd((B, ch, h, w), s) + b for h, w in sizes] for ch, s, b in ((C, 1.0, -2.0), (5, 0.5, 0.0), (C, 1.0, -2.0), (5, 0.5, 0.0))]
            init = [grid_anchors(hw, s, 4.0, DEV) for hw, s in zip(sizes, strides)]
            refine = []
            for a, (h, w) in zip(init, sizes):
                r = a.view(1, h, w, 5).repeat(B, 1, 1, 1)
                r[..., :2] += rnd((B, h, w, 2)) * a[0, 2] * 0.1
                r[..., 4] = (torch.rand((B, h, w), device=DEV, generator=gen) - 0.25) * math.pi
                refine.append(r.contiguous())
            ts = torch.empty((B * n_gt, 7), device=DEV)
            ts[:, 0] = torch.arange(B, device=DEV).repeat_interleave(n_gt).float()
            ts[:, 1] = torch.randint(0, C, (B * n_gt,), device=DEV, generator=gen).float()
            ts[:, 2:4] = torch.rand((B * n_gt, 2), device=DEV, generator=gen) * 256
            ts[:, 4:6] = 8 + torch.rand((B * n_gt, 2), device=DEV, generator=gen) * 60
            ts[:, 6] = (torch.rand((B * n_gt,), device=DEV, generator=gen) - 0.25) * math.pi
            off = torch.arange(B + 1, device=DEV, dtype=torch.int64) * n_gt
            ids = torch.randint(-2, n_gt, (2, B, A), device=DEV, generator=gen)      # ignored, negative and positive anchors
            ids[:, :, 0] = 1
            # the float64 restatement and its autograd gradients
            leaves = [[t.detach().clone().requires_grad_(True) for t in lst] for lst in maps]
            rl, ritems = ref_loss64(leaves + [init, refine], ids, ts, off, **DEFAULTS)
            rl.sum().backward()
            ref_grads = [t.grad for lst in leaves for t in lst]
            p = _lib.LossParams()
            p.batch, p.num_classes, p.n_levels = B, C, nl
            p.fl_gamma, p.fl_alpha, p.smooth_l1_beta = DEFAULTS["fl_gamma"], DEFAULTS["fl_alpha"], DEFAULTS["smoothL1_beta"]
            p.reg_balance, p.odm_balance = DEFAULTS["reg_balance"], DEFAULTS["odm_balance"]
            names = ["g%d_%d" % (k, l) for k in range(4) for l in range(nl)]

            def outputs():
                o = {n: Out(tuple(maps[k][l].shape), torch.float32) for n, (k, l) in zip(names, ((k, l) for k in range(4) for l in range(nl)))}
                o.update(loss=Out((1,), torch.float32), items=Out((4,), torch.float32), norm=Out((4,), torch.float32))
                return o

            def call(outs, ws):
                for m in range(2):
                    for l, (h, w) in enumerate(sizes):
                        e = p.map[m][l]
                        e.cls, e.bbox = maps[2 * m][l].data_ptr(), maps[2 * m + 1][l].data_ptr()
                        e.anchors = (refine if m else init)[l].data_ptr()
                        e.grad_cls, e.grad_bbox = outs["g%d_%d" % (2 * m, l)].data_ptr(), outs["g%d_%d" % (2 * m + 1, l)].data_ptr()
                        e.anchor_batch_stride, e.height, e.width = (h * w * 5 if m else 0), h, w
                        e.cls_dtype = e.bbox_dtype = _lib.DTYPE_F32
                        e.fpn_balance = 1.0
                return L.s2a_s2anet_loss_forward(p, vp(ids), vp(ts), vp(off), vp(outs["loss"]), vp(outs["items"]), vp(outs["norm"]), vp(ws),
                                                 ws.numel(), stream())

            def verify(res):
                # the bounds of test_gpu_loss.check_against_restatement
                np.testing.assert_allclose(res["items"], ritems.detach().cpu().numpy(), rtol=2e-5, atol=1e-7)
                np.testing.assert_allclose(res["loss"], rl.detach().cpu().numpy(), rtol=2e-5, atol=1e-7)
                assert res["items"].min() > 0
                for j, n in enumerate(names):                                        # d loss / d map = raw gradient x its normaliser
                    grads_close(torch.from_numpy(res[n].astype(np.float64) * float(res["norm"][j // nl])), ref_grads[j])
            return Case("s2a_s2anet_loss_forward", tag, L.s2a_s2anet_loss_workspace_bytes(B, A), outputs, call,
                        lambda o: {k: v.numpy() for k, v in o.items()}, verify)
        yield "s2a_s2anet_loss_forward", tag, make


# ------------------------------------------------------------------------------------------------ scene merge
@register
def scene_merge_cases():
    for n_rows in (1, 300):
        for cap in (0, 256):
            tag = "rows%d-cap%d" % (n_rows, cap)

            def make(n_rows=n_rows, cap=cap, tag=tag):
                from s2anet_amd.scene import SceneDetections
                from test_gpu_scene import assert_equals_oracle, make_rows, oracle_merge
                _lib, L = lib()
                C = 15
                if n_rows == 1:
                    rows = dict(dets=np.array([[[100.0, 90.0, 40.0, 20.0, 0.3, 0.75]]], np.float32), labels=np.array([[4]], np.int32),
                                counts=np.array([1], np.int32), origins=np.array([[824, 0]], np.int32), rates=np.array([1.0]))
                else:
                    rows = make_rows(23, 1500, 1500, 40, K=75)                       # 2 x 2 chips of 75 slots, ragged counts
                n_chips, K = rows["labels"].shape
                assert n_chips * K == n_rows
                want = oracle_merge(rows)
                td, tl, tc, to, tr = (cu(rows[k]) for k in ("dets", "labels", "counts", "origins", "rates"))

                def outputs():
                    return {"polys": Out((n_rows, 8), torch.float64), "scores": Out((n_rows,), torch.float64), "labels": Out((n_rows,), torch.int64),
                            "src": Out((n_rows,), torch.int64), "class_counts": Out((C,), torch.int64), "status": Out((4,), torch.int64)}

                def call(outs, ws):
                    return L.s2a_scene_merge(vp(td), vp(tl), vp(tc), vp(to), vp(tr), n_chips, K, C, 0.5, cap, vp(outs["polys"]),
                                             vp(outs["scores"]), vp(outs["labels"]), vp(outs["src"]), vp(outs["class_counts"]),
                                             vp(outs["status"]), vp(ws), ws.numel(), stream())

                def verify(res):
                    r = SceneDetections(*(torch.from_numpy(res[k]) for k in ("polys", "scores", "labels", "src", "class_counts", "status")))
                    assert_equals_oracle(r, want, tag)
                    assert n_rows == 1 or 0 < want[4].sum() < rows["counts"].sum()
                return Case("s2a_scene_merge", tag, L.s2a_scene_merge_workspace_bytes(n_rows, cap), outputs, call,
                            lambda o: {k: v.numpy() for k, v in o.items()}, verify)
            yield "s2a_scene_merge", tag, make


# ------------------------------------------------------------------------------------------------ Task-1 evaluation
class _Refused(Exception):
    pass


@register
def eval_cases():
    for D, G, C, I in ((1, 1, 1, 1), (65, 33, 3, 2)):
        tag = "D%dG%dC%dI%d" % (D, G, C, I)

        def make(D=D, G=G, C=C, I=I, tag=tag):
            from s2anet_amd import evaluate
            from test_gpu_eval import KEYS, assert_equals_reference, cpu_reference, host, make_data
            _lib, L = lib()
            rng = np.random.default_rng(D)
            full = make_data(rng, C, I, n_gt=G, n_fa=2 * D, dup=(1, 3), span=120.0)
            assert full["ds"].size >= D and full["gl"].size == G
            data = {k: (v[:D] if k[0] == "d" else v) for k, v in full.items()}        # the first D detections of the shuffled rows
            ref = cpu_reference(data, C, I)
            tens = [cu(data[k]) for k in KEYS]
            sizes = dict(order=D, ovmax=D, argmax=D, tp_cum=D, fp_cum=D, rec=D, prec=D, seg_start=C + 1)

            def outputs():
                return {"_store": {}}

            def call(outs, ws):
                # through the Python host side, which owns the long argument list: its workspace and its error check replaced
                store = outs["_store"]

                def alloc(name, n, dtype):
                    assert n == sizes.get(name, C)
                    store[name] = outs[name] = Out((n,), dtype)
                    return outs[name].value()

                def workspace(nbytes, device, tag_):
                    assert nbytes == need and tag_ == "eval_task1"
                    return ws

                def check(rc):
                    if rc != _lib.OK:
                        raise _Refused(rc)
                keep = _lib.workspace, _lib.check
                _lib.workspace, _lib.check = workspace, check
                try:
                    outs["_res"] = evaluate.evaluate_task1(*tens, C, I, curves=True, alloc=alloc)
                    return _lib.OK
                except _Refused as e:
                    return e.args[0]
                finally:
                    _lib.workspace, _lib.check = keep

            def results(o):
                return host(o["_res"])

            def verify(res):
                assert_equals_reference(res, ref, True, tag)
                assert res["ndet"].sum() == D and (D == 1 or res["valid"].any())
            need = L.s2a_eval_task1_workspace_bytes(D, G, C, I)
            return Case("s2a_eval_task1", tag, need, outputs, call, results, verify)
        yield "s2a_eval_task1", tag, make


# ------------------------------------------------------------------------------------------------ the tests
def test_every_entry_point_of_the_audit_has_a_case():
    covered = {p.id.split("-")[0] for p in CASES} | {"train_update"}
    assert covered == {op[len("s2a_"):] for op in ENTRY_QUERY}, covered ^ {op[len("s2a_"):] for op in ENTRY_QUERY}


@pytest.mark.parametrize("make", CASES)
def test_workspace_contract(make, monkeypatch):
    run_contract(make(), monkeypatch)


# ------------------------------------------------------------------------------------------------ the training update
def _update_specs(which):
    from optim_twin import Spec
    from test_gpu_optim import make_specs
    if which == "one_chunk":
        g = torch.Generator().manual_seed(3)
        return [Spec("t5", torch.randn(5, generator=g), "param", 1), Spec("stat", torch.randn(19, generator=g), "buffer")]
    return make_specs()


def _update_steps(specs, scale_of, step_fn):
    """three steps of the twelve-step sequence's inputs, the middle one its inf step -> what step_fn returned per step"""
    from test_gpu_optim import INF_STEP, LAST, step_inputs
    gen = torch.Generator().manual_seed(5)
    has_last = any(s.name == LAST for s in specs)                  # (step_inputs puts its inf into that tensor)
    out = []
    for step in (INF_STEP - 1, INF_STEP, INF_STEP + 1):
        grads, lrs, stat = step_inputs(specs, step, scale_of(), gen, inf=has_last)
        if step == INF_STEP and not has_last:
            grads["t5"][-1] = float("inf")
        out.append(step_fn(grads, lrs, stat))
    return out


@pytest.mark.parametrize("which", ["one_chunk", "twelve_step_specs"])
def test_train_update_on_scratch_that_was_never_zero(which):
    """s2a_train_update has only ever seen the zeroed workspace TrainUpdate owns: here its workspace is a guarded view of exactly
    s2a_train_update_workspace_bytes(n_trained_chunks) bytes, replaced after construction and before the first step; three steps,
    the inf step among them, against the float64 Twin at the tolerance of test_gpu_optim; bit-equal for all three fills"""
    import copy
    from optim_twin import Twin
    from s2anet_amd import TrainUpdate
    from test_gpu_optim import GROUPS, KW, Holder, build, check_against_twin, gpu_step, snapshot
    _lib, L = lib()
    specs = _update_specs(which)

    def construct():
        if which == "one_chunk":
            model = Holder(specs)
            avg = copy.deepcopy(model).eval()
            upd = TrainUpdate([{"params": [model.t5], **GROUPS[1]}], model, avg, **KW)
            return model, avg, upd
        return build(specs)

    def twin(dtype):
        sp = specs
        groups = GROUPS
        if which == "one_chunk":
            from optim_twin import Spec
            sp = [Spec(s.name, s.init, s.kind, 0) for s in specs]
            groups = [GROUPS[1]]
        t = Twin(sp, groups, dtype=dtype, **KW)

        def step(grads, lrs, stat):
            info = t.step(grads, lrs[1:2] if which == "one_chunk" else lrs, buffers={"stat": stat})
            state = {"scale": t.scale, "growth_tracker": t.growth_tracker, "updates": t.updates, **info}
            for s in specs:
                state["p/" + s.name] = t.value[s.name].detach().clone()
                state["ema/" + s.name] = t.ema[s.name].clone()
                if s.kind == "param":
                    state["buf/" + s.name] = t.buf(s.name).detach().clone()
            return state
        return _update_steps(specs, lambda: t.scale, step)
    f64, f32 = twin(torch.float64), twin(torch.float32)
    assert [w["found_inf"] for w in f64] == [False, True, False]

    def guard(upd, gw):
        """the owned zero workspace and the three small outputs -> guarded ones, in the argument block the launch reads"""
        need = L.s2a_train_update_workspace_bytes(upd.n_trained_chunks)
        assert need > 0 and (which != "one_chunk" or upd.n_trained_chunks == 1)
        upd._ws = gw(need, torch.device(DEV), "train_update")
        assert upd._ws.data_ptr() % 16 == 0
        outs = {}
        for name, attr in (("stats", "stats"), ("scale", "scale"), ("counters", "counters")):
            old = getattr(upd, attr)
            o = Out(tuple(old.shape), old.dtype, written=name == "stats", init=None if name == "stats" else old)
            setattr(upd, attr, o.value())
            setattr(upd._args, name, o.data_ptr())
            outs[name] = o
        return need, outs

    runs = []
    for fill, slack in ((0x00, generous), (0xA5, None), (0xFF, None)):
        model, avg, upd = construct()
        gw = GuardedWorkspaces(fill, slack)
        need, outs = guard(upd, gw)
        assert slack is not None or upd._ws.numel() == need

        def step(grads, lrs, stat):
            gpu_step(model, upd, grads, lrs[1:2] if which == "one_chunk" else lrs, stat)
            torch.cuda.synchronize()
            gw.check()                                                                # (b) after every call
            assert all(o.guard_ok() for o in outs.values())                          # (c)
            assert not outs["stats"].holds_fill()
            return snapshot(specs, model, avg, upd)
        snaps = _update_steps(specs, lambda: float(upd.scale.item()), step)
        worst = [0.0]
        for i, (g, w, s) in enumerate(zip(snaps, f64, f32)):                          # (a): the twin, as test_twelve_steps_match_...
            st = g["stats"]
            assert g["scale"] == w["scale"] == st[4] and g["counters"] == [w["growth_tracker"], w["updates"]], (fill, i)
            assert bool(st[2]) == w["found_inf"] and bool(st[3]) == w["skipped"], (fill, i)
            if not w["found_inf"]:
                assert abs(float(st[0]) - w["norm"]) <= 16 * 2.0 ** -24 * w["norm"], (fill, i, st[0], w["norm"])
            check_against_twin(specs, g, w, s, "fill %#04x step %d" % (fill, i), worst)
        runs.append(snaps)
    for other, fill in ((runs[1], 0xA5), (runs[2], 0xFF)):                            # (a): invariance, bit for bit
        for a, b in zip(runs[0], other):
            for k in a:
                same = np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else (
                    torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])
                assert same, "s2a_train_update: %s depends on the scratch contents (fill %#04x)" % (k, fill)
    # (d) one byte short, then NULL: refused with S2A_EWORKSPACE, nothing launched
    model, avg, upd = construct()
    gw = GuardedWorkspaces(0xA5)
    need, outs = guard(upd, gw)
    before = snapshot(specs, model, avg, upd)
    for what, ptr, nbytes in (("one byte short", upd._ws.data_ptr(), need - 1), ("NULL workspace", 0, need)):
        rc = L.s2a_train_update(ctypes.byref(upd._args), ctypes.c_void_p(ptr), nbytes, stream())
        torch.cuda.synchronize()
        msg = last_error()
        assert rc == _lib.EWORKSPACE and "train_update" in msg and "workspace" in msg, (what, rc, msg)
        after = snapshot(specs, model, avg, upd)
        for k in before:
            same = np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else (
                torch.equal(before[k], after[k]) if torch.is_tensor(before[k]) else before[k] == after[k])
            assert same, (what, k)
        assert all(o.untouched() for o in outs.values()) and gw.untouched(), what
