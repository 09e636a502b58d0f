"""CPU: the *_workspace_bytes() queries of the C ABI over the small-shape grid of tests/test_gpu_workspace_contract.py --
positive for a valid problem, 0 for one the entry point refuses (the convention of s2a_assign_labels_batched_workspace_bytes,
tests/test_assign_batched_cpu.py), and non-decreasing when any one size argument grows by one step: a query that wraps or
drops a term shows up here, without a GPU.  And the audit table of the GPU test names exactly the queries the library exports."""
import ctypes

import pytest

from test_gpu_workspace_contract import AUDIT, ENTRY_QUERY

F32, F16 = 0, 1
SMALL, RAGGED = (1, 32, 3, 3, 16), (2, 64, 5, 7, 64)


def _dcn(L, lib, B, C, H, W, O, dtype=F32):
    p = lib.DcnParams(B, C, H, W, O, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, dtype, F32, lib.LAYOUT_NCHW, 0)
    return L.s2a_deform_conv_workspace_bytes(ctypes.byref(p))


def _align(L, lib, B, C, H, W, O, dtype=F32):
    p = lib.AlignParams(B, C, H, W, O, 8.0, dtype, lib.LAYOUT_NCHW, 1, 0)
    return L.s2a_align_conv_workspace_bytes(ctypes.byref(p))


# query -> (valid argument tuples, refused argument tuples, step of each size argument (None: not a size))
# a step larger than one: the entry point takes multiples of it only (channel counts of the matrix kernels)
GRID = {
    "s2a_box_iou_rotated_workspace_bytes": ([(1, 1), (3, 257)], [(-1, 1), (1, -1), (1 << 31, 1)], (1, 1)),
    "s2a_assign_labels_workspace_bytes": ([(1, 1), (1364, 3), (1364, 129)], [(-1, 1), (1, -1)], (1, 1)),
    "s2a_assign_labels_batched_workspace_bytes": ([(1, 1, 1, 1, 1), (2, 2, 1364, 132, 256)],
                                                  [(0, 1, 1, 1, 1), (5, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, -1, 1),
                                                   (1, 1, 1, 1, -1)], (None, 1, 1, 1, 1)),
    "s2a_nms_poly_workspace_bytes": ([(1,), (65,)], [(-1,)], (1,)),
    "s2a_nms_rotated_workspace_bytes": ([(1, 1), (65, 65), (65, 1), (257, 257), (257, 1)], [(-1, 1)], (1, 1)),
    "s2a_nms_rotated_f64_workspace_bytes": ([(1,), (65,), (257,)], [(-1,)], (1,)),
    "s2a_multiclass_candidates_workspace_bytes": ([(15,), (15 * 257,)], [(-1,), (1 << 31,)], (1,)),
    "s2a_deform_conv_workspace_bytes": ([SMALL, RAGGED, (2, 16, 6, 7, 8)], [(1, 0, 3, 3, 16), (-1, 32, 3, 3, 16), (1, 32, 3, 3, 0)],
                                        (1, 1, 1, 1, 1)),
    "s2a_align_conv_workspace_bytes": ([(1, 64, 3, 3, 64), RAGGED], [(1, 64, 2, 3, 64), (1, 0, 3, 3, 64), (-1, 64, 3, 3, 64)],
                                       (1, 1, 1, 1, 1)),
    "s2a_scene_merge_workspace_bytes": ([(1, 0), (1, 256), (300, 0), (300, 256)], [(-1, 0)], (1, 1)),
    "s2a_eval_task1_workspace_bytes": ([(1, 1, 1, 1), (65, 33, 3, 2), (0, 0, 1, 1)],
                                       [(-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, 0, 1), (1, 1, 1025, 1), (1, 1, 1, 0)], (1, 1, 1, 1)),
    "s2a_conv_backward_prep_f16_workspace_bytes": ([(15, 64), (189, 320)], [(0, 64), (15, 0), (15, 72), (-1, 64)], (1, 64)),
    "s2a_conv_backward_weight_f16_workspace_bytes": ([(1, 128, 3, 5, 320, 3), (2, 64, 5, 5, 320, 1)],
                                                     [(0, 64, 5, 5, 64, 3), (1, 96, 5, 5, 64, 3), (1, 64, 5, 5, 72, 3), (1, 64, 5, 5, 64, 2),
                                                      (1, 64, 0, 5, 64, 3)], (1, 64, 1, 1, 64, None)),
    "s2a_deform_conv_backward_input_workspace_bytes": ([SMALL, RAGGED], [(-1, 32, 3, 3, 16), (1, 0, 3, 3, 16), (1, 32, 2, 3, 16), (1, 32, 3, 3, 0)],
                                                       (1, 1, 1, 1, 1)),
    "s2a_deform_conv_backward_input_f32_workspace_bytes": ([SMALL, RAGGED], [(-1, 32, 3, 3, 16), (1, 32, 3, 2, 16)], (1, 1, 1, 1, 1)),
    "s2a_deform_conv_backward_weight_workspace_bytes": ([RAGGED], [(-1, 64, 5, 7, 64), (2, 64, 5, 7, 0)], (1, 1, 1, 1, 1)),
    "s2a_deform_conv_backward_weight_f32_workspace_bytes": ([RAGGED], [(-1, 64, 5, 7, 64), (2, 0, 5, 7, 64)], (1, 1, 1, 1, 1)),
    "s2a_deform_conv_backward_workspace_bytes": ([(F16,) + RAGGED, (F32,) + RAGGED], [(2,) + RAGGED, (F16, -1, 64, 5, 7, 64)],
                                                 (None, 1, 1, 1, 1, 1)),
    "s2a_s2anet_loss_workspace_bytes": ([(1, 31), (2, 1364)], [(0, 31), (1, 0), (-1, 31)], (1, 1)),
    "s2a_train_update_workspace_bytes": ([(1,), (21,), (0,)], [(-1,)], (1,)),
}


def call(name, args):
    from s2anet_amd import _lib
    L = _lib.lib()
    if name == "s2a_deform_conv_workspace_bytes":
        return _dcn(L, _lib, *args)
    if name == "s2a_align_conv_workspace_bytes":
        return _align(L, _lib, *args)
    return getattr(L, name)(*args)


def test_the_audit_names_every_exported_query():
    """every *_workspace_bytes symbol of the built library has a row in the audit of the GPU test, a grid here, and every
    entry point that takes (workspace, workspace_bytes) belongs to a row"""
    import re
    import subprocess
    from s2anet_amd import _lib
    _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(s2a_\w+_workspace_bytes)\b", out))
    assert len(exported) == 20
    assert exported == set(AUDIT) == set(GRID), (exported ^ set(AUDIT), exported ^ set(GRID))
    assert exported == {n for n in _lib.SYMBOLS if n.endswith("_workspace_bytes")}
    # an entry point takes a workspace when its bound signature ends (..., void* workspace, size_t bytes, stream)
    takes = {n for n, (res, args) in _lib.SYMBOLS.items() if len(args) >= 3 and args[-2] is ctypes.c_size_t and args[-3] is ctypes.c_void_p}
    assert takes == set(ENTRY_QUERY), takes ^ set(ENTRY_QUERY)
    for row in AUDIT.values():
        assert row["buffers"] and all(len(b) == 2 and all(b) for b in row["buffers"])
        assert row["reproducible"] is True or (isinstance(row["reproducible"], tuple) and row["reproducible"])


@pytest.mark.parametrize("name", sorted(GRID))
def test_query_is_positive_zero_for_refused_sizes_and_monotone(name):
    valid, refused, steps = GRID[name]
    for args in valid:
        base = call(name, args)
        assert base > 0, (name, args)
        assert call(name, args) == base                                    # the same answer twice
        for i, step in enumerate(steps):
            if step is None or (name == "s2a_scene_merge_workspace_bytes" and i == 1 and args[1] == 0):
                continue                                                   # (pair_capacity 0 is not a size: "derive it from n_rows")
            grown = tuple(a + step if j == i else a for j, a in enumerate(args))
            assert call(name, grown) >= base, (name, args, "argument %d grown by %d" % (i, step), call(name, grown), base)
    for args in refused:
        assert call(name, args) == 0, (name, args, call(name, args))


def test_null_parameter_blocks_have_no_workspace():
    from s2anet_amd import _lib
    L = _lib.lib()
    assert L.s2a_deform_conv_workspace_bytes(None) == 0 and L.s2a_align_conv_workspace_bytes(None) == 0
