"""CPU: the batched label assignment's surface -- symbols exported and bound, argument checks that answer before any HIP
call, wrappers that refuse CPU tensors, the head's capturable loss entry."""
import ctypes
import inspect

import pytest
import torch


def test_symbols_are_exported_and_bound():
    import s2anet_amd as S
    from s2anet_amd import _lib
    L = _lib.lib()
    for name in ("s2a_assign_labels_batched", "s2a_assign_labels_batched_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert "assign_labels_batched" in S.__all__ and callable(S.assign_labels_batched)
    assert ctypes.sizeof(_lib.AnchorSet) == 16
    # the workspace grows with every size; sizes the call refuses have none
    small = L.s2a_assign_labels_batched_workspace_bytes(2, 2, 1364, 96, 1000)
    assert small > 0
    assert L.s2a_assign_labels_batched_workspace_bytes(2, 2, 1364, 96, 2000) > small
    assert L.s2a_assign_labels_batched_workspace_bytes(2, 4, 1364, 96, 1000) > small
    assert L.s2a_assign_labels_batched_workspace_bytes(2, 2, 1364, 960, 1000) > small
    assert L.s2a_assign_labels_batched_workspace_bytes(0, 2, 1364, 96, 1000) == 0
    assert L.s2a_assign_labels_batched_workspace_bytes(2, 2, 1364, -1, 1000) == 0


def test_argument_checks_return_codes_without_touching_the_gpu():
    from s2anet_amd import _lib
    L = _lib.lib()
    z = ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)          # never dereferenced: the checks fail first
    sets = (_lib.AnchorSet * 5)()
    for e in sets:
        e.anchors, e.batch_stride = 16, 0
    sets[1].batch_stride = 50

    def call(n_sets=2, batch=2, anchors=10, cap=4, pairs=80, table=sets, targets=one, ids=one, sorted_t=one, offsets=one,
             status=one, pos=0.5, min_pos=0.0, ws=one, ws_bytes=1 << 30):
        rc = L.s2a_assign_labels_batched(table, n_sets, batch, anchors, targets, cap, z, 100.0, 100.0, pos, 0.4, min_pos, 1, 1, 1,
                                         ids, sorted_t, offsets, status, pairs, ws, ws_bytes, z)
        return rc, L.s2a_last_error().decode()

    for n in (0, 5, -1):
        rc, msg = call(n_sets=n)
        assert rc == _lib.EINVAL and "1 to 4 anchor sets" in msg
    for kw in (dict(batch=-1), dict(batch=0), dict(anchors=-3), dict(cap=-1), dict(pairs=-1)):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and "negative or empty size" in msg, kw
    rc, msg = call(batch=1 << 20)
    assert rc == _lib.EINVAL and "out of range" in msg
    for kw in (dict(ids=z), dict(sorted_t=z), dict(offsets=z), dict(status=z), dict(targets=z),
               dict(table=ctypes.cast(z, ctypes.POINTER(_lib.AnchorSet)))):
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and "NULL" in msg, kw
    null_set = (_lib.AnchorSet * 2)()
    null_set[0].anchors = 16
    rc, msg = call(table=null_set)
    assert rc == _lib.EINVAL and "NULL" in msg and "set 1" in msg
    sets[1].batch_stride = 49                                     # neither shared nor a whole image apart
    rc, msg = call()
    assert rc == _lib.EINVAL and "batch_stride" in msg
    sets[1].batch_stride = 50
    rc, msg = call(pos=0.0)
    assert rc == _lib.EINVAL and "pos_iou_thr > 0" in msg
    rc, msg = call(min_pos=-0.1)
    assert rc == _lib.EINVAL and "min_pos_iou_thr >= 0" in msg
    rc, msg = call(ws=ctypes.c_void_p(24))
    assert rc == _lib.EINVAL and "aligned" in msg
    rc, msg = call(ws_bytes=1)
    assert rc == _lib.EWORKSPACE and "too small" in msg
    rc, msg = call(ws=z, ws_bytes=0)
    assert rc == _lib.EWORKSPACE and "too small" in msg
    need = L.s2a_assign_labels_batched_workspace_bytes(2, 2, 10, 4, 80)
    rc, msg = call(ws_bytes=need - 1024 - 1)
    assert rc == _lib.EWORKSPACE and "too small" in msg


def test_wrappers_refuse_cpu_tensors():
    import s2anet_amd as S
    from s2anet_amd.head import S2ANetHead
    a = torch.zeros(6, 5)
    with pytest.raises(NotImplementedError):
        S.assign_labels_batched([a, a[None].repeat(2, 1, 1)], torch.zeros(3, 7), 2)
    head = S2ANetHead(15)
    p = [[torch.zeros(1, 15, 2, 2)], [torch.zeros(1, 5, 2, 2)], [torch.zeros(1, 15, 2, 2)], [torch.zeros(1, 5, 2, 2)],
         [torch.zeros(1, 2, 2, 5)]]
    with pytest.raises(NotImplementedError):
        head.compute_loss_device(p, torch.zeros(1, 7))


def test_head_has_the_capturable_loss_entry():
    from s2anet_amd.head import S2ANetHead
    sig = inspect.signature(S2ANetHead.compute_loss_device)
    assert list(sig.parameters) == ["self", "p", "targets", "num_targets", "pair_capacity"]
    assert sig.parameters["num_targets"].default is None and sig.parameters["pair_capacity"].default is None
    assert list(inspect.signature(S2ANetHead.compute_loss).parameters) == ["self", "p", "targets"]
    src = inspect.getsource(S2ANetHead.compute_loss_device)
    for word in (".tolist(", ".item(", "bincount", "nonzero", ".cpu("):
        assert word not in src, word
