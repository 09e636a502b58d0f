"""GPU: the batched, sync-free label assignment (s2a_assign_labels_batched, csrc/assign_ops.hip) and the loss routes built on
it (S2ANetHead.compute_loss_device / compute_loss).  Comparators: oracle.assign_labels per (set, image) -- the CPU
restatement pinned to the reference's own Python by tests/golden/assign_labels.npz -- and the per-image op assign_labels;
never the batched code's own output."""
import functools
import math

import numpy as np
import pytest
import torch

import oracle
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE = 256
STRIDES = (8, 16, 32, 64, 128)
B = 4
# per-image gt counts of the three calls: 0 and 1, both sides of a wave (63 / 64 / 65), both sides of the cull's LDS chunk of
# 128 gts (127 / 128 / 129), several chunks (257, 300), an empty image between full ones
COUNTS = ((0, 1, 63, 64), (65, 127, 128, 129), (257, 0, 300, 2))
SETTINGS = (dict(), dict(gt_max_assign_all=False), dict(pos_iou_thr=0.3, neg_iou_thr=0.1, min_pos_iou_thr=0.2))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def pyramid():
    """-> (grid anchors [A,5], per-image perturbed anchors [B,A,5]), A = 1 364: at 256^2 the anchors of strides 64 / 128
    (256 / 512 px) are all invalid, so the -2 rule is exercised"""
    rng = np.random.default_rng(11)
    levels = []
    for s in STRIDES:
        n = SIZE // s
        ys, xs = np.meshgrid(np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32), indexing="ij")
        a = np.zeros((n, n, 5), np.float32)
        a[..., 0] = xs * s + 0.5 * (s - 1)
        a[..., 1] = ys * s + 0.5 * (s - 1)
        a[..., 2:4] = 4.0 * s
        levels.append(a.reshape(-1, 5))
    grid = np.concatenate(levels)
    assert grid.shape == (1364, 5)
    ref = np.repeat(grid[None], B, 0).copy()
    ref[..., :2] += (rng.standard_normal((B, 1364, 2)) * grid[None, :, 2:3] * 0.1).astype(np.float32)
    ref[..., 2:4] *= np.exp(rng.standard_normal((B, 1364, 2)) * 0.2).astype(np.float32)
    ref[..., 4] = ((rng.random((B, 1364)) - 0.25) * math.pi).astype(np.float32)
    return grid, ref.astype(np.float32)


def make_targets(counts, seed):
    """[G,7] targets in shuffled order.  Every image of 8 or more gts holds: two identical rows, a gt exactly equal to a grid
    anchor, a gt far outside the image, a gt with w = 0, and one gt that all such images share"""
    rng = np.random.default_rng(seed)
    grid, _ = pyramid()
    shared = np.array([100.5, 90.25, 44.0, 21.0, 0.4], np.float32)
    rows = []
    for b, n in enumerate(counts):
        t = np.zeros((n, 7), np.float32)
        t[:, 0] = b
        t[:, 1] = rng.integers(0, 15, n)
        t[:, 2:4] = rng.uniform(0, SIZE, (n, 2))
        t[:, 4:6] = 8 + rng.uniform(0, 80, (n, 2))
        t[:, 6] = (rng.random(n) - 0.25) * math.pi
        if n >= 8:
            t[1, 2:] = t[0, 2:]
            t[2, 2:] = grid[5 * 32 + 7 + b]                      # a stride-8 grid anchor, exactly
            t[3, 2:4] = (5000.0, -3000.0)
            t[4, 4] = 0.0
            t[5, 2:] = shared
            t[n - 1, 2:] = grid[1024 + 3 * 16 + 9]               # and a stride-16 one as the image's last gt
        rows.append(t)
    t = np.concatenate(rows)
    return np.ascontiguousarray(t[rng.permutation(t.shape[0])])


def sort_reference(t, batch):
    """t[argsort(image, stable)] over the rows of images [0, batch), and the cumulative counts"""
    img = t[:, 0].astype(np.int64)
    keep = (img >= 0) & (img < batch)
    t, img = t[keep], img[keep]
    ts = t[np.argsort(img, kind="stable")]
    off = np.zeros(batch + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(img, minlength=batch)[:batch])
    return ts, off


def oracle_ids(sets, ts, off, imgs_size, **kw):
    """oracle.assign_labels of every (set, image) -> [S,B,A]"""
    out = []
    for a in sets:
        per = []
        for b in range(len(off) - 1):
            ab = a if a.ndim == 2 else a[b]
            per.append(oracle.assign_labels(ab, ts[off[b]:off[b + 1], 2:7], imgs_size=imgs_size, **kw))
        out.append(np.stack(per))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def case(i):
    """inputs of call i and the oracle's ids at the default settings: computed once, shared, never modified"""
    t = make_targets(COUNTS[i], 100 + i)
    ts, off = sort_reference(t, B)
    assert tuple(np.diff(off)) == COUNTS[i]
    want = oracle_ids(pyramid(), ts, off, (SIZE, SIZE))
    for a in (t, ts, off, want):
        a.setflags(write=False)
    return t, ts, off, want


def run_batched(t, **kw):
    from s2anet_amd import assign_labels_batched
    grid, ref = pyramid()
    return assign_labels_batched((cu(grid), cu(ref)), t if torch.is_tensor(t) else cu(t), B, imgs_size=(SIZE, SIZE), **kw)


# ----------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("i", range(len(COUNTS)))
def test_parity_with_oracle_and_per_image_op(i):
    from s2anet_amd.rotated import assign_labels
    t, ts, off, want_default = case(i)
    grid, ref = pyramid()
    for kw in SETTINGS:
        ids, got_ts, got_off, status = run_batched(t, **kw)
        assert ids.shape == (2, B, 1364) and ids.dtype == torch.int64 and status.dtype == torch.int64
        st = status.cpu().numpy()
        assert st[0] == 0 and st[2] == ts.shape[0] and st[3] == 0 and st[1] > 0, st
        assert np.array_equal(got_ts.cpu().numpy().view(np.uint32), ts.view(np.uint32))
        assert np.array_equal(got_off.cpu().numpy(), off)
        want = want_default if not kw else oracle_ids((grid, ref), ts, off, (SIZE, SIZE), **kw)
        got = ids.cpu().numpy()
        assert np.array_equal(got, want), (kw, int((got != want).sum()))
        for s, a in enumerate((grid, ref)):
            for b in range(B):
                ab = cu(a if a.ndim == 2 else a[b])
                per = assign_labels(ab, cu(ts[off[b]:off[b + 1], 2:7]), imgs_size=(SIZE, SIZE), **kw).cpu().numpy()
                assert np.array_equal(got[s, b], per), (kw, s, b)
    # the rules are all exercised: ignored (-2, the oversized levels), negatives, positives
    # (grid anchors: the 20 of strides 64 / 128 are invalid, the other 1 344 valid)
    assert (want_default[0, :, 1344:] == -2).all() and (want_default == -1).any() and (want_default >= 0).any()
    assert (want_default[0, np.array(COUNTS[i]) == 0, :1344] == -1).all()           # the empty-image rule


# ----------------------------------------------------------------------------- 2. padding
@pytest.mark.parametrize("i", range(len(COUNTS)))
def test_padding_rows_and_device_row_count(i):
    t, ts, off, want = case(i)
    G = t.shape[0]
    cap = 2 * G + 40
    rng = np.random.default_rng(5)
    table = np.full((cap, 7), -1.0, np.float32)
    table[:, 2:] = rng.uniform(0, SIZE, (cap, 5))                # padding rows hold plausible boxes: only the image index says so
    at = np.sort(rng.choice(2 * G + 8, G, replace=False))        # the real rows, -1 rows interleaved, in the same order
    table[at] = t
    free = np.setdiff1d(np.arange(2 * G + 8), at)
    table[free[0], 0] = B                                        # an image index >= B is padding too
    table[free[1], 0] = B + 7
    cut = 2 * G + 8
    table[cut:, 0] = rng.integers(0, B, cap - cut)               # trailing rows that only num_targets cuts off
    trimmed = table.copy()
    trimmed[cut:, 0] = -1
    for tab, n in ((trimmed, None), (table, torch.tensor(cut, dtype=torch.int64, device=DEV))):
        ids, got_ts, got_off, status = run_batched(tab, num_targets=n)
        st = status.cpu().numpy()
        assert st[0] == 0 and st[2] == G
        assert np.array_equal(got_off.cpu().numpy(), off) and int(got_off[B]) == G
        got_ts = got_ts.cpu().numpy()
        assert got_ts.shape == (cap, 7)
        assert np.array_equal(got_ts[:G].view(np.uint32), ts.view(np.uint32))
        assert not got_ts[G:].view(np.uint32).any()
        assert np.array_equal(ids.cpu().numpy(), want)


# ----------------------------------------------------------------------------- 3. real size
def test_real_size_against_per_image_op_and_oracle():
    from s2anet_amd import assign_labels_batched
    from s2anet_amd.rotated import assign_labels
    from test_gpu_loss import full_size_batch
    p, t = full_size_batch(B=2)
    init = torch.cat([a.reshape(-1, 5) for a in p[4]], 0)
    refine = torch.cat([a.reshape(2, -1, 5) for a in p[5]], 1)
    assert init.shape == (21824, 5)
    ids, ts, off, status = assign_labels_batched((init, refine), t, 2)
    st = status.cpu().numpy()
    assert st[0] == 0 and st[2] == 60
    tn = t.cpu().numpy()
    want_ts, want_off = sort_reference(tn, 2)
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), want_ts.view(np.uint32))
    assert np.array_equal(off.cpu().numpy(), want_off)
    got = ids.cpu().numpy()
    want = oracle_ids((init.cpu().numpy(), refine.cpu().numpy()), want_ts, want_off, (1024, 1024))
    assert np.array_equal(got, want)
    assert (got[0] >= 0).any() and (got[1] >= 0).any()
    for s, a in enumerate((init, refine)):
        for b in range(2):
            per = assign_labels(a if a.dim() == 2 else a[b], cu(want_ts[want_off[b]:want_off[b + 1], 2:7]))
            assert np.array_equal(got[s, b], per.cpu().numpy())


# ----------------------------------------------------------------------------- 4. overflow
def test_pair_list_overflow_is_reported_and_a_second_call_fits():
    """a handled condition: the cull counts every pair and writes only those below the capacity"""
    from s2anet_amd import _lib
    t, ts, off, want = case(0)
    grid, ref = pyramid()
    _, _, _, status = run_batched(t)
    found = int(status[1])                                       # the uncapped run
    assert found > 256 and int(status[0]) == 0
    # the C entry point on guarded buffers: a guard of 64 words behind every output
    S, A, G, cap, guard = 2, 1364, t.shape[0], 256, 64
    L = _lib.lib()
    sets = [cu(grid), cu(ref)]
    table = (_lib.AnchorSet * 2)()
    table[0].anchors, table[0].batch_stride = sets[0].data_ptr(), 0
    table[1].anchors, table[1].batch_stride = sets[1].data_ptr(), A * 5
    tg = cu(t)
    need = L.s2a_assign_labels_batched_workspace_bytes(S, B, A, G, cap)
    ids = torch.full((S * B * A + guard,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    sorted_t = torch.full((G * 7 + guard,), 12345.0, dtype=torch.float32, device=DEV)
    offsets = torch.full((B + 1 + guard,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    st = torch.full((4 + guard,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)
    ws = torch.full((need + guard,), 0xa5, dtype=torch.uint8, device=DEV)
    _lib.check(L.s2a_assign_labels_batched(table, S, B, A, _lib.ptr(tg), G, None, float(SIZE), float(SIZE), 0.5, 0.4, 0.0, 1, 1, 1,
                                           _lib.ptr(ids), _lib.ptr(sorted_t), _lib.ptr(offsets), _lib.ptr(st), cap,
                                           _lib.ptr(ws), need, _lib.stream_ptr(torch.device(DEV))))
    torch.cuda.synchronize()
    assert int(st[0]) & 1 and int(st[1]) == found and int(st[2]) == G
    assert bool((ids[S * B * A:] == 0x5a5a5a5a).all()) and bool((sorted_t[G * 7:] == 12345.0).all())
    assert bool((offsets[B + 1:] == 0x5a5a5a5a).all()) and bool((st[4:] == 0x5a5a5a5a).all())
    assert bool((ws[need:] == 0xa5).all())
    capped = ids[:S * B * A]
    assert bool(((capped >= -2) & (capped < max(COUNTS[0]))).all())                  # unspecified, but ids all the same
    # the capacity the first call asked for fits exactly
    ids2, _, _, status2 = run_batched(t, pair_capacity=found)
    assert int(status2[0]) == 0 and int(status2[1]) == found
    assert np.array_equal(ids2.cpu().numpy(), want)


# ----------------------------------------------------------------------------- 5. head
def test_head_routes_agree_bit_for_bit(monkeypatch):
    from test_gpu_loss import all_grads, golden_p, make_head
    g = golden("s2anet_loss.npz")
    head = make_head()
    for key in ("targets", "targets_case2"):
        targets = torch.from_numpy(g[key]).to(DEV)
        res = []
        for switch in (None, "0"):
            if switch is None:
                monkeypatch.delenv("S2A_ASSIGN_BATCHED", raising=False)
            else:
                monkeypatch.setenv("S2A_ASSIGN_BATCHED", switch)
            _, p = golden_p()
            loss, items = head.compute_loss(p, targets)
            assert isinstance(items, np.ndarray) and items.dtype == np.float32
            loss.backward()
            res.append((loss.detach().clone(), items, all_grads(p)))
        monkeypatch.delenv("S2A_ASSIGN_BATCHED", raising=False)
        (l1, i1, g1), (l0, i0, g0) = res
        assert torch.equal(l1, l0) and np.array_equal(i1, i0)
        assert len(g1) == 20 and all(torch.equal(a, b) for a, b in zip(g1, g0))
        _, p = golden_p()
        loss, items, status = head.compute_loss_device(p, targets)
        assert items.is_cuda and status.is_cuda and loss.is_cuda and loss.grad_fn is not None
        assert int(status[0]) == 0 and int(status[2]) == targets.shape[0]
        assert torch.equal(loss.detach(), l0) and np.array_equal(items.cpu().numpy(), i0)


def test_compute_loss_retries_when_the_pair_list_is_too_small(monkeypatch):
    """status bit 0 -> one more run at the capacity the first run reported, same result as the per-image route"""
    from s2anet_amd import rotated
    from test_gpu_loss import golden_p, make_head
    g = golden("s2anet_loss.npz")
    head = make_head()
    targets = torch.from_numpy(g["targets"]).to(DEV)
    _, p = golden_p()
    monkeypatch.setenv("S2A_ASSIGN_BATCHED", "0")
    l0, i0 = head.compute_loss(p, targets)
    monkeypatch.delenv("S2A_ASSIGN_BATCHED")
    monkeypatch.setattr(rotated, "ASSIGN_PAIR_CAPACITY", 16)
    _, _, status = head.compute_loss_device(p, targets)
    assert int(status[0]) == 1 and int(status[1]) > 16
    l1, i1 = head.compute_loss(p, targets)
    assert torch.equal(l1.detach(), l0.detach()) and np.array_equal(i1, i0)


# ----------------------------------------------------------------------------- 6. capture
def test_whole_loss_captured_and_replayed_against_new_targets(monkeypatch):
    from test_gpu_loss import full_size_batch, make_head
    head = make_head()
    head.imgs_size = (1024, 1024)
    p, t0 = full_size_batch(seed=2, B=2)
    maps = [x for lst in p[:4] for x in lst]
    table = torch.full((96, 7), -1.0, device=DEV)
    table[:60] = t0

    def step():
        loss, items, status = head.compute_loss_device(p, table)
        return (loss, items, status, *torch.autograd.grad(loss, maps))

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    monkeypatch.setenv("S2A_ASSIGN_BATCHED", "0")                # the eager comparator: the per-image route
    for seed, counts in ((3, (41, 17)), (4, (0, 55))):           # other targets, other per-image counts, then an empty image
        _, t = full_size_batch(seed=seed, B=2, n_gt=max(counts))
        t = torch.cat([t[t[:, 0] == b][:n] for b, n in enumerate(counts)])
        t = t[torch.randperm(t.shape[0], device=DEV)]
        new = torch.full((96, 7), -1.0, device=DEV)
        new[torch.randperm(96, device=DEV)[:t.shape[0]].sort()[0]] = t
        table.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        assert int(static[2][0]) == 0 and int(static[2][2]) == sum(counts)
        loss, items = head.compute_loss(p, t)
        grads = torch.autograd.grad(loss, maps)
        assert torch.equal(static[0], loss.detach()) and np.array_equal(static[1].cpu().numpy(), items)
        assert len(grads) == 20 and all(torch.equal(a, b) for a, b in zip(static[3:], grads))
        assert float(static[1][1]) > 0 and float(static[1][3]) > 0
