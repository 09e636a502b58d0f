"""The KEYS of the inference-side weight caches, without a GPU: since the head trains, a packed filter must follow every
route by which a parameter can change between two no-grad forwards.

The key logic is plain Python; only the packers launch kernels.  Here the packers are patched to copies
(conv_pack_weight, conv_wino_pack_weight, stem_pack_weight, alignconv.pack_weight, orn.arf_forward), so "the value the
cache returns" can be compared with "a fresh pack of the current tensor" by torch.equal:
  * PackedWeightCache.get / get_wino / get_bias (through FusedConv2d.packed_args / packed_args_wino),
    ORConv2d.rotate_arf + its packed forms, AlignConv.packed_weight, the stem's filter / bias of
    DetectorBackbone.forward_u8 -- every update route of ROUTES, weight only / bias only / both, four consecutive
    rounds per case on the same module
  * allocator address reuse, deterministically: torch.from_numpy on ONE numpy buffer gives a new tensor object at the
    same address with version 0 on every call -- "a temporary on every call" and "A -> B -> A across the direct and
    the Winograd slot"
  * `.data` in-place writes (no key can see them) are followed after s2anet_amd.drop_weight_caches
  * the caches stay plain attributes: state_dict() has the same entries before and after they are filled

ROUTES / TARGETS are shared with tests/test_gpu_weight_caches.py, which runs the same matrix through the real kernels.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


# ------------------------------------------------------------------------------------------------- update routes
def _new_like(p, gen):
    """new values in p's dtype / device / layout, of p's own scale (so that no f16 map overflows downstream)"""
    scale = float(p.detach().float().std()) if p.numel() > 1 else 1.0
    v = torch.randn(p.shape, generator=gen, dtype=torch.float32) * max(scale, 1e-2)
    out = torch.empty_like(p.detach())
    out.copy_(v)
    return out


def r_mul(owner, name, gen):
    with torch.no_grad():
        p = getattr(owner, name).mul_(1.25)
        if name == "bias":
            p.add_(1.0 / 64)                                # (a bias that is all zero would not notice the factor)


def r_add(owner, name, gen):
    p = getattr(owner, name)
    with torch.no_grad():
        p.add_(_new_like(p, gen) * 0.5)


def r_copy(owner, name, gen):
    p = getattr(owner, name)
    with torch.no_grad():
        p.copy_(_new_like(p, gen))


def _opt_step(make, owner, name, gen):
    p = getattr(owner, name)
    p.grad = _new_like(p, gen)
    opt = make([p])
    opt.step()
    p.grad = None


def r_sgd(owner, name, gen):
    _opt_step(lambda ps: torch.optim.SGD(ps, lr=0.5), owner, name, gen)


def r_adamw(owner, name, gen):
    p = getattr(owner, name)
    lr = 0.25 * max(float(p.detach().float().abs().mean()), 1e-2)       # Adam's first step is lr * sign(grad)
    eps = 1e-3 if p.dtype == torch.float16 else 1e-8                    # (the default eps is 0 in f16: 0 / 0 for a small grad)
    _opt_step(lambda ps: torch.optim.AdamW(ps, lr=lr, eps=eps, foreach=True), owner, name, gen)


def r_load(owner, name, gen):
    sd = {k: v.clone() for k, v in owner.state_dict().items()}
    sd[name] = _new_like(getattr(owner, name), gen)
    owner.load_state_dict(sd, strict=True)


def r_param(owner, name, gen):
    setattr(owner, name, nn.Parameter(_new_like(getattr(owner, name), gen)))


def r_data(owner, name, gen):
    p = getattr(owner, name)
    p.data = _new_like(p, gen)


def r_twice(owner, name, gen):
    """two replacements with no forward in between: the first one's storage is free again when the second is made"""
    r_data(owner, name, gen)
    r_data(owner, name, gen)
    r_param(owner, name, gen)
    r_param(owner, name, gen)


def r_dtype(owner, name, gen):
    """.float() -> change -> .half() (or the other way round for an f32 module)"""
    p = getattr(owner, name)
    if p.dtype == torch.float16:
        owner.float()
        r_add(owner, name, gen)
        owner.half()
    else:
        owner.half()
        r_add(owner, name, gen)
        owner.float()


ROUTES = {"a_mul": r_mul, "a_add": r_add, "a_copy": r_copy, "b_sgd": r_sgd, "b_adamw_foreach": r_adamw,
          "c_load_state_dict": r_load, "d_new_parameter": r_param, "d_data_assign": r_data, "d_twice_no_forward": r_twice,
          "e_float_change_half": r_dtype}
TARGETS = ("weight", "bias", "both")
ROUNDS = 4


def apply_route(route, owner, target, gen):
    names = ("weight", "bias") if target == "both" else (target,)
    for n in names:
        if getattr(owner, n, None) is not None:
            ROUTES[route](owner, n, gen)


def i_data_normal(owner, name, gen):
    getattr(owner, name).data.normal_(0, 0.05, generator=None)


def i_data_copy(owner, name, gen):
    p = getattr(owner, name)
    p.data.copy_(_new_like(p, gen))


DATA_ROUTES = {"i_data_normal_": i_data_normal, "i_data_copy_": i_data_copy}


# ------------------------------------------------------------------------------------------------- copying packers
@pytest.fixture
def copy_packers(monkeypatch):
    from s2anet_amd import alignconv, fused, orn
    monkeypatch.setattr(fused, "conv_pack_weight", lambda w: w.detach().clone())
    monkeypatch.setattr(fused, "conv_wino_pack_weight", lambda w: w.detach().clone() * 2)
    monkeypatch.setattr(fused, "stem_pack_weight", lambda w: w.detach().clone())
    monkeypatch.setattr(alignconv, "pack_weight", lambda w, dtype: w.detach().to(dtype).clone())
    monkeypatch.setattr(orn, "arf_forward", lambda w, idx: w.detach().flatten(1, 2).repeat(8, 1, 1, 1))
    # the stem kernel and the stages behind it: hand back the operands the launch would have got
    monkeypatch.setattr(fused, "stem_u8", lambda imgs, w, b, divisor=255.0: (w, b))


def pad_bias(b, width):
    v = b.detach().to(torch.float16)
    if v.numel() < width:
        v = torch.cat([v, v.new_zeros(width - v.numel())])
    return v


class Subject:
    """one cached module: owner of the parameters, the values its caches hand out, and fresh packs of the same"""

    def __init__(self, kind):
        from s2anet_amd.alignconv import AlignConv
        from s2anet_amd.detector import DetectorBackbone
        from s2anet_amd.fused import FusedConv2d
        from s2anet_amd.orn import ORConv2d
        self.kind = kind
        torch.manual_seed(5)
        if kind == "fused":
            self.mod = FusedConv2d(64, 64, 3, padding=1, relu=True)
            self.owner = self.mod
        elif kind == "fused_narrow":
            self.mod = FusedConv2d(64, 15, 1)
            self.owner = self.mod
        elif kind == "orconv":
            self.mod = ORConv2d(64, 8, 3, padding=1, arf_config=(1, 8))
            self.owner = self.mod
        elif kind == "align":
            self.mod = AlignConv(64, 64)
            self.owner = self.mod.deform_conv
        elif kind == "stem":
            self.mod = DetectorBackbone(layers=(1, 1, 1, 1))
            self.mod.backbone[0] = nn.Sequential(FusedConv2d(3, 64, 7, stride=2, padding=3, relu=True), nn.Identity())
            self.mod._stages = lambda x: x
            self.owner = self.mod.backbone[0][0]
        with torch.no_grad():
            if getattr(self.owner, "bias", None) is not None:
                self.owner.bias.normal_(0, 0.1)

    def cached(self):
        m = self.mod
        with torch.no_grad():
            if self.kind in ("fused", "fused_narrow"):
                w, b, _ = m.packed_args()
                out = {"direct": w, "bias": b}
                if m.wino_ok():
                    ww, bw, _ = m.packed_args_wino()
                    out.update(wino=ww, bias_wino=bw)
                return out
            if self.kind == "orconv":
                e = m.rotate_arf()
                c = m.packed_cache()
                return {"arf": e, "direct": c.get(e), "wino": c.get_wino(m.rotate_arf()),
                        "bias": c.get_bias(m.bias, e.shape[0])}
            if self.kind == "align":
                return {"f16": m.packed_weight(torch.float16), "f32": m.packed_weight(torch.float32)}
            w, b = m.forward_u8(None)
            return {"stem_w": w, "stem_b": b}

    def fresh(self):
        o = self.owner
        w = o.weight.detach()
        if self.kind in ("fused", "fused_narrow"):
            width = max(64, o.out_channels)
            out = {"direct": w.clone(), "bias": pad_bias(o.bias, width)}
            if o.wino_ok():
                out.update(wino=w * 2, bias_wino=pad_bias(o.bias, o.out_channels))
            return out
        if self.kind == "orconv":
            e = w.flatten(1, 2).repeat(8, 1, 1, 1)
            return {"arf": e, "direct": e, "wino": e * 2, "bias": pad_bias(o.bias, e.shape[0])}
        if self.kind == "align":
            return {"f16": w.to(torch.float16), "f32": w.to(torch.float32)}
        return {"stem_w": w.clone(), "stem_b": pad_bias(o.bias, 64)}

    def check(self, what):
        got, want = self.cached(), self.fresh()
        assert got.keys() == want.keys()
        for k in want:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), \
                f"stale cache: {self.kind}.{k} does not follow {what}"
        return got


KINDS = ("fused", "fused_narrow", "orconv", "align", "stem")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", KINDS)
def test_cached_value_follows_update_route(copy_packers, kind, route):
    """ROUNDS consecutive rounds of (update -> read the caches -> compare with a fresh pack) per target on ONE module"""
    s = Subject(kind)
    gen = torch.Generator().manual_seed(11)
    before = {k: v.clone() for k, v in s.check("construction").items()}
    for target in TARGETS:
        if target != "weight" and getattr(s.owner, "bias", None) is None:
            continue
        for r in range(ROUNDS):
            apply_route(route, s.owner, target, gen)
            now = s.check(f"route {route} on {target}, round {r}")
            assert any(not torch.equal(now[k].float(), before[k].float()) for k in now), "the update changed nothing"
            before = {k: v.clone() for k, v in now.items()}
            s.check("a second read with no update in between")


@pytest.mark.parametrize("kind", ("fused", "orconv", "stem"))
def test_bias_only_weight_only_and_both(copy_packers, kind):
    """the bias entry has a key of its own: it follows a bias-only update, and a weight-only update leaves the SAME
    cached bias object in place (and the other way round)"""
    s = Subject(kind)
    gen = torch.Generator().manual_seed(3)
    wk, bk = ("stem_w", "stem_b") if kind == "stem" else ("direct", "bias")
    for r in range(ROUNDS):
        a = s.check("construction")
        r_copy(s.owner, "bias", gen)
        b = s.check("a bias-only update")
        assert b[wk] is a[wk], "a bias-only update repacked the filter"
        r_copy(s.owner, "weight", gen)
        c = s.check("a weight-only update")
        assert c[bk] is b[bk], "a weight-only update rebuilt the bias"
        r_copy(s.owner, "weight", gen)
        r_copy(s.owner, "bias", gen)
        d = s.check("an update of both")
        assert d[wk] is not c[wk] and not torch.equal(d[bk], c[bk])


def test_temporary_at_a_recycled_address_each_call(copy_packers):
    """the CPU stand-in for a caching allocator that hands a freed block out again: a NEW tensor object at the SAME
    address with version 0 and other contents on every call"""
    from s2anet_amd.fused import PackedWeightCache
    c = PackedWeightCache()
    wbuf = np.zeros((64, 64, 3, 3), np.float32)
    bbuf = np.zeros((64,), np.float32)
    addr = None
    for i in range(1, 6):
        wbuf[...] = i
        bbuf[...] = -i
        for get, buf, want in ((c.get, wbuf, float(i)), (c.get_wino, wbuf, 2.0 * i)):
            t = torch.from_numpy(buf)
            assert t._version == 0 and (addr is None or t.data_ptr() == addr)
            addr = t.data_ptr()
            got = get(t)
            del t
            assert float(got.min()) == float(got.max()) == want, f"stale cache: call {i} got the pack of call {got.max()}"
        b = torch.from_numpy(bbuf)
        assert b._version == 0
        gb = c.get_bias(b, 64)
        del b
        assert float(gb.float().min()) == float(gb.float().max()) == -i, "stale cache: bias of an earlier temporary"


def test_address_reuse_a_b_a_across_the_direct_and_winograd_slots(copy_packers):
    """S2A_CONV_WINO switched between updates: expansion A packed for the direct slot, B for the Winograd slot, then a
    third one at A's address for the direct slot again -- every call must see its own contents"""
    from s2anet_amd.fused import PackedWeightCache
    c = PackedWeightCache()
    bufs = [np.zeros((64, 64, 3, 3), np.float32), np.zeros((64, 64, 3, 3), np.float32)]
    val = 0.0
    for r in range(ROUNDS):
        for slot, (get, scale) in enumerate(((c.get, 1.0), (c.get_wino, 2.0))):
            val += 1.0
            bufs[slot][...] = val                      # "the optimizer step": new contents, same address, version 0
            t = torch.from_numpy(bufs[slot])
            got = get(t)
            del t
            assert float(got.min()) == float(got.max()) == scale * val, \
                f"stale cache: round {r}, {'wino' if slot else 'direct'} slot returned {float(got.max())}"
    # and the other diagonal: the buffer that fed the Winograd slot now feeds the direct one
    for slot, (get, scale) in enumerate(((c.get_wino, 2.0), (c.get, 1.0))):
        val += 1.0
        bufs[slot][...] = val
        t = torch.from_numpy(bufs[slot])
        got = get(t)
        del t
        assert float(got.max()) == scale * val, "stale cache: slots swapped"


def test_orconv_expansion_is_cached_in_train_mode_under_no_grad_and_follows_updates(copy_packers):
    """S2ANetHead() is born in train mode; under no_grad the expansion handed to the packed-filter cache must be the
    cached one (keyed on the 5-D parameter), not a fresh temporary, in train() as in eval(), and across toggles"""
    s = Subject("orconv")
    gen = torch.Generator().manual_seed(1)
    oc = s.mod
    for r in range(2 * ROUNDS):
        oc.train(r % 2 == 0)
        with torch.no_grad():
            a = oc.rotate_arf()
            assert oc.rotate_arf() is a, f"training={oc.training}: a temporary was handed out under no_grad"
            pa = oc.packed_cache().get(a)
            assert oc.packed_cache().get(oc.rotate_arf()) is pa
        ROUTES[list(ROUTES)[r % len(ROUTES)]](oc, "weight", gen)
        s.check(f"an update in round {r} (training={oc.training})")
        with torch.no_grad():
            assert oc.rotate_arf() is not a
    oc.channels_last = True                                 # the layout flag is part of the expansion's key
    with torch.no_grad():
        e = oc.rotate_arf()
    assert e.is_contiguous(memory_format=torch.channels_last) and not e.is_contiguous()


@pytest.mark.parametrize("kind", KINDS)
def test_deepcopy_of_a_warm_module_follows_its_own_parameters(copy_packers, kind):
    s = Subject(kind)
    gen = torch.Generator().manual_seed(2)
    warm = {k: v.clone() for k, v in s.check("construction").items()}
    t = copy.copy(s)
    t.mod = copy.deepcopy(s.mod)
    if kind == "stem":
        t.mod._stages = lambda x: x
    t.owner = {"align": lambda m: m.deform_conv, "stem": lambda m: m.backbone[0][0]}.get(kind, lambda m: m)(t.mod)
    assert t.owner.weight is not s.owner.weight
    for r in range(ROUNDS):
        for target in TARGETS:
            apply_route("a_copy" if r % 2 else "d_data_assign", t.owner, target, gen)
            t.check(f"an update of the copy ({target}, round {r})")
            got = s.check("an update of its deep copy")
            assert all(torch.equal(got[k], warm[k]) for k in warm), "the original changed with its copy"


@pytest.mark.parametrize("route", list(DATA_ROUTES))
@pytest.mark.parametrize("kind", KINDS)
def test_data_inplace_write_needs_drop_weight_caches(copy_packers, kind, route):
    """`.data` in-place writes bump no version counter and move no storage: drop_weight_caches is the documented way"""
    import s2anet_amd
    s = Subject(kind)
    gen = torch.Generator().manual_seed(4)
    for r in range(ROUNDS):
        for target in TARGETS:
            s.check("the previous round")
            v = s.owner.weight._version
            for n in (("weight", "bias") if target == "both" else (target,)):
                if getattr(s.owner, n, None) is not None:
                    DATA_ROUTES[route](s.owner, n, gen)
            assert s.owner.weight._version == v, "this torch bumps the version on .data writes: the route is visible"
            assert s2anet_amd.drop_weight_caches(s.mod) is s.mod
            s.check(f"{route} on {target} followed by drop_weight_caches, round {r}")


def test_drop_weight_caches_reaches_every_cache_of_a_module_tree(copy_packers):
    import s2anet_amd
    subs = [Subject(k) for k in KINDS]
    tree = nn.ModuleList(s.mod for s in subs)
    olds = [s.check("construction") for s in subs]
    for s in subs:
        s.owner.weight.data.mul_(3.0)
        if getattr(s.owner, "bias", None) is not None:
            s.owner.bias.data.add_(1.0)
    s2anet_amd.drop_weight_caches(tree)
    for s, old in zip(subs, olds):
        new = s.check(".data writes + drop_weight_caches on the parent tree")
        for k in new:
            assert new[k] is not old[k], f"{s.kind}.{k} survived drop_weight_caches"


def test_caches_are_plain_attributes_state_dict_is_unchanged(copy_packers):
    """a reference checkpoint must keep loading strictly after the caches were filled"""
    from s2anet_amd.detector import fuse_epilogues
    from s2anet_amd.fused import FusedConv2d
    from s2anet_amd.head import S2ANetHead
    torch.manual_seed(0)
    head = fuse_epilogues(S2ANetHead(15, in_channels=64, feat_channels=64))
    stem = Subject("stem")
    tree = nn.ModuleDict({"head": head, "trunk": stem.mod})
    before = {k: v.clone() for k, v in tree.state_dict().items()}
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, FusedConv2d):
                m.packed_args()
                if m.wino_ok():
                    m.packed_args_wino()
        e = head.or_conv.rotate_arf()
        head.or_conv.packed_cache().get(e)
        head.or_conv.packed_cache().get_wino(e)
        head.or_conv.packed_cache().get_bias(head.or_conv.bias, e.shape[0])
        head.align_conv.packed_weight(torch.float16)
        stem.cached()
    after = tree.state_dict()
    assert list(after.keys()) == list(before.keys())
    assert all(torch.equal(after[k], before[k]) for k in before)
    tree.load_state_dict(before, strict=True)
    twin = nn.ModuleDict({"head": fuse_epilogues(S2ANetHead(15, in_channels=64, feat_channels=64)),
                          "trunk": Subject("stem").mod})
    twin.load_state_dict(copy.deepcopy(tree).state_dict(), strict=True)
