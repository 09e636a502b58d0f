"""The training BatchNorm kernels (s2anet_amd/csrc/bn_ops.hip) at slice-edge geometries against float64: the five s2a_bn_*
entry points through the C ABI, each ALONE on given inputs -- apply gets the float64 statistics rounded to f32, not the stats
kernel's; backward_input gets float64's coefficients, not backward_reduce's -- per channel and per element, under the bounds of
tests/bn_geometry_cases.py (case table, inputs, references, bounds; tests/test_bn_geometry_cpu.py checks those without a GPU).

Buffers: every input is a view into a NaN-filled buffer with 64 KiB of NaN on each side, so a read outside a tensor comes back
as a NaN; every output and both `partial`s are views into byte buffers with 64 KiB of fill on each side and are launched into
twice, over 0xFF (NaN in every float format) and over 0xA5: the two launches give the same bits (no byte kept its fill), the
bands keep theirs, and finite inputs give no NaN.

What each entry point is held to is stated in tests/bn_geometry_cases.py; in short
  stats           mean and invstd per channel; running statistics in f32, in f16 and as the NULL pair; momentum 0 leaves the
                  bits, momentum 1 stores the bits of `mean` and M2 / (P - 1)
  apply           per element, {residual, none} x {ReLU, none} x {f32, f16 parameters}
  backward_reduce sum g and sum g / P EQUAL float64's (the cotangent is dyadic: one row dropped, doubled or misplaced shows at
                  any P); sum g xhat under its bound; the masked gradient bit for bit, over +-0, subnormals and NaN outputs;
                  every call form, the two refused ones included
  backward_input  per element, with and without the mask re-applied
  the chain       the four passes as production chains them, the statistics' bound propagated to first order
  non-finite x    in the unrolled walk: a lane's first row, the second row of a trip, a tail row

Set S2A_BN_GEOMETRY_REPORT=<path> to write every measured ratio (error over bound), one per (test, tensor, case), as JSON when
the file has run; the committed run is
profiles/bn_geometry_ratios.json."""
import json
import math
import os

import pytest
import torch

import bn_geometry_cases as G
from conv_geometry_cases import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32, F64 = torch.float16, torch.float32, torch.float64
NAME = {F32: "f32", F16: "f16", None: "none"}
REPORT = {}                       # "test | tensor" -> {case id: worst ratio}
FILLS = (0xFF, 0xA5)


def record(test, d, tensor, ratio):
    row = REPORT.setdefault("%s | %s" % (test, tensor), {})
    row[d["c"]["id"]] = max(ratio, row.get(d["c"]["id"], 0.0))
    print("%-34s %-26s %-14s ratio %.3f" % (test, d["c"]["id"], tensor, ratio))
    return [] if ratio <= 1.0 else ["%s: %s is %.3f bounds off" % (test, tensor, ratio)]


def write_report(path):
    """one ratio per (test, tensor, case): "cases" names the columns, every other key is "test | tensor" with one ratio per
    case in that order (null: the test does not run the case), a line each"""
    ids = [c["id"] for c in G.CASES]
    lines = ['"cases": ' + json.dumps(ids)]
    for key in sorted(REPORT):
        lines.append(json.dumps(key) + ": " + json.dumps([None if i not in REPORT[key] else round(REPORT[key][i], 3) for i in ids],
                                                         separators=(",", ":")))
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    if os.environ.get("S2A_BN_GEOMETRY_REPORT"):
        write_report(os.environ["S2A_BN_GEOMETRY_REPORT"])


# ----------------------------------------------------------------------------- buffers
def vec(t):
    """a per-channel input as a view into a NaN-filled buffer of its own dtype, 64 KiB of NaN on each side"""
    pad = G.GUARD_BYTES // t.element_size()
    buf = torch.full((2 * pad + t.numel(),), math.nan, dtype=t.dtype, device=DEV)
    v = buf[pad:pad + t.numel()]
    assert v.data_ptr() % 16 == 0
    v.copy_(t)
    return v


class Outputs:
    """outputs as views into byte buffers pre-filled with one byte, 64 KiB of it on each side of every view"""

    def __init__(self, fill):
        self.fill, self.bufs = fill, {}

    def new(self, name, shape, dtype, init=None):
        n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        whole = torch.full((2 * G.GUARD_BYTES + n,), self.fill, dtype=torch.uint8, device=DEV)
        view = whole[G.GUARD_BYTES:G.GUARD_BYTES + n].view(dtype).view(shape)
        assert view.data_ptr() % 16 == 0
        if init is not None:
            view.copy_(init)
        self.bufs[name] = (whole, n, view)
        return view

    def untouched(self, name):
        return bool((self.bufs[name][0] == self.fill).all())

    def done(self):
        torch.cuda.synchronize()
        for name, (whole, n, _) in self.bufs.items():
            assert bool((whole[:G.GUARD_BYTES] == self.fill).all()) and bool((whole[G.GUARD_BYTES + n:] == self.fill).all()), \
                "%s: a byte of its bands was written" % name
        return {k: v[2] for k, v in self.bufs.items()}


def bits(t):
    return t.contiguous().view(torch.uint8)


def twice(launch, finite=True):
    """launch(Outputs) over both fills -> the outputs, equal bit for bit, bands intact, no NaN"""
    runs = []
    for fill in FILLS:
        o = Outputs(fill)
        launch(o)
        runs.append(o.done())
    a, b = runs
    assert set(a) == set(b) and a
    for k in a:
        assert torch.equal(bits(a[k]), bits(b[k])), "%s: a byte kept its fill, or two launches differ" % k
        if finite:
            assert not bool(torch.isnan(a[k]).any()), "%s holds a NaN" % k
    return a


# ----------------------------------------------------------------------------- a case on the device
def load(c, x=None):
    from s2anet_amd import _lib
    inp = G.make_inputs(c)
    if x is not None:
        inp["x"] = x(inp["x"])
    P, C = c["P"], c["C"]
    d = dict(c=c, P=P, C=C, pl=G.plan(P, C), n=_lib.lib().s2a_bn_slices(P, C), edge=inp["edge"].to(DEV))
    assert d["n"] == d["pl"]["slices"]
    for k in ("x", "g", "r", "y"):
        d[k] = Guarded(inp[k], DEV).t
    d["st"] = G.stats64(d["x"])
    mean, invstd = G.given_stats(d["st"])
    d["mean"], d["invstd"] = vec(mean), vec(invstd)
    d["gamma"] = {t: vec(inp["gamma"].to(t)) for t in (F32, F16)}
    d["beta"] = {t: vec(inp["beta"].to(t)) for t in (F32, F16)}
    d["running_mean"], d["running_var"] = inp["running_mean"].to(DEV), inp["running_var"].to(DEV)
    return d


@pytest.fixture(scope="module", params=G.CASES, ids=lambda c: c["id"])
def dev(request):
    return load(request.param)


def call(name, *args):
    from s2anet_amd import _lib
    L = _lib.lib()
    _lib.check(getattr(L, name)(*[_lib.ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], _lib.stream_ptr(DEV)))


def code(dtype):
    from s2anet_amd import _lib
    return _lib.DTYPE_F16 if dtype == F16 else _lib.DTYPE_F32


# ----------------------------------------------------------------------------- the launches
def launch_stats(d, o, rdtype, momentum, eps=G.EPS):
    n, C = d["n"], d["C"]
    partial, mean, invstd = o.new("partial", (n, 2, C), F32), o.new("mean", (C,), F32), o.new("invstd", (C,), F32)
    rm = rv = None
    if rdtype is not None:
        rm = o.new("running_mean", (C,), rdtype, d["running_mean"])
        rv = o.new("running_var", (C,), rdtype, d["running_var"])
    call("s2a_bn_train_stats_f16", d["x"], d["P"], C, eps, momentum, partial, n, mean, invstd, rm, rv, code(rdtype))


def launch_apply(d, o, mean, invstd, pdtype, res, relu):
    out = o.new("out", (d["P"], d["C"]), F16)
    call("s2a_bn_train_apply_f16", d["x"], mean, invstd, d["gamma"][pdtype], d["beta"][pdtype], code(pdtype),
         d["r"] if res else None, out, d["P"], d["C"], int(relu))


def launch_reduce(d, o, go, y, mean, invstd, pdtype, want_g, sums=True):
    P, C, n = d["P"], d["C"], d["n"]
    g = o.new("g", (P, C), F16) if want_g else None
    if not sums:
        call("s2a_bn_backward_reduce_f16", go, None, y, None, None, g, None, 0, None, None, code(pdtype), None, P, C)
        return
    partial, coef = o.new("partial", (n, 2, C), F32), o.new("coef", (2, C), F32)
    gw, gb = o.new("grad_weight", (C,), pdtype), o.new("grad_bias", (C,), pdtype)
    call("s2a_bn_backward_reduce_f16", go, d["x"], y, mean, invstd, g, partial, n, gw, gb, code(pdtype), coef, P, C)


def launch_input(d, o, go, y, mean, invstd, pdtype, coef):
    gx = o.new("grad_input", (d["P"], d["C"]), F16)
    call("s2a_bn_backward_input_f16", go, d["x"], y, mean, invstd, d["gamma"][pdtype], code(pdtype), coef, gx, d["P"], d["C"])


# ----------------------------------------------------------------------------- 1. statistics
def check_stats(test, d, got, eps=G.EPS):
    bad = record(test, d, "mean", G.compare_mean(got["mean"], d["st"]))
    bad += record(test, d, "invstd", G.compare_invstd(got["invstd"], d["st"], eps))
    used = G.used_slices(d["pl"])
    if not bool((got["partial"][used:] == 0).all()):
        bad.append("an empty slice's partial is not the identity")
    return bad


def test_stats_without_running_statistics(dev):
    got = twice(lambda o: launch_stats(dev, o, None, 0.1))
    assert set(got) == {"partial", "mean", "invstd"}
    bad = check_stats("stats/none", dev, got)
    assert not bad, bad


@pytest.mark.parametrize("rdtype", [F32, F16], ids=["f32", "f16"])
def test_running_statistics(dev, rdtype):
    """momentum 0.1 inside the bound; 0 leaves the bits; 1 stores the bits of `mean` (f16: a nearest f16 of it) and
    M2 / (P - 1) inside the variance's bound"""
    d, tag = dev, "stats/" + NAME[rdtype]
    before = (d["running_mean"].to(rdtype), d["running_var"].to(rdtype))
    bad, means = [], []
    for momentum in (0.1, 0.0, 1.0):
        got = twice(lambda o: launch_stats(d, o, rdtype, momentum))
        means.append((got["mean"], got["invstd"], got["partial"]))
        if momentum == 0.0:
            assert torch.equal(bits(got["running_mean"]), bits(before[0])) and torch.equal(bits(got["running_var"]), bits(before[1]))
            continue
        (rm, bm), (rv, bv) = G.running64(d["st"], before[0], before[1], momentum)
        t = "%s/m%g" % (tag, momentum)
        bad += record(t, d, "running_mean", G._ratio((got["running_mean"].to(F64) - rm).abs(), bm))
        bad += record(t, d, "running_var", G._ratio((got["running_var"].to(F64) - rv).abs(), bv))
        if momentum == 1.0:
            # f32: the bits of `mean`.  f16: a nearest f16 of `mean` -- the source writes (f16)(f32)value, but under hipcc's default
            # contraction the binary rounds the double ONCE (no f64 -> f32 convert in k_bn_stats_final<f16>), so where the f32
            # mean is exactly a tie of two f16 values the double's remaining bits decide, not the even one
            near = got["mean"].to(rdtype)
            off = (got["running_mean"].float() - got["mean"]).abs() > (near.float() - got["mean"]).abs()
            if rdtype == F32:
                off = (bits(got["running_mean"]) != bits(got["mean"])).view(-1, 4).any(1)
            assert not bool(off.any()), "running_mean is not mean's bits: " + "; ".join(
                "c %d mean %s -> %r, stored %r" % (c, float(got["mean"][c]).hex(), float(near[c]), float(got["running_mean"][c]))
                for c in off.nonzero().flatten()[:4].tolist())
    bad += check_stats(tag, d, dict(zip(("mean", "invstd", "partial"), means[0])))
    for m in means[1:]:                                       # the statistics do not know the momentum
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(means[0], m))
    assert not bad, bad


def test_stats_with_eps_zero():
    c = G.case_of("unrolled-31", 320)
    assert c["family"] != "constant"
    d = load(c)
    got = twice(lambda o: launch_stats(d, o, F32, 0.1, eps=0.0))
    bad = check_stats("stats/eps0", d, got, eps=0.0)
    assert not bad, bad


# ----------------------------------------------------------------------------- 2. apply
@pytest.mark.parametrize("pdtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("res", [True, False], ids=["res", "nores"])
def test_apply_on_given_statistics(dev, res, relu, pdtype):
    d = dev
    got = twice(lambda o: launch_apply(d, o, d["mean"], d["invstd"], pdtype, res, relu))
    ref, S = G.apply64(d["x"], d["mean"], d["invstd"], d["gamma"][pdtype], d["beta"][pdtype], d["r"] if res else None, relu)
    test = "apply/%s%s/%s" % ("res" if res else "nores", "+relu" if relu else "", NAME[pdtype])
    bad = record(test, d, "out", G.compare_elementwise(got["out"], ref, S, G.K_A))
    if relu:
        assert bool((got["out"] >= 0).all())
    assert not bad, bad


def test_apply_relu_keeps_a_nan():
    d = load(G.case_of("unrolled-1", 64))
    rows = [int(d["edge"][3]), 1234]
    clean = twice(lambda o: launch_apply(d, o, d["mean"], d["invstd"], F32, True, True))["out"]

    def plant(x):
        x = x.clone()
        for i, r in enumerate(rows):
            x[r, 9 + i] = math.nan
        return x
    d2 = load(d["c"], x=plant)
    got = twice(lambda o: launch_apply(d2, o, d["mean"], d["invstd"], F32, True, True), finite=False)["out"]
    want = torch.zeros_like(got, dtype=torch.bool)
    for i, r in enumerate(rows):
        want[r, 9 + i] = True
    assert torch.equal(got.isnan(), want)
    assert torch.equal(got[~want], clean[~want])


# ----------------------------------------------------------------------------- 3. backward: reduce
REDUCE_FORMS = [("sums+g", F32), ("sums+g", F16), ("sums_masked", F32), ("sums_masked", F16), ("sums", F32), ("sums", F16),
                ("mask", F32)]


@pytest.mark.parametrize("form,pdtype", REDUCE_FORMS, ids=["%s-%s" % (f, NAME[t]) for f, t in REDUCE_FORMS])
def test_backward_reduce_on_given_statistics(dev, form, pdtype):
    d, P, C = dev, dev["P"], dev["C"]
    y = None if form == "sums" else d["y"]
    want_g = form in ("sums+g", "mask")
    got = twice(lambda o: launch_reduce(d, o, d["g"], y, d["mean"], d["invstd"], pdtype, want_g, sums=form != "mask"))
    gm = G.masked(d["g"], y)
    test = "reduce/%s/%s" % (form, NAME[pdtype])
    if want_g:
        assert torch.equal(bits(got["g"]), bits(gm)), "the masked gradient differs from where(out <= 0, 0, grad_out)"
        hit = d["y"][d["edge"]]
        if hit.numel() >= 7:                                  # the mask met +-0, both subnormals and a NaN
            assert bool(hit.isnan().any()) and bool((hit == 0).any()) and bool(((hit != 0) & (hit.float().abs() < 1e-7)).any())
    if form == "mask":
        assert set(got) == {"g"}
        return
    assert set(got) == {"partial", "coef", "grad_weight", "grad_bias"} | ({"g"} if want_g else set())
    red = G.reduce64(gm, d["x"], d["mean"], d["invstd"])
    assert torch.equal(got["grad_bias"], red["sg"].to(pdtype)), "grad_bias is not float64's sum rounded once"
    assert torch.equal(got["coef"][0], (red["sg"] / P).to(F32)), "coef[0:C] is not float64's sum / P rounded once"
    bad = record(test, d, "grad_weight", G.compare_sum(got["grad_weight"], red["sgx"], red["l1"], pdtype))
    bad += record(test, d, "coef[C:2C]", G.compare_sum(got["coef"][1], red["sgx"], red["l1"], F32, over=P))
    if not bool((got["partial"][G.used_slices(d["pl"]):] == 0).all()):
        bad.append("an empty slice's partial is not zero")
    assert not bad, bad


def test_backward_reduce_refused_forms_touch_nothing():
    from s2anet_amd import _lib
    L = _lib.lib()
    d = load(G.case_of("few_rows", 320))
    P, C, n = d["P"], d["C"], d["n"]
    ptr, st = _lib.ptr, _lib.stream_ptr(DEV)
    for fill in FILLS:
        o = Outputs(fill)
        g, partial, coef = o.new("g", (P, C), F16), o.new("partial", (n, 2, C), F32), o.new("coef", (2, C), F32)
        gw, gb = o.new("grad_weight", (C,), F32), o.new("grad_bias", (C,), F32)
        rc = L.s2a_bn_backward_reduce_f16(ptr(d["g"]), ptr(d["x"]), None, ptr(d["mean"]), ptr(d["invstd"]), ptr(g), ptr(partial), n,
                                          ptr(gw), ptr(gb), 0, ptr(coef), P, C, st)
        assert rc == _lib.EINVAL and "needs the forward output" in L.s2a_last_error().decode()      # g without out
        rc = L.s2a_bn_backward_reduce_f16(ptr(d["g"]), ptr(d["x"]), ptr(d["y"]), ptr(d["mean"]), ptr(d["invstd"]), None, None, n,
                                          None, None, 0, None, P, C, st)
        assert rc == _lib.EINVAL and "nothing to write" in L.s2a_last_error().decode()              # neither partial nor g
        o.done()
        assert all(o.untouched(k) for k in o.bufs)


# ----------------------------------------------------------------------------- 4. backward: input
@pytest.mark.parametrize("pdtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("with_out", [False, True], ids=["plain", "masked"])
def test_backward_input_on_given_coefficients(dev, with_out, pdtype):
    d = dev
    y = d["y"] if with_out else None
    gm = G.masked(d["g"], y)
    coef = vec(G.given_coef(G.reduce64(gm, d["x"], d["mean"], d["invstd"]), d["P"]))
    got = twice(lambda o: launch_input(d, o, d["g"], y, d["mean"], d["invstd"], pdtype, coef))
    ref, S = G.input64(gm, d["x"], d["mean"], d["invstd"], d["gamma"][pdtype], coef)
    test = "input/%s/%s" % ("masked" if with_out else "plain", NAME[pdtype])
    bad = record(test, d, "grad_input", G.compare_elementwise(got["grad_input"], ref, S, G.K_I))
    assert not bad, bad


# ----------------------------------------------------------------------------- 5. the chain
@pytest.mark.parametrize("why,C", G.CHAIN_CASES, ids=["%s-C%d" % wc for wc in G.CHAIN_CASES])
def test_the_four_passes_chained(why, C):
    """statistics -> apply (+ residual, ReLU) -> reduce behind the mask of that output -> input, each on the pass before's own
    results, as s2anet_amd/norm.py chains them; out and grad_input per element with the statistics' bound carried along"""
    d = load(G.case_of(why, C))
    P = d["P"]

    def launch(o):
        launch_stats(d, o, F32, 0.1)
        v = {k: b[2] for k, b in o.bufs.items()}
        launch_apply(d, o, v["mean"], v["invstd"], F32, True, True)
        out = o.bufs["out"][2]
        partial = o.bufs.pop("partial")
        launch_reduce(d, o, d["g"], out, v["mean"], v["invstd"], F32, True)
        o.bufs["partial_stats"] = partial
        launch_input(d, o, o.bufs["g"][2], None, v["mean"], v["invstd"], F32, o.bufs["coef"][2])
    got = twice(launch)
    assert len(got) == 12
    gm = G.masked(d["g"], got["out"])
    assert torch.equal(bits(got["g"]), bits(gm))
    ref = G.chain64(d["x"], d["r"], gm, d["gamma"][F32], d["beta"][F32], d["st"], G.EPS)
    test = "chain"
    bad = record(test, d, "out", G.compare_within(got["out"], ref["out"], ref["out_scale"]))
    bad += record(test, d, "grad_input", G.compare_within(got["grad_input"], ref["dx"], ref["dx_scale"]))
    bad += record(test, d, "mean", G.compare_mean(got["mean"], d["st"]))
    bad += record(test, d, "invstd", G.compare_invstd(got["invstd"], d["st"], G.EPS))
    assert torch.equal(got["grad_bias"], ref["sg"].to(F32)) and torch.equal(got["coef"][0], (ref["sg"] / P).to(F32))
    assert not bad, bad


# ----------------------------------------------------------------------------- 6. non-finite values in the unrolled walk
@pytest.mark.parametrize("value", [math.inf, -math.inf, math.nan], ids=["inf", "-inf", "nan"])
def test_non_finite_value_in_the_unrolled_walk(value):
    """one +-inf or NaN in one channel at a lane's first row (LaneAcc::start takes K = 0), at the second row of a trip and at
    a tail row: mean and invstd of that channel have float64's class, every other channel keeps the clean run's bits"""
    c = G.case_of("unrolled-1", 64)
    pl = G.plan(c["P"], c["C"])
    assert pl["rps"] == 160
    r0, r1 = G.slice_rows(pl, 3)
    assert G.lane_walk(r0, r1, 5) == (r0 + 5, [r0 + 37], [])
    l0, l1 = G.slice_rows(pl, G.used_slices(pl) - 1)
    first, trips, tail = G.lane_walk(l0, l1, 31)
    assert not trips and len(tail) == 3                        # the last lane of the ragged slice walks its rows in the tail
    spots = {"first": (r0 + 5, 7), "trip": (r0 + 5 + 64, 21), "tail": (tail[0], 40)}
    clean_d = load(c)
    clean = twice(lambda o: launch_stats(clean_d, o, F32, 0.1))
    for name, (row, ch) in spots.items():
        def plant(x):
            x = x.clone()
            x[row, ch] = value
            return x
        d = load(c, x=plant)
        got = twice(lambda o: launch_stats(d, o, F32, 0.1), finite=False)
        st = d["st"]
        want_invstd = 1.0 / torch.sqrt(st["var"] + G.EPS)
        assert not bool(torch.isfinite(st["mean"][ch])) and bool(want_invstd[ch].isnan())
        assert torch.equal(G.classes(got["mean"]), G.classes(st["mean"])), name
        assert torch.equal(G.classes(got["invstd"]), G.classes(want_invstd)), name
        keep = [i for i in range(c["C"]) if i != ch]
        for k in ("mean", "invstd", "running_mean", "running_var"):
            assert torch.equal(bits(got[k][keep]), bits(clean[k][keep])), (name, k)
        assert not bool(torch.isfinite(got["running_var"][ch])) and not bool(torch.isfinite(got["running_mean"][ch]))
