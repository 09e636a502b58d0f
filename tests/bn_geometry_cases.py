"""The training BatchNorm case table (s2anet_amd/csrc/bn_ops.hip, bn_plan.hpp), its inputs, the float64 references, the bounds
and the comparators shared by tests/test_bn_geometry_cpu.py (which checks the table, the inputs, the references and the bounds
without a GPU) and tests/test_gpu_bn_geometry.py (which holds the five s2a_bn_* entry points to them on guarded buffers).

Nothing here is imported from the library.  plan(), slice_rows(), lane_rows() and the restate_*() functions are the tests' own
statement of bn_plan.hpp, as route() is in tests/conv_geometry_cases.py: the slice plan, and in f32 the arithmetic ORDER of the
kernels -- a lane's sums around its first value, the merge of 32 lanes, sixteen final lanes each merging every sixteenth
slice.  The restatement is never compared with a kernel (the kernels contract s2 += d * d into an FMA, it does not); it is
measured against float64 and fixes the constants of the bounds: each K below is twice the worst ratio the restatement
reaches over the whole table, rounded up to an integer (the rule of oracle/glue64.py).  tests/test_bn_geometry_cpu.py measures
the ratios again and asserts each stays under K / 2.

Bounds.  u32 = 2^-24, u16 = 2^-11; every reference is float64 from the same f16 / parameter bits.
  statistics, per channel:
      |mean - mean64| <= K_M u32 (|mean64| + max_r |x - mean64|)
      the variance the kernel divides by, var, obeys |var - var64| <= K_V u32 var64 (a constant channel: exactly 0); it is
      judged through the one number the kernel hands on, invstd = rnd32(1 / sqrt(var + eps)):
      |invstd - f(var64)| <= max |f(var64 (1 +- K_V u32)) - f(var64)| + u32 f(var64 (1 - K_V u32)),   f(v) = 1 / sqrt(v + eps)
      running statistics, r' = (1 - m) r + m s:  |r' - r'64| <= b + rnd(|r'64| + b), b = m * (the bound of s), and rnd the
      roundings of the store: u32 for f32; for f16 the kernel stores (f16)(f32)value, two roundings: u16 + 2 u32, and 2^-25
      absolute where the f16 is subnormal
  apply, per element, mean and invstd GIVEN (f32):  S = |(x - mean) invstd gamma| + |beta| + |r|,  t = K_A u32 S,
      |out - y64| <= t + u16 (|y64| + t) + 2^-25                    (an f32 error of a few operations, then one f16 rounding)
  backward reduce:  sum g and sum g / P EQUAL float64's rounded once (the cotangent is dyadic, see make_inputs);
      |sum g xhat - ref| <= K_W u32 sum |g xhat| + rnd(|ref| + that) (rnd as above), the coefficient the same over P
  backward input, per element, coef / mean / invstd GIVEN:  S = |a| (|g| + |k1| + |xhat k2|), a = invstd gamma, t = K_I u32 S,
      |dx - dx64| <= t + u16 (|dx64| + t) + 2^-25
"""
import math
import zlib

import torch

F16, F32, F64 = torch.float16, torch.float32, torch.float64
U16, U32 = 2.0 ** -11, 2.0 ** -24
TINY = 2.0 ** -25                 # half an f16 subnormal step
GUARD_BYTES = 65536               # fill on each side of a guarded output
EPS = 1e-5
SUBNORMAL = 2.0 ** -24            # the smallest f16 subnormal

# the constants of the bounds: ceil(2 * worst ratio of the restatement over CASES); measured by
# tests/test_bn_geometry_cpu.py::test_restatement_stays_under_half_of_every_constant, which prints the ratios
K_M, K_V, K_A, K_W, K_I = 2, 7, 8, 10, 10
SEPARATION = 4.0                  # an edge row left out or counted twice moves mean or variance by this many bounds

# ----------------------------------------------------------------------------- the plan (bn_plan.hpp, restated)
ROW_LANES, GROUP, MAX_SLICES, BLOCKS_AIM, FINAL_LANES = 32, 64, 256, 1024, 16


def plan(P, C):
    groups = C // GROUP
    slices = max(1, min(MAX_SLICES, BLOCKS_AIM // groups))
    tiles = -(-P // ROW_LANES)
    rps = -(-tiles // slices) * ROW_LANES
    return dict(P=P, C=C, groups=groups, slices=slices, tiles=tiles, rps=rps)


def slice_rows(pl, s):
    r0 = min(s * pl["rps"], pl["P"])
    return r0, min(s * pl["rps"] + pl["rps"], pl["P"])


def lane_rows(r0, r1, ry):
    first = r0 + ry
    return 0 if first >= r1 else -(-(r1 - first) // ROW_LANES)


def used_slices(pl):
    return -(-pl["P"] // pl["rps"])


def lane_walk(r0, r1, ry):
    """the three-part walk of k_bn_stats for one lane -> (first row or None, [first row of each trip], [tail rows])"""
    r = r0 + ry
    if r >= r1:
        return None, [], []
    first, trips, tail = r, [], []
    r += ROW_LANES
    while r + 3 * ROW_LANES < r1:
        trips.append(r)
        r += 4 * ROW_LANES
    while r < r1:
        tail.append(r)
        r += ROW_LANES
    return first, trips, tail


def regime(pl):
    """what the walk does at this plan: the facts the CPU test asserts the table's coverage from"""
    used = used_slices(pl)
    counts, ragged_unrolled, trips, tails = set(), False, set(), set()
    for s in sorted({0, 1, used - 2, used - 1, used, pl["slices"] - 1}):
        if not 0 <= s < pl["slices"]:
            continue
        r0, r1 = slice_rows(pl, s)
        mine = [lane_rows(r0, r1, ry) for ry in range(ROW_LANES)]
        counts.update(mine)
        if pl["rps"] >= 160 and r1 > r0 and len(set(mine)) > 1:
            ragged_unrolled = True
        for ry in range(ROW_LANES):
            _, t, tl = lane_walk(r0, r1, ry)
            trips.add(len(t))
            tails.add(len(tl))
    return dict(lane_counts=counts, used=used, empty=pl["slices"] - used, ragged_unrolled=ragged_unrolled, trips=trips,
                tails=tails, idle_final_lane=pl["slices"] < FINAL_LANES)


def edge_rows(pl):
    """the rows a wrong walk loses or doubles first: 0, 31, 32, P - 1; the first and last row of the first, the second, the
    last used and the last full slice; where the unrolled loop runs (rps >= 160), for lanes 0, 5 and 31 of those slices the
    lane's first row and the second and fourth row of its first trip; the first tail row of those lanes"""
    P, rps = pl["P"], pl["rps"]
    used, full = used_slices(pl), P // rps
    rows = {0, 31, 32, P - 1}
    for s in {0, 1, used - 1, full - 1}:
        if not 0 <= s < used:
            continue
        r0, r1 = slice_rows(pl, s)
        rows.update((r0, r1 - 1))
        for ry in (0, 5, 31):
            first, trips, tail = lane_walk(r0, r1, ry)
            if first is None:
                continue
            if rps >= 160:
                rows.update((first, first + 2 * ROW_LANES, first + 4 * ROW_LANES))
            if tail and rps > ROW_LANES:
                rows.add(tail[0])
    return sorted(r for r in rows if 0 <= r < P)


# ----------------------------------------------------------------------------- the table
CHANNELS = {64: 256, 128: 256, 320: 204, 2048: 32, 4096: 16, 4160: 15, 8192: 8, 65536: 1, 65600: 1}     # C: slices
FEW_ROWS = (2, 3, 31, 32, 33, 63, 64, 65)
IMAGES = (3 * 117 * 117, 64)       # a batch of three 117 x 117 maps


def _rows(S):
    """row counts by what the walk does with them, named"""
    return {"one_tile-1": 32 * S - 1, "one_tile": 32 * S, "one_tile+1": 32 * S + 1, "four_rows-1": 128 * S - 1,
            "four_rows": 128 * S, "unrolled_ragged": 128 * S + 1, "unrolled-31": 160 * S - 31, "unrolled-1": 160 * S - 1,
            "unrolled": 160 * S, "trip_tail1": 192 * S, "trip_tail3_ragged": 256 * S - 33, "two_trips": 288 * S}


WANTED = {
    64: list(_rows(1)),
    128: ["one_tile+1", "trip_tail3_ragged"],
    320: ["one_tile-1", "one_tile+1", "four_rows", "unrolled-31", "trip_tail1"],
    2048: ["one_tile+1", "four_rows-1", "unrolled-31", "trip_tail3_ragged", "two_trips"],
    4096: ["one_tile", "unrolled-31", "unrolled", "two_trips"],
    4160: ["one_tile+1", "unrolled-31", "two_trips"],
    8192: ["one_tile-1", "unrolled", "two_trips"],
    65536: ["unrolled-31", "unrolled", "two_trips"],
    65600: ["one_tile+1", "unrolled-31"],
}
# the other data families, each on walks the plain family has too: (row name, C, family)
FAMILIES = [("unrolled-1", 64, "offset"), ("trip_tail3_ragged", 64, "offset"), ("unrolled-1", 64, "spike"),
            ("unrolled-31", 2048, "spike"), ("trip_tail1", 64, "constant"), ("unrolled-31", 320, "constant")]
CONSTANT_CHANNEL, CONSTANT_VALUE = 5, 0.75


def _build():
    cases, seen = [], set()

    def add(P, C, family, why):
        if (P, C, family) in seen:
            return
        seen.add((P, C, family))
        cases.append(dict(id="P%d_C%d_%s" % (P, C, family), P=P, C=C, family=family, why=why))
    for C, S in CHANNELS.items():
        assert plan(2, C)["slices"] == S
        if C in (64, 320, 65536):
            for P in FEW_ROWS:
                add(P, C, "plain", "few_rows")
        rows = _rows(S)
        for name in WANTED[C]:
            add(rows[name], C, "plain", name)
    add(IMAGES[0], IMAGES[1], "plain", "images")
    for name, C, family in FAMILIES:
        add(_rows(CHANNELS[C])[name], C, family, name)
    return cases


CASES = _build()
BY_ID = {c["id"]: c for c in CASES}


def case_of(why, C, family="plain"):
    return next(c for c in CASES if (c["why"], c["C"], c["family"]) == (why, C, family))


CHAIN_CASES = (("unrolled-1", 64), ("trip_tail3_ragged", 2048), ("unrolled", 65536))


# ----------------------------------------------------------------------------- inputs
EDGE_SIGMAS = 2.5                  # where an edge row's x stands from the channel's mean, in the channel's spread


def make_inputs(c):
    """CPU tensors, from a generator seeded by the case id.
    x [P, C] f16: Gaussian with a per-channel mean of the order of the spread; `offset`: mean 8, sigma 1/16; `spike`: every 97th
      row times 40 (a lane whose first value is such a row shifts by an outlier); `constant`: channel 5 is 0.75 in every row.
      On the edge rows x is the channel's mean +- 2.5 sigma, the sign alternating per channel and per edge row (so that they
      do not move the mean together), except in the constant channel.
    g [P, C] f16, the cotangent: k / 4, 1 <= |k| <= 8, so every partial sum of it is a multiple of 1/4 below 2^22, exact in f32
      in any order; +-2 on edge rows, where |xhat| >= 2: |g xhat| there is above the channel's mean |g xhat|.
    r [P, C] f16, a residual ~ N(0, 1).
    y [P, C] f16, a forward output for the mask: N(0, 1), and on edge rows a cycle of +0, -0, the smallest subnormal of both
      signs, NaN, 1 and -1.
    gamma, beta [C] f32: a ramp over the channel's place in its octet plus noise, so that no two channels of an octet agree, as
      f16 either; running_mean, running_var [C] f32."""
    gen = torch.Generator().manual_seed(zlib.crc32(c["id"].encode()))
    P, C, family = c["P"], c["C"], c["family"]
    pl = plan(P, C)
    x = torch.randn((P, C), generator=gen)
    if family == "offset":
        x = 8.0 + x / 16.0
    else:
        x = x * 0.8 + torch.randn((1, C), generator=gen)
    if family == "spike":
        x[::97] *= 40.0
    x = x.to(F16)
    xd = x.to(F64)
    m, sd = xd.mean(0), xd.std(0, unbiased=False)
    sd = sd.clamp_min(0.25 * float(sd.median()))             # (two rows may all but agree in one channel of 65536)
    E = torch.tensor(edge_rows(pl))
    ch = torch.arange(C)
    sign = 1.0 - 2.0 * ((ch[None, :] + torch.arange(len(E))[:, None]) % 2).to(F64)
    x[E] = (m[None, :] + sign * EDGE_SIGMAS * sd[None, :]).to(F16)
    if family == "constant":
        x[:, CONSTANT_CHANNEL] = CONSTANT_VALUE
    k = torch.randint(1, 9, (P, C), generator=gen).to(F32) * (1.0 - 2.0 * torch.randint(0, 2, (P, C), generator=gen).to(F32))
    g = (k / 4.0).to(F16)
    g[E] = torch.where(g[E] < 0, -2.0, 2.0).to(F16)
    r = torch.randn((P, C), generator=gen).to(F16)
    y = torch.randn((P, C), generator=gen).to(F16)
    cycle = torch.tensor([0.0, -0.0, SUBNORMAL, -SUBNORMAL, float("nan"), 1.0, -1.0], dtype=F16)
    y[E] = cycle[(ch[None, :] + torch.arange(len(E))[:, None]) % 7]
    place = (ch % 8).to(F32)
    gamma = 0.5 + place / 8.0 + 0.02 * torch.randn((C,), generator=gen)
    beta = -0.7 + 0.2 * place + 0.02 * torch.randn((C,), generator=gen)
    return dict(x=x, g=g, r=r, y=y, gamma=gamma, beta=beta, running_mean=torch.randn((C,), generator=gen),
                running_var=torch.rand((C,), generator=gen) + 0.5, edge=E)


def params(inp, dtype):
    """gamma and beta as the kernel gets them (f32 or f16 bits)"""
    return inp["gamma"].to(dtype), inp["beta"].to(dtype)


# ----------------------------------------------------------------------------- float64 references (any device)
def stats64(x):
    """-> dict(mean, m2, var (biased), spread = max_r |x - mean|), float64, two passes"""
    xd = x.to(F64)
    P = xd.shape[0]
    mean = xd.mean(0)
    d = xd - mean
    m2 = (d * d).sum(0)
    return dict(P=P, mean=mean, m2=m2, var=m2 / P, spread=d.abs().amax(0))


def given_stats(st, eps=EPS):
    """the float64 statistics rounded to f32: what apply and the backward passes are GIVEN, independent of the stats kernel"""
    return st["mean"].to(F32), (1.0 / torch.sqrt(st["var"] + eps)).to(F32)


def apply64(x, mean, invstd, gamma, beta, r, relu):
    """-> (y, S): the output and the scale of its bound, from the given f32 mean / invstd and the parameters' bits"""
    t = (x.to(F64) - mean.to(F64)) * (invstd.to(F64) * gamma.to(F64))
    y, S = t + beta.to(F64), t.abs() + beta.to(F64).abs()
    if r is not None:
        y, S = y + r.to(F64), S + r.to(F64).abs()
    return (torch.relu(y) if relu else y), S


def masked(g, y):
    """the rule of both backward kernels: out <= 0 -> 0, a NaN output passes the gradient"""
    return g if y is None else torch.where(y <= 0, torch.zeros_like(g), g)


def reduce64(g, x, mean, invstd):
    """-> dict(sg, sgx, l1 = sum |g xhat|), float64; g already behind its mask"""
    gd = g.to(F64)
    gx = gd * ((x.to(F64) - mean.to(F64)) * invstd.to(F64))
    return dict(sg=gd.sum(0), sgx=gx.sum(0), l1=gx.abs().sum(0))


def given_coef(red, P):
    return torch.cat([red["sg"] / P, red["sgx"] / P]).to(F32)


def input64(g, x, mean, invstd, gamma, coef):
    """-> (dx, S) from the given f32 coef / mean / invstd; g already behind its mask"""
    C = x.shape[1]
    a = invstd.to(F64) * gamma.to(F64)
    xh = (x.to(F64) - mean.to(F64)) * invstd.to(F64)
    k1, k2 = coef[:C].to(F64), coef[C:].to(F64)
    gd = g.to(F64)
    return a * (gd - k1 - xh * k2), a.abs() * (gd.abs() + k1.abs() + (xh * k2).abs())


# ----------------------------------------------------------------------------- bounds and comparators
def _ratio(err, bound):
    """largest error over bound; 0 / 0 counts as inside, a NaN anywhere as outside"""
    q = torch.where((err == 0) & (bound == 0), torch.zeros_like(err), err / bound)
    return float(torch.nan_to_num(q, nan=math.inf, posinf=math.inf).max())


def store_rounding(dtype):
    return U32 if dtype == F32 else U16 + 2 * U32


def store_floor(dtype):
    """below 2^-14 an f16 is subnormal and its rounding an absolute 2^-25 (some channel of 65536 lands there)"""
    return 0.0 if dtype == F32 else TINY


def mean_bound(st, K=None):
    return (K_M if K is None else K) * U32 * (st["mean"].abs() + st["spread"])


def var_bound(st, K=None):
    return (K_V if K is None else K) * U32 * st["var"]


def invstd_bound(st, eps):
    def f(v):
        return 1.0 / torch.sqrt(v + eps)
    k = K_V * U32
    mid, lo, hi = f(st["var"]), f(st["var"] * (1 + k)), f(st["var"] * (1 - k))
    return torch.maximum(hi - mid, mid - lo) + U32 * hi


def compare_mean(mean, st):
    return _ratio((mean.to(F64) - st["mean"]).abs(), mean_bound(st))


def compare_invstd(invstd, st, eps):
    return _ratio((invstd.to(F64) - 1.0 / torch.sqrt(st["var"] + eps)).abs(), invstd_bound(st, eps))


def running64(st, rm, rv, momentum):
    """-> ((ref, bound) of running_mean, (ref, bound) of running_var) for buffers of rm's dtype holding rm / rv before"""
    P, rnd = st["P"], store_rounding(rm.dtype)
    out = []
    for old, new, b in ((rm, st["mean"], mean_bound(st)), (rv, st["m2"] / (P - 1), var_bound(st) * P / (P - 1))):
        ref = (1.0 - momentum) * old.to(F64) + momentum * new
        b = momentum * b
        out.append((ref, b + rnd * (ref.abs() + b) + store_floor(rm.dtype)))
    return out


def compare_elementwise(got, ref, S, K):
    """|got - ref| <= t + u16 (|ref| + t) + 2^-25 with t = K u32 S, at every element"""
    return compare_within(got, ref, K * U32 * S)


def compare_within(got, ref, t):
    """an f32 error of at most t, then one f16 rounding of the perturbed value"""
    assert tuple(got.shape) == tuple(ref.shape)
    return _ratio((got.to(F64) - ref).abs(), t + U16 * (ref.abs() + t) + TINY)


def compare_sum(got, ref, l1, dtype, over=1.0):
    """grad_weight (over = 1) and coef[C:] (over = P): K_W u32 sum |g xhat| / over, then the store's rounding"""
    b = K_W * U32 * l1 / over
    return _ratio((got.to(F64) - ref / over).abs(), b + store_rounding(dtype) * ((ref / over).abs() + b) + store_floor(dtype))


def chain64(x, r, gm, gamma, beta, st, eps):
    """the four passes chained (residual, ReLU, f32 parameters), float64 throughout from the float64 statistics; gm is the
    cotangent behind PRODUCTION's mask.  The scales are the complete t of compare_within: the pass's own
    K u32 S plus what the statistics' bounds dm, di allow, to first order:
        out:  dm |invstd gamma| + |x - mean| |gamma| di
        dx = a (g - k1 - xhat k2):  dxhat = dm invstd + |x - mean| di,  da = |gamma| di,  dk1 = u32 |k1| (sum g is exact),
              dk2 = (K_W u32 sum |g xhat| + sum |g| dxhat) / P + u32 |k2|,
              da |g - k1 - xhat k2| + |a| (dk1 + dxhat |k2| + |xhat| dk2)"""
    P = x.shape[0]
    xd, gd, ga = x.to(F64), gm.to(F64), gamma.to(F64)
    mean, invstd = st["mean"], 1.0 / torch.sqrt(st["var"] + eps)
    dm, di = mean_bound(st), invstd_bound(st, eps)
    dev = xd - mean
    a = invstd * ga
    t = dev * a
    pre = t + beta.to(F64) + r.to(F64)
    S = t.abs() + beta.to(F64).abs() + r.to(F64).abs()
    out_scale = K_A * U32 * S + dm * a.abs() + dev.abs() * ga.abs() * di
    xh = dev * invstd
    dxh = dm * invstd + dev.abs() * di
    gx = gd * xh
    sg, sgx, l1 = gd.sum(0), gx.sum(0), gx.abs().sum(0)
    k1, k2 = sg / P, sgx / P
    dk1 = U32 * k1.abs()
    dk2 = (K_W * U32 * l1 + (gd.abs() * dxh).sum(0)) / P + U32 * k2.abs()
    inner = gd - k1 - xh * k2
    own = K_I * U32 * a.abs() * (gd.abs() + k1.abs() + (xh * k2).abs())
    dx_scale = own + ga.abs() * di * inner.abs() + a.abs() * (dk1 + dxh * k2.abs() + xh.abs() * dk2)
    return dict(out=torch.relu(pre), out_scale=out_scale, dx=a * inner, dx_scale=dx_scale, sg=sg)


def classes(t):
    t = t.to(F64)
    return torch.where(t.isnan(), 3, torch.where(t == math.inf, 2, torch.where(t == -math.inf, 1, 0)))


# ----------------------------------------------------------------------------- the f32 restatement of the kernels' order
def _sliced(t, pl, fill=0.0):
    """[P, C] -> [slices, steps, 32, C] (rows past P hold `fill`) and the [slices, steps, 32] map of rows that exist"""
    S, rps, P = pl["slices"], pl["rps"], pl["P"]
    full = torch.full((S * rps, t.shape[1]), fill, dtype=t.dtype)
    full[:P] = t
    exists = (torch.arange(S * rps) < P).view(S, rps // ROW_LANES, ROW_LANES)
    return full.view(S, rps // ROW_LANES, ROW_LANES, t.shape[1]), exists


def _merge(n, mean, m2):
    """the k-way merge of bn_plan.hpp over dim 0, in double: members of count 0 take no part -> (n, mean, M2)"""
    n = n.to(F64)
    while n.dim() < mean.dim():
        n = n.unsqueeze(-1)
    tot = n.sum(0)
    safe = torch.where(tot == 0, torch.ones_like(tot), tot)
    mu = (n * mean * (n > 0)).sum(0) / safe
    q = ((m2 + n * (mean - mu) ** 2) * (n > 0)).sum(0)
    return tot, torch.where(tot == 0, torch.zeros_like(mu), mu), torch.where(tot == 0, torch.zeros_like(q), q)


def restate_stats(x):
    """k_bn_stats + k_bn_stats_final on the CPU: f32 lane sums around the lane's first value, LaneAcc::finish in f32, the merge
    of the 32 lanes in double and its rounding to the f32 `partial`, sixteen final lanes each merging every sixteenth slice,
    their merge -> (mean, M2) in double, before any store"""
    P, C = x.shape
    pl = plan(P, C)
    xs, exists = _sliced(x.to(F32), pl)
    n = exists.sum(1)                                        # [slices, 32]: a lane's rows
    K = xs[:, 0]
    s1 = torch.zeros_like(K)
    s2 = torch.zeros_like(K)
    for t in range(1, xs.shape[1]):
        d = xs[:, t] - K
        on = exists[:, t, :, None]
        s1 = torch.where(on, s1 + d, s1)
        s2 = torch.where(on, s2 + d * d, s2)
    inv = (1.0 / n.clamp_min(1).to(F32))[..., None]
    mean = K + s1 * inv
    v = s2 - s1 * s1 * inv
    m2 = torch.where(v < 0, torch.zeros_like(v), v)
    ns, ms, qs = _merge(n.t(), mean.transpose(0, 1).to(F64), m2.transpose(0, 1).to(F64))       # lanes -> slices
    ms, qs = ms.to(F32).to(F64), qs.to(F32).to(F64)          # `partial` is f32
    ns = ns[:, 0] if ns.dim() > 1 else ns
    lanes = [_merge(ns[q::FINAL_LANES], ms[q::FINAL_LANES], qs[q::FINAL_LANES]) for q in range(min(FINAL_LANES, pl["slices"]))]
    nl = torch.stack([l[0].reshape(()) for l in lanes])
    tot, mu, q = _merge(nl, torch.stack([l[1] for l in lanes]), torch.stack([l[2] for l in lanes]))
    assert int(tot) == P
    return mu, q


def restate_apply(x, mean, invstd, gamma, beta, r):
    """k_bn_apply before the ReLU and the store, f32"""
    y = (x.to(F32) - mean) * (invstd * gamma.to(F32)) + beta.to(F32)
    return y if r is None else y + r.to(F32)


def restate_reduce(g, x, mean, invstd):
    """k_bn_bwd_reduce + k_bn_bwd_final: a lane adds its rows in f32, the 32 lanes are added in f32 in lane order, the slices
    in double -> (sum g, sum g xhat) in double, before any store"""
    pl = plan(*x.shape)
    gs, exists = _sliced(g.to(F32), pl)
    xs, _ = _sliced(x.to(F32), pl)
    sg = torch.zeros_like(gs[:, 0])
    sgx = torch.zeros_like(sg)
    for t in range(gs.shape[1]):                             # (rows that do not exist hold g = 0 and x = 0: they add +-0)
        sg = sg + gs[:, t]
        sgx = sgx + gs[:, t] * ((xs[:, t] - mean) * invstd)
    a = torch.zeros_like(sg[:, 0])
    b = torch.zeros_like(a)
    for q in range(ROW_LANES):
        a = a + sg[:, q]
        b = b + sgx[:, q]
    return a.to(F64).sum(0), b.to(F64).sum(0)


def restate_input(g, x, mean, invstd, gamma, coef):
    """k_bn_bwd_input before the store, f32"""
    C = x.shape[1]
    a = invstd * gamma.to(F32)
    xh = (x.to(F32) - mean) * invstd
    return a * (g.to(F32) - coef[:C] - xh * coef[C:])


def restatement_ratios(c, inp=None):
    """the restatement against float64 on one case, in units of u32 times each bound's scale -> {constant name: worst ratio}"""
    inp = make_inputs(c) if inp is None else inp
    x, g, P = inp["x"], inp["g"], c["P"]
    st = stats64(x)
    mu, q = restate_stats(x)
    out = {"K_M": _ratio((mu - st["mean"]).abs(), mean_bound(st, 1)), "K_V": _ratio((q / P - st["var"]).abs(), var_bound(st, 1))}
    mean, invstd = given_stats(st)
    ka = ki = kw = 0.0
    # the sums take every row; the two elementwise passes, whose error does not know the shape, take every n-th row and the
    # edge rows once a case has more than 2^21 elements
    rows = torch.arange(0, P, max(1, (P * c["C"]) >> 21))
    rows = torch.cat([rows, inp["edge"]]).unique()
    xs, rs = x[rows], inp["r"][rows]
    for y in (None, inp["y"]):
        gm = masked(g, y)
        red = reduce64(gm, x, mean, invstd)
        a, b = restate_reduce(gm, x, mean, invstd)
        assert torch.equal(a, red["sg"])                     # dyadic: exact whatever the order
        kw = max(kw, _ratio((b - red["sgx"]).abs(), U32 * red["l1"]))
        coef = given_coef(red, P)
        for dtype in (F32, F16):
            gamma, beta = params(inp, dtype)
            dx, S = input64(gm[rows], xs, mean, invstd, gamma, coef)
            ki = max(ki, _ratio((restate_input(gm[rows], xs, mean, invstd, gamma, coef).to(F64) - dx).abs(), U32 * S))
            if y is None:
                for r in (None, rs):
                    ref, S = apply64(xs, mean, invstd, gamma, beta, r, False)
                    ka = max(ka, _ratio((restate_apply(xs, mean, invstd, gamma, beta, r).to(F64) - ref).abs(), U32 * S))
    out.update(K_A=ka, K_W=kw, K_I=ki)
    return out


# ----------------------------------------------------------------------------- the separation of one row
def separation(c, inp, st):
    """for every edge row and channel: how far the float64 mean or variance moves when the row is left out, or counted twice,
    in units of the statistic's bound; the larger of the two statistics, the smaller of the two defects -> [edge rows, C]"""
    P = c["P"]
    xe = inp["x"][inp["edge"]].to(F64)
    d = xe - st["mean"]
    worst = None
    for n2, sgn in ((P - 1, -1.0), (P + 1, 1.0)):
        mean2 = st["mean"] + sgn * d / n2
        m2 = st["m2"] + sgn * d * d * P / n2                 # the pairwise update with one member of count 1
        moved = torch.maximum((mean2 - st["mean"]).abs() / mean_bound(st), (m2 / n2 - st["var"]).abs() / var_bound(st))
        worst = moved if worst is None else torch.minimum(worst, moved)
    return worst
