"""Inputs and case tables of tests/test_gpu_glue.py, shared with tests/test_glue64_cpu.py: the CPU test holds the float32
oracle against oracle/glue64.py on exactly the rows the GPU test feeds the kernels, and checks that the candidate
selection cases reach every route of s2a_pyramid_candidates."""
import numpy as np

DECODE_CLIPS = (1e-6, 16 / 1000)
DECODE_SIZES = (1, 255, 257, 5000)
WRAP_EPS = (0.0, 1e-6, -1e-6, 1e-3, -1e-3)


def wrap_rows():
    """32 rows whose raw angle pi*da + a sits 0, +-1e-6 and +-1e-3 from a wrap point -pi/4 + m*pi (anchor angle and
    m varied; da solved for in float64 and rounded to float32, so "0" means within a float32 rounding of the point)"""
    rois, deltas = [], []
    combos = [(a, m) for a in (-0.7, 0.0, 0.3, 1.1, 2.2, 2.35) for m in (-1, 0, 1, 2)]
    rng = np.random.default_rng(77)
    for i in range(32):
        a, m = combos[i % len(combos)]
        a = float(np.float32(a))
        eps = WRAP_EPS[i % len(WRAP_EPS)]
        da = np.float32((-np.pi / 4 + m * np.pi + eps - a) / np.pi)
        assert abs(da) <= 3
        rois.append([rng.uniform(0, 1024), rng.uniform(0, 1024), rng.uniform(4, 512), rng.uniform(4, 512), a])
        deltas.append(list(rng.standard_normal(4) * 0.6) + [da])
    r, d = np.asarray(rois, np.float32), np.asarray(deltas, np.float32)
    r[0, 4], d[0, 4] = np.float32(-np.pi / 4), 0.0                  # the float32 lower end itself, untouched by a delta
    r[1, 4], d[1, 4] = np.nextafter(np.float32(3 * np.pi / 4), np.float32(0)), 0.0
    return r, d


def decode_rows(n, seed=0):
    """the decode distribution: centres uniform in [0, 1024), sizes in [4, 512), anchor angle in [-pi/4, 3pi/4), deltas
    N(0, 0.6), da uniform in [-3, 3], 1 % of the rows with dw / dh scaled x40 (both sides of the clip saturate at
    either clip), and from 255 rows on the first 32 rows replaced by wrap_rows()"""
    rng = np.random.default_rng(seed)
    r = np.empty((n, 5), np.float32)
    r[:, 0:2] = rng.uniform(0, 1024, (n, 2))
    r[:, 2:4] = rng.uniform(4, 512, (n, 2))
    r[:, 4] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, n)
    d = (rng.standard_normal((n, 5)) * 0.6).astype(np.float32)
    d[:, 4] = rng.uniform(-3, 3, n).astype(np.float32)
    sat = np.arange(n) % 100 == 99
    d[sat, 2:4] *= 40
    d[99::200, 2:4] = (30.0, -30.0)                                  # whatever the draw: both signs in every set of >= 200 rows
    d[199::200, 2:4] = (-30.0, 30.0)
    if n >= 255:
        r[:32], d[:32] = wrap_rows()
    return r, d


# fam_refine_anchors: (B, H, W) x stride, f32 / f16, NCHW / channels-last
REFINE_SHAPES = ((1, 1, 1), (2, 12, 20), (3, 17, 15))
REFINE_STRIDES = (8, 128)
PYRAMID5 = (2, ((33, 47), (17, 24), (9, 12), (5, 6), (3, 3)), (8, 16, 32, 64, 128))
PYRAMID8 = (2, ((6, 7), (5, 5), (4, 6), (3, 4), (3, 3), (2, 2), (1, 2), (1, 1)), (4, 8, 16, 32, 64, 128, 256, 512))
PYRAMID_ROW_STRIDE = 64


def refine_pred(shape, seed=0):
    """[..., 5]-last deltas of the decode distribution as float16-representable float32 (the same values serve the
    f32 and the f16 kernels): N(0, 0.6), da in [-3, 3], every 100th row's dw / dh x40 (past the 1e-6 clip)"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal(tuple(shape) + (5,)) * 0.6
    d[..., 4] = rng.uniform(-3, 3, tuple(shape))
    flat = d.reshape(-1, 5)
    flat[np.arange(flat.shape[0]) % 100 == 99, 2:4] *= 40
    flat[0, 2:4] = (30.0, -30.0)
    return d.astype(np.float16).astype(np.float32)


# align_offsets: (H, W, stride, kernel size)
ALIGN_CASES = ((12, 20, 8, 3), (12, 20, 64, 3), (7, 9, 8, 3), (7, 9, 64, 3), (7, 9, 8, 5))
ALIGN_BATCH = 2


def align_anchors(H, W, stride, seed=0):
    """[ALIGN_BATCH, H*W, 5]: grid centres moved by N(0, 3 strides), every 7th anchor 40-60 strides off the grid, sides
    of 1 to 40 strides, any angle of [-pi/4, 3pi/4)"""
    rng = np.random.default_rng(seed)
    n = H * W
    a = np.empty((ALIGN_BATCH, n, 5), np.float64)
    ys, xs = np.divmod(np.arange(n), W)
    a[..., 0] = xs * stride + 0.5 * (stride - 1) + rng.standard_normal((ALIGN_BATCH, n)) * 3 * stride
    a[..., 1] = ys * stride + 0.5 * (stride - 1) + rng.standard_normal((ALIGN_BATCH, n)) * 3 * stride
    far = np.arange(n) % 7 == 3
    a[:, far, :2] += rng.choice([-1.0, 1.0], (ALIGN_BATCH, int(far.sum()), 2)) * rng.uniform(40, 60, (ALIGN_BATCH, int(far.sum()), 2)) * stride
    a[..., 2:4] = rng.uniform(1, 40, (ALIGN_BATCH, n, 2)) * stride
    a[..., 4] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, (ALIGN_BATCH, n))
    return a.astype(np.float32)


# ---------------------------------------------------------------------------------------------- candidate selection
TOPK_MAX_N = 24576                                                   # kTopkMaxN of glue_ops.hip


def _eight_levels():
    return ((40, 60), (20, 30), (10, 15), (5, 8), (3, 4), (2, 2), (1, 2), (1, 1))


# (name, B, C, level sizes, k)
CAND_CASES = (
    ("one_dropped", 2, 15, ((3, 667),), 2000),
    ("cap_keys", 2, 15, ((128, 192),), 2000),
    ("cap_vector", 2, 3, ((128, 192),), 2000),
    ("two_vectors", 2, 9, ((60, 100),), 300),
    ("one_vector", 2, 8, ((60, 100),), 150),
    ("generic17", 2, 17, ((60, 100),), 100),
    ("generic64", 2, 64, ((60, 100),), 40),
    ("around_k", 2, 16, ((50, 50), (45, 45), (44, 45), (5, 7)), 2000),
    ("k1", 2, 1, ((70, 90),), 1),
    ("eight_levels", 3, 15, _eight_levels(), 500),
)
KEY_KINDS = ("distinct", "ties", "equal", "negative", "special")


def out_slots(sizes, k):
    """first output slot of every level, and the row count n per image (cand_levels of glue_ops.hip)"""
    out0, n = [], 0
    for h, w in sizes:
        out0.append(n)
        n += k if (k > 0 and h * w > k) else h * w
    return out0, n


def topk_route(batch, sizes, num_classes, k):
    """which key route s2a_pyramid_candidates takes.  Mirrors glue_ops.hip, s2a_pyramid_candidates:
    `if (rows * sizeof(unsigned short) <= total * num_classes * sizeof(float) && cls % 16 == 0)` -> keys precomputed by
    k_pyr_keys into the scores buffer ("K"); otherwise k_pyr_topk computes them: `else if (nvec > 2)` with
    nvec = (num_classes + 7) / 8 is the plain loop ("L-generic"), the rest the four-in-flight vector loop
    ("L-vector").  (torch allocations are 16-byte aligned.)"""
    rows = batch * sum(h * w for h, w in sizes)
    total = batch * out_slots(sizes, k)[1]
    if rows * 2 <= total * num_classes * 4:
        return "K"
    return "L-generic" if (num_classes + 7) // 8 > 2 else "L-vector"


def _f16_pool(lo, hi):
    """every float16 value of [lo, hi] except the two zeros, ascending"""
    v = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    v = v[np.isfinite(v) & (v != 0) & (v >= lo) & (v <= hi)]
    return np.sort(v)


def cand_logits(batch, num_classes, sizes, kind, seed=0):
    """class logits [P, 64] float16 of a pyramid-packed buffer whose per-row maximum over the first num_classes columns
    follows `kind`, the maximum sitting in a random column; columns >= num_classes hold +inf (a read past the classes
    wins every comparison and shows).  Finite logits stay >= -9, where the float16 sigmoid is still a normal number;
    no zero of either sign is used (the kernel orders -0 below +0, a float comparison does not)."""
    rng = np.random.default_rng(seed)
    C = num_classes
    segs = [h * w for h, w in sizes for _ in range(batch)]
    P = sum(segs)
    mx = np.empty(P, np.float16)
    p = 0
    for hw in segs:
        if kind == "distinct":                                     # distinct inside every (image, level)
            m = rng.permutation(_f16_pool(-6, 6))[:hw]
            assert m.size == hw
        elif kind == "ties":
            m = rng.choice(np.array([-1.5, -0.25, 0.5, 0.75, 2.0, 3.0], np.float16), hw)
        elif kind == "equal":
            m = np.full(hw, 0.5, np.float16)
        elif kind == "negative":
            m = rng.choice(_f16_pool(-6, -1e-7), hw)
        elif kind == "special":                                    # sign branch of f16_key, both infinities, subnormals
            sub = np.array([1, 2, 3, 512, 1023], np.uint16).view(np.float16)
            special = np.concatenate([np.array([np.inf, -np.inf, 65504.0, -6.0, 6.1e-5, -6.1e-5], np.float16), sub, -sub])
            m = np.where(rng.random(hw) < 0.5, rng.choice(special, hw), rng.choice(_f16_pool(-6, 6), hw))
        else:
            raise ValueError(kind)
        mx[p:p + hw] = m
        p += hw
    cls = np.full((P, 64), np.inf, np.float16)
    with np.errstate(invalid="ignore"):
        low = mx.astype(np.float32)[:, None] - rng.uniform(0, 3, (P, C)).astype(np.float32)
    low[np.isnan(low)] = -np.inf                                   # never: inf - finite; kept for safety
    cls[:, :C] = np.minimum(low.astype(np.float16), mx[:, None])
    cls[np.arange(P), rng.integers(0, C, P)] = mx
    return cls


def cand_reg_anchors(P, seed=0):
    """box deltas [P,64] float16 (first five columns; the rest NaN: never read) and rotated anchors [P,5] float32"""
    rng = np.random.default_rng(seed + 1)
    reg = np.full((P, 64), np.nan, np.float16)
    d = rng.standard_normal((P, 5)) * 0.6
    d[:, 4] = rng.uniform(-3, 3, P)
    d[np.arange(P) % 100 == 99, 2:4] *= 40
    reg[:, :5] = d
    anc = np.empty((P, 5), np.float32)
    anc[:, 0:2] = rng.uniform(0, 1024, (P, 2))
    anc[:, 2:4] = rng.uniform(4, 512, (P, 2))
    anc[:, 4] = rng.uniform(-np.pi / 4, 3 * np.pi / 4, P)
    return reg, anc


# ---------------------------------------------------------------------------------------------- epilogue
# (B, C, H, W, dtypes): C is the f16 channel count; f32 runs the same shape (the first one with 4 channels)
EPILOGUE_SHAPES = (
    (1, 8, 1, 1),          # one vector
    (2, 24, 5, 7),         # cvec 3: bias not hoisted
    (1, 320, 9, 11),       # cvec 40: not hoisted
    (1, 4096, 3, 3),       # cvec 512 > 256
    (1, 2048, 4, 4),       # cvec 256: hoisted
    (2, 64, 33, 47),
)
EPILOGUE_LARGE = (1, 64, 524, 524)    # f16: 2 196 608 vectors, past the 2048-workgroup cap (one full four-stream trip + tail)
# the four-stream loop makes a second trip only beyond 7 * 2048 * 256 = 3 670 016 vectors: 3 699 200 here
EPILOGUE_SECOND_TRIP = (1, 64, 680, 680)
