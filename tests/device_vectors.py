"""The unit vectors of the device-math headers (vo_math.h, vo_linalg.h, vo_svd_wide.h, vo_epnp.h, vo_lkmath.h, vo_isa.h): one set of
generators for the CPU tests (host build, emulator) and for the GPU test that runs the same vectors on gfx950
(tests/test_gpu_device_units.py through tests/host_check/device_check.hip).  A plain module: no fixtures, no assertions about
the code under test -- only inputs, each with a fixed seed."""
import numpy as np

K_KITTI = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)

# the hand-over of vo_cos / vo_sin to the platform's function (vo_math.h): nothing at or above it is bit-portable
TRIG_BOUND = 823549.6


# ---------------------------------------------------------------------------------------------
# vo_math.h
def cbrt_args():
    rng = np.random.default_rng(1)
    return np.concatenate([rng.uniform(0, 10, 200000), 10 ** rng.uniform(-300, 300, 200000), [1e-310, 5e-324]])


CBRT_EDGES = [0.0, -1.0, np.inf, np.nan, 8.0, 27.0, 1e-300]


def acos_args():
    rng = np.random.default_rng(2)
    return np.concatenate([rng.uniform(-1, 1, 400000), 1 - 10 ** rng.uniform(-16, 0, 50000), -1 + 10 ** rng.uniform(-16, 0, 50000),
                           [0.0, 0.5, -0.5, 1e-20, -1e-20]])


ACOS_EDGES = [1.0, -1.0, 1.0000001, -2.0, np.nan]


def cos_args():
    rng = np.random.default_rng(3)
    near = np.pi / 2 * np.arange(1, 64) + rng.uniform(-1e-9, 1e-9, 63)  # next to the multiples of pi / 2 (cancellation)
    return np.concatenate([rng.uniform(0, 5.3, 400000), rng.uniform(-1000, 1000, 100000), near, [0.0, np.pi / 2, np.pi, 2 * np.pi / 3]])


def sin_args():
    rng = np.random.default_rng(4)
    near = np.pi / 2 * np.arange(1, 64) + rng.uniform(-1e-9, 1e-9, 63)
    return np.concatenate([rng.uniform(-3.2, 3.2, 400000), rng.uniform(-1000, 1000, 100000), near, -near, [0.0, 1e-300, -1e-10]])


def trig_large_args():
    """vo_cos / vo_sin up to, but below, the hand-over bound: the whole range log-uniformly, the last stretch before the bound,
    and arguments within 1e-9 of the multiples of pi / 2 just below it (n up to 2^19 - 1: the deepest cancellation the
    two-piece reduction has to carry)"""
    rng = np.random.default_rng(41)
    k = np.arange(2 ** 19 - 256, 2 ** 19)
    near = np.pi / 2 * k + rng.uniform(-1e-9, 1e-9, len(k))
    x = np.concatenate([10 ** rng.uniform(0, np.log10(TRIG_BOUND), 100000), rng.uniform(TRIG_BOUND - 1000, TRIG_BOUND, 50000), near,
                        [np.nextafter(TRIG_BOUND, 0), TRIG_BOUND - 1e-6]])
    x = x[np.abs(x) < TRIG_BOUND]
    return np.concatenate([x, -x])


TRIG_NONFINITE = [np.nan, np.inf, -np.inf]   # compared by class only: the platform's function answers


def lm_lambda_args():
    return np.arange(-20, 21).astype(np.float64)   # (clamped to [-16, 16] by the routine)


# ---------------------------------------------------------------------------------------------
# vo_lkmath.h: the composites
def weights(rng, n):
    a, b = rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)
    a[:4], b[:4] = [0, 0, 1 - 2**-20, 0.5], [0, 1 - 2**-20, 0, 0.5]
    one = np.float32(1)
    s = np.float32(1 << 14)
    w00 = np.rint((one - a) * (one - b) * s).astype(np.int32)
    w01 = np.rint(a * (one - b) * s).astype(np.int32)
    w10 = np.rint((one - a) * b * s).astype(np.int32)
    w11 = (1 << 14) - w00 - w01 - w10
    return np.ascontiguousarray(np.stack([w00, w01, w10, w11], 1).astype(np.int32))


def descale(x, n):
    return (x + (1 << (n - 1))) >> n


def bilinear_operands():
    """top, bot: n x 8 bytes; w: n x 4 weights (rows 4 .. 11 forced: one weight 2^14, and iw11 = -1)"""
    rng = np.random.default_rng(5)
    n = 20000
    top = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    bot = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    top[:8], bot[:8] = 255, 255
    top[8:16], bot[8:16] = 0, 255
    w = weights(rng, n)
    w[4:8] = [[16384, 0, 0, 0], [0, 16384, 0, 0], [0, 0, 16384, 0], [0, 0, 0, 16384]]
    # three roundings can add up to 2^14 + 1, leaving iw11 = -1 (seen on the MI355X at a = b ~ 0.006)
    w[8:12] = [[16385, 0, 0, -1], [16189, 98, 98, -1], [1, 16383, 1, -1], [8192, 8192, 1, -1]]
    return top, bot, w


def bilinear_reference(top, bot, w):
    t, b = top.astype(np.int64), bot.astype(np.int64)
    return descale(t[:, :7] * w[:, [0]] + t[:, 1:] * w[:, [1]] + b[:, :7] * w[:, [2]] + b[:, 1:] * w[:, [3]], 9)


def deriv_operands():
    """dx, dy: 2 (top / bottom row) x n x 8 true Scharr samples; packed: the same as stored (4 d, two per dword); w: n x 4"""
    rng = np.random.default_rng(6)
    n = 20000
    # true Scharr samples are in [-4080, 4080]; stored pre-multiplied by 4
    dx = rng.integers(-4080, 4081, (2, n, 8)).astype(np.int64)
    dy = rng.integers(-4080, 4081, (2, n, 8)).astype(np.int64)
    dx[:, :4], dy[:, :4] = 4080, -4080
    dx[:, 4:8], dy[:, 4:8] = -4080, 4080
    packed = (((dx * 4) & 0xffff) | (((dy * 4) & 0xffff) << 16)).astype(np.uint32)
    w = weights(rng, n)
    return dx, dy, packed, w


def deriv_reference(d, w):
    return descale(d[0][:, :7] * w[:, [0]] + d[0][:, 1:] * w[:, [1]] + d[1][:, :7] * w[:, [2]] + d[1][:, 1:] * w[:, [3]], 14)


def diff_dot_operands():
    rng = np.random.default_rng(7)
    n = 5000
    val = rng.integers(0, 8161, (n, 7)).astype(np.int16)
    I = rng.integers(0, 8161, (n, 7)).astype(np.int16)
    ix = rng.integers(-4080, 4081, (n, 7)).astype(np.int16)
    val[0], I[0], ix[0] = 8160, 0, 4080       # largest per-lane partial: 7 * 8160 * 4080 < 2^28
    val[1], I[1], ix[1] = 0, 8160, 4080
    return val, I, ix


def scharr_patches():
    """n x 8 neighbours (p00 p01 p02 p10 p12 p20 p21 p22) of random and of extreme 3 x 3 patches"""
    rng = np.random.default_rng(8)
    p = rng.integers(0, 256, (4096, 8)).astype(np.int32)
    p[0], p[1] = 0, 255
    p[2] = [0, 0, 255, 0, 255, 0, 0, 255]      # full-contrast vertical edge: 4 Ix = 16320
    p[3] = [255, 255, 255, 0, 0, 0, 0, 0]      # horizontal edge: 4 Iy = -16320
    return np.ascontiguousarray(p)


# ---------------------------------------------------------------------------------------------
# vo_isa.h (and pack_w of vo_lkmath.h): the raw instruction wrappers.  (n, 3) uint32 operand triples a, b, c per wrapper: 2^20 random ones inside the
# range the header defines the wrapper on, after the edge rows.
LK_RAW = ["perm_b32", "udot2", "sdot2", "sdot2_first", "pk_sub_i16", "pk_lshr1_u16", "udot4", "pk_add_u16", "pk_subsat_u16",
          "pk_min_u16", "pk_mad_u16", "alignbyte", "pack_w", "pk_absdiff_i16"]
N_RAW = 1 << 20


def sel_pix(k):
    return 0x0c | (k << 8) | (0x0c << 16) | ((k + 1) << 24)


# every v_perm_b32 selector the product uses: VO_SEL_PIX(0 .. 6), VO_SEL_LO16, VO_SEL_HI16 (vo_lkmath.h), the four of fast.hip
PRODUCT_SELECTORS = [sel_pix(k) for k in range(7)] + [0x05040100, 0x07060302, 0x0c010c00, 0x0c040c03, 0x0c020c01, 0x0c030c02]


def _pack16(lo, hi):
    return ((np.asarray(lo, np.int64) & 0xffff) | ((np.asarray(hi, np.int64) & 0xffff) << 16)).astype(np.uint32)


def lk_raw_operands(name):
    rng = np.random.default_rng(100 + LK_RAW.index(name))
    r = rng.integers(0, 1 << 32, (N_RAW, 3), dtype=np.uint64).astype(np.uint32)
    words = np.array([0, 0xffffffff, 0x0000ffff, 0xffff0000, 0x80008000, 0x7fff7fff, 0x00010001, 0x80007fff, 0x7fff8000], np.uint32)
    # every pair of the edge words as (a, b), c = 0 and c = all ones
    ea, eb = [g.ravel() for g in np.meshgrid(words, words, indexing="ij")]
    edges = np.concatenate([np.stack([ea, eb, np.full_like(ea, c)], 1) for c in (0, 0xffffffff)])
    if name == "perm_b32":
        # selector bytes 0 .. 7 and 0x0c: what the host text defines
        sel_bytes = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0x0c], np.uint32)
        s = sel_bytes[rng.integers(0, 9, (N_RAW, 4))]
        r[:, 2] = s[:, 0] | s[:, 1] << 8 | s[:, 2] << 16 | s[:, 3] << 24
        single = [b | b << 8 | b << 16 | b << 24 for b in sel_bytes.tolist()]
        sels = np.array(PRODUCT_SELECTORS + single + [0x07060504, 0x03020100, 0x00010203, 0x0c0c0c0c], np.uint32)
        data = np.array([[0, 0], [0xffffffff, 0xffffffff], [0x07060504, 0x03020100], [0x80c0e0f0, 0x01030307], [0xffffffff, 0], [0, 0xffffffff]],
                        np.uint32)
        edges = np.array([[a, b, s_] for a, b in data.tolist() for s_ in sels.tolist()], np.uint32)
    elif name in ("sdot2", "sdot2_first"):
        # the documented ranges: |lane| <= 16320, |accumulator| < 2^28 -- the clamp of sdot2_first must never act, and the host
        # text's int32 sum does not overflow.  The two wrappers get the SAME operands.
        rng = np.random.default_rng(102)
        lanes = rng.integers(-16320, 16321, (N_RAW, 4))
        acc = rng.integers(-(1 << 28) + 1, 1 << 28, N_RAW)
        r = np.stack([_pack16(lanes[:, 0], lanes[:, 1]), _pack16(lanes[:, 2], lanes[:, 3]), (acc & 0xffffffff).astype(np.uint32)], 1)
        ext = [-16320, 16320, 0, -1, 1]
        accs = [0, -1, (1 << 28) - 1, -(1 << 28) + 1, 1 << 15]
        edges = np.array([[int(_pack16(p, q)), int(_pack16(u, v)), c & 0xffffffff] for p in ext for q in ext for u in ext[:2] for v in ext[:3]
                          for c in accs], np.uint32)
    elif name == "udot2":
        # exact sums beyond 2^32: they must wrap
        edges = np.concatenate([edges, np.array([[0xffffffff, 0xffffffff, 0xffffffff], [0xffff0000, 0xffff0000, 0x0001ffff],
                                                 [0xffffffff, 0xffffffff, 0], [0x8000ffff, 0xffff8000, 0xfffffff0]], np.uint32)])
    elif name == "pk_sub_i16":
        # across the wrap: -32768 - 1, 32767 - (-1), 0 - (-32768)
        edges = np.concatenate([edges, np.array([[0x80008000, 0x00010001, 0], [0x7fff7fff, 0xffffffff, 0], [0x00000000, 0x80008000, 0],
                                                 [0x80007fff, 0x0001ffff, 0]], np.uint32)])
    elif name == "pk_subsat_u16":
        # a < b, a == b, 0xffff - 0 in either lane
        edges = np.concatenate([edges, np.array([[0x00010002, 0x00020003, 0], [0x12345678, 0x12345678, 0], [0xffffffff, 0, 0],
                                                 [0x0001ffff, 0x00020000, 0], [0xffff0001, 0x00000002, 0]], np.uint32)])
    elif name == "pk_mad_u16":
        # products beyond 16 bits (and beyond 32 with the accumulator): only the low 16 bits of each lane stay
        edges = np.concatenate([edges, np.array([[0xffffffff, 0xffff, 0xffffffff], [0x01000100, 0x0100, 0x00010001],
                                                 [0x8000ffff, 0x0002, 0xffff0001], [0x12345678, 0xabcd, 0x9abcdef0]], np.uint32)])
    elif name == "alignbyte":
        r[:, 2] &= 3
        edges = np.array([[a, b, k] for a, b in [(0, 0), (0xffffffff, 0xffffffff), (0x07060504, 0x03020100), (0xffffffff, 0), (0, 0xffffffff)]
                          for k in range(4)], np.uint32)
    elif name == "pack_w":
        # [-2^14, 2^14] only: outside int16 the device instruction saturates and the host text wraps; the header rules that out
        w = rng.integers(-(1 << 14), (1 << 14) + 1, (N_RAW, 2))
        r[:, 0], r[:, 1] = (w[:, 0] & 0xffffffff).astype(np.uint32), (w[:, 1] & 0xffffffff).astype(np.uint32)
        ext = [-(1 << 14), 1 << 14, 0, -1, 1, 16383, -16383]
        edges = np.array([[p & 0xffffffff, q & 0xffffffff, 0] for p in ext for q in ext], np.uint32)
    elif name == "pk_absdiff_i16":
        # int16 lanes whose difference fits int16 (the kernel's |Jp - Ip| <= 8160): both lanes of both operands from
        # [-2^14, 2^14 - 1]; the edge rows hold +-2^14, 0 and equal operands in every lane combination
        v = rng.integers(-(1 << 14), 1 << 14, (N_RAW, 4))
        r[:, 0], r[:, 1] = _pack16(v[:, 0], v[:, 1]), _pack16(v[:, 2], v[:, 3])
        ext = [-(1 << 14), 1 << 14, 0, (1 << 14) - 1, -1, 1, 8160, -8160]
        edges = np.array([[int(_pack16(p, q)), int(_pack16(u, v_)), 0] for p in ext for q in ext for u in ext for v_ in ext], np.uint32)
    return np.ascontiguousarray(np.concatenate([edges.astype(np.uint32), r]))


# ---------------------------------------------------------------------------------------------
# vo_svd_wide.h
def _epnp_shaped(rng):
    """M^T M with M's sparsity: rows (a fu, 0, a (uc - u)) / (0, a fv, a (vc - v)) per control point"""
    M = np.zeros((10, 12))
    al = rng.normal(0.25, 0.6, (5, 4))
    uv = rng.uniform(0, 1241, (5, 2)) * [1, 0.3]
    for p in range(5):
        for q in range(4):
            M[2 * p, 3 * q] = al[p, q] * 718.856
            M[2 * p, 3 * q + 2] = al[p, q] * (607.19 - uv[p, 0])
            M[2 * p + 1, 3 * q + 1] = al[p, q] * 718.856
            M[2 * p + 1, 3 * q + 2] = al[p, q] * (185.2 - uv[p, 1])
    return M.T @ M


def svd12_matrices():
    """14 EPnP-shaped M^T M (rank 10), 4 full-rank, one with zero rows and columns, the zero matrix, the identity"""
    rng = np.random.default_rng(7)
    mats = []
    for _ in range(14):
        mats.append(_epnp_shaped(rng))
    for _ in range(4):
        A = rng.normal(size=(12, 12))
        mats.append(A @ A.T)
    Z = rng.normal(size=(12, 12))
    Z[3] = 0
    Z[:, 3] = 0
    Z[7] = 0
    Z[:, 7] = 0
    mats += [(Z + Z.T) / 2 + 12 * np.diag((np.arange(12) % 4 != 3).astype(float)), np.zeros((12, 12)), np.eye(12)]
    return np.ascontiguousarray(np.array(mats), np.float64)


def svd12_matrices_more():
    """svd12_matrices() (the first matrix stays the first), 256 more EPnP-shaped ones, a diagonal matrix already in sorted order
    (no pair ever rotates: the speculative next sweep takes its early exit), a matrix with two exactly equal rows (one
    rotation leaves an exactly zero row: the pseudo-random fill of jacobi_finish)"""
    rng = np.random.default_rng(70)
    more = [_epnp_shaped(rng) for _ in range(256)]
    more.append(np.diag(np.arange(12.0, 0.0, -1.0)))
    A = rng.normal(size=(12, 12))
    A[9] = A[4]
    more.append(A)
    return np.ascontiguousarray(np.concatenate([svd12_matrices(), np.array(more)]), np.float64)


def solve6_systems():
    """A: n x 6 x 6, b: n x 6 -- 40 normal matrices of projection Jacobians with a scaled diagonal, an ill-conditioned, a
    singular and the zero system"""
    rng = np.random.default_rng(11)
    As, bs = [], []
    for _ in range(40):
        J = rng.normal(size=(rng.integers(8, 400), 6)) * [300, 300, 300, 40, 40, 8]
        A = J.T @ J
        A[np.diag_indices(6)] *= 1 + 10.0 ** rng.integers(-8, 2)
        As.append(A)
        bs.append(J.T @ rng.normal(size=len(J)))
    H = np.vander(np.linspace(1, 2, 6), 6)
    As += [H.T @ H, np.diag([4.0, 3.0, 0.0, 2.0, 0.0, 1.0]), np.zeros((6, 6))]
    bs += [np.ones(6), np.arange(6.0), np.ones(6)]
    return np.ascontiguousarray(np.array(As), np.float64), np.ascontiguousarray(np.array(bs), np.float64)


def epnp_split_sets(orc):
    """X: 28 x 5 x 3, U: 28 x 5 x 2 (f32), K: noisy, exact, far and near-planar 5-point sets"""
    rng = np.random.default_rng(21)
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)
    X, U = [], []
    for case in range(28):
        lo, hi = ([-8, -2, 4], [8, 2, 40]) if case % 4 else ([-30, -6, 60], [30, 6, 200])
        xyz = rng.uniform(lo, hi, (5, 3)).astype(np.float32)
        if case % 7 == 3:
            xyz[:, 2] = xyz[0, 2] + rng.normal(0, 0.01, 5).astype(np.float32)  # almost fronto-parallel plane
        rv, tv = rng.normal(0, 0.02, 3), rng.normal(0, 0.5, 3)
        uv = orc.project_points(xyz, rv, tv, K) + (rng.normal(0, 0.4, (5, 2)) if case % 3 else 0)
        X.append(xyz)
        U.append(uv.astype(np.float32))
    return np.ascontiguousarray(np.array(X, np.float32)), np.ascontiguousarray(np.array(U, np.float32)), K


# ---------------------------------------------------------------------------------------------
# row_ordered_sum<N> / row_ordered_sum_x2<N>: one value per lane of a wavefront
def serial_sum(v):
    """((0 + v_0) + v_1) + ... in f64, along the last axis"""
    s = np.zeros(v.shape[:-1], np.float64)
    for k in range(v.shape[-1]):
        s = s + v[..., k]
    return s


def other_order_sums(v):
    """the same terms summed in three other orders: reversed, pairwise tree, sorted by value"""
    def tree(t):
        while t.shape[-1] > 1:
            if t.shape[-1] % 2:
                t = np.concatenate([t, np.zeros(t.shape[:-1] + (1,))], -1)
            t = t[..., 0::2] + t[..., 1::2]
        return t[..., 0]
    return serial_sum(v[..., ::-1]), tree(v), serial_sum(np.sort(v, -1))


def _order_sensitive_terms(rng, n):
    """n terms, magnitudes over 40 binades, mixed signs, with cancelling giants in between, for which the serial sum differs IN ITS
    BITS from the reversed, the pairwise and the sorted sum (checked here, with numpy: a set no order can tell apart tests
    nothing)"""
    while True:
        v = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-21, 21, n) * rng.uniform(1, 2, n)
        i, j = rng.choice(n, 2, replace=False)
        v[j] = -v[i] * (1 + rng.integers(-2, 3) * 2.0 ** -30)
        s = serial_sum(v)
        if all(o.view(np.uint64) != s.view(np.uint64) for o in other_order_sums(v)):
            return v


def row_sum_sets(n_cases=48):
    """n_cases x 4 (x6, y6, x12, y12) x 64 lanes: a different order-sensitive set in every DPP row, NaN in lanes N .. 15 of
    every row (those lanes must never enter a sum)"""
    rng = np.random.default_rng(16)
    out = np.full((n_cases, 4, 4, 16), np.nan)
    for c in range(n_cases):
        for a, n in enumerate((6, 6, 12, 12)):
            for row in range(4):
                out[c, a, row, :n] = _order_sensitive_terms(rng, n)
    # the hand-made one: every partial sum of the serial order is exact or rounds in a known way
    out[0, 0, 0, :6] = [1e16, 1, -1e16, 3, 2.0 ** -30, -2.0 ** -31]
    out[0, 2, 0, :12] = [1e16, 1, -1e16, 3, 2.0 ** -30, 1e-8, 2.0 ** 60, -5, 1, 2.0 ** -60, -2.0 ** 60, 7.5]
    return np.ascontiguousarray(out.reshape(n_cases, 4, 64))


def row_sum_terms(sets):
    """the terms that enter the sums, per DPP row: x6, y6 (n, 4 rows, 6), x12, y12 (n, 4 rows, 12)"""
    v = sets.reshape(len(sets), 4, 4, 16)
    return v[:, 0, :, :6], v[:, 1, :, :6], v[:, 2, :, :12], v[:, 3, :, :12]


# ---------------------------------------------------------------------------------------------
# pose headers: scenes of a KITTI-like camera (no oracle needed: these are inputs only)
def _rot(rv):
    rv = np.asarray(rv, np.float64)
    th = np.linalg.norm(rv)
    if th < 1e-300:
        return np.eye(3)
    k = rv / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _project(X, rv, t, K):
    Xc = X.astype(np.float64) @ _rot(rv).T + t
    return np.stack([K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]], 1)


def pnp_sets(n_pts, n_sets, seed):
    """n_sets records (xyz f32 [n_pts][3] | uv f32 [n_pts][2] | K f32 [9]): near and far, noisy and exact, near-planar sets"""
    rng = np.random.default_rng(seed)
    K = K_KITTI
    rec = []
    for case in range(n_sets):
        lo, hi = ([-8, -2, 4], [8, 2, 40]) if case % 4 else ([-30, -6, 60], [30, 6, 200])
        xyz = rng.uniform(lo, hi, (n_pts, 3)).astype(np.float32)
        if case % 7 == 3:
            xyz[:, 2] = xyz[0, 2] + rng.normal(0, 0.01, n_pts).astype(np.float32)
        rv, tv = rng.normal(0, 0.02, 3), rng.normal(0, 0.5, 3)
        uv = _project(xyz, rv, tv, K) + (rng.normal(0, 0.4, (n_pts, 2)) if case % 3 else 0)
        rec.append(np.concatenate([xyz.ravel(), uv.astype(np.float32).ravel(), K.ravel()]))
    return np.ascontiguousarray(np.array(rec, np.float32))


def deg4_coefficients():
    """quartics with four real, two real and no real roots, scaled; degree drops (a = 0, a = b = 0); a double root"""
    rng = np.random.default_rng(51)
    c = []
    for _ in range(400):
        r = rng.uniform(-3, 3, 4)
        if rng.random() < 0.5:
            p = np.poly1d([1, -2 * r[0], r[0] ** 2 + abs(r[1]) + 0.1]) * np.poly1d(np.poly(r[2:]))
        else:
            p = np.poly1d(np.poly(r))
        c.append(p.coeffs * rng.uniform(0.5, 2.0))
    c += [[1, -10, 35, -50, 24], [0, 1, -6, 11, -6], [0, 0, 1, -3, 2], [1, -4, 6, -4, 1], [1, 0, 2, 0, 1], [1, 0, 0, 0, 0], [0, 0, 0, 0, 1]]
    return np.ascontiguousarray(np.array(c, np.float64))


def rotation_vectors():
    rng = np.random.default_rng(52)
    r = [rng.normal(0, 0.5, 3) for _ in range(1000)] + [rng.normal(0, 1e-9, 3) for _ in range(20)]
    r += [np.zeros(3), [np.pi, 0, 0], [0, np.pi - 1e-9, 0], [1e-200, 0, 0], [3.0, 0.5, -0.2], [4.0, -3.0, 2.0], [2 * np.pi, 0, 0]]
    return np.ascontiguousarray(np.array(r, np.float64))


def rotation_matrices():
    """the matrices of rotation_vectors() as numpy forms them (any near-rotation is a valid operand), and the exact half turns"""
    R = [_rot(r) for r in rotation_vectors()]
    R += [np.eye(3), np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1]), np.array([[0.0, 1, 0], [1, 0, 0], [0, 0, -1]])]
    return np.ascontiguousarray(np.array(R, np.float64).reshape(-1, 9))


def triangulation_records():
    """Pl[12], Pr[12], xl, yl, xr, yr (f32) over the KITTI rig: disparities 0.5 .. 120 px, a fraction of a pixel of row noise"""
    rng = np.random.default_rng(1)
    n = 2000
    Pl = np.array([[718.856, 0, 607.1928, 0], [0, 718.856, 185.2157, 0], [0, 0, 1, 0]], np.float32)
    Pr = Pl.copy()
    Pr[0, 3] = -386.1448
    pl = rng.uniform([0, 0], [1241, 376], (n, 2)).astype(np.float32)
    pr = pl.copy()
    pr[:, 0] -= rng.uniform(0.5, 120, n).astype(np.float32)
    pr[:, 1] += rng.normal(0, 0.3, n).astype(np.float32)
    rec = np.concatenate([np.tile(Pl.ravel(), (n, 1)), np.tile(Pr.ravel(), (n, 1)), pl, pr], 1)
    return np.ascontiguousarray(rec, np.float32)


def two_view_scene(seed, n=40):
    rng = np.random.default_rng(seed)
    R = _rot(np.random.default_rng(100 + seed).normal(0, 0.03, 3))
    t = np.r_[np.random.default_rng(200 + seed).normal(0, 0.2, 2), 1.0]
    t = t / np.linalg.norm(t)
    X = np.c_[rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(5, 40, n)]
    x1 = X[:, :2] / X[:, 2:]
    X2 = X @ R.T + t
    x2 = X2[:, :2] / X2[:, 2:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    return R, t, x1, x2, E / np.linalg.norm(E)


def essential_records():
    """five_point: q1[10], q2[10]; sampson: E[9], x1, x2; decompose: E[9]; cheirality: P[12], x1, x2, dist -- from 24 two-view
    scenes (8 groups of five correspondences each), exact and with a pixel's worth of noise, and a pure rotation"""
    five, samp, dec, che = [], [], [], []
    rng = np.random.default_rng(53)
    for seed in range(24):
        R, t, x1, x2, E = two_view_scene(seed)
        if seed % 3 == 2:
            x2 = x2 + rng.normal(0, 1e-3, x2.shape)
        for g in range(8):
            five.append(np.r_[x1[5 * g:5 * g + 5].ravel(), x2[5 * g:5 * g + 5].ravel()])
        dec.append(E.ravel())
        dec.append((E + rng.normal(0, 1e-3, (3, 3))).ravel())
        for i in range(40):
            samp.append(np.r_[E.ravel(), x1[i], x2[i]])
            for P in (np.c_[R, t], np.c_[R, -t]):
                che.append(np.r_[P.ravel(), x1[i], x2[i], 50.0])
    R, t, x1, x2, E = two_view_scene(99)
    five.append(np.r_[x1[:5].ravel(), x1[:5].ravel()])     # no motion at all
    as64 = lambda a: np.ascontiguousarray(np.array(a, np.float64))
    return as64(five), as64(samp), as64(dec), as64(che)


# ---------------------------------------------------------------------------------------------
# tests/host_check/device_check.hip: its inputs (one file of raw records per operation), its build and its outputs
OUT_TYPES = {"math_cbrt": ("f8", 1), "math_acos": ("f8", 1), "math_cos": ("f8", 1), "math_sin": ("f8", 1), "math_lambda": ("f8", 1),
             "epnp5": ("f8", 6), "p3p4": ("f8", 7), "p3p_deg4": ("f8", 5), "rodrigues_v2m": ("f8", 36), "rodrigues_m2v": ("f8", 3),
             "triangulate": ("f4", 3), "five_point": ("f8", 91), "sampson": ("f4", 1), "decompose": ("f8", 21), "cheirality": ("i4", 1),
             "solve6": ("f8", 6), "svd12": ("f8", 156), "lk_bilinear7_u8": ("i2", 7), "lk_blend7": ("i2", 7),
             "lk_bilinear7_deriv": ("i2", 14), "lk_diff_dot": ("i4", 1), "lk_scharr4": ("u4", 1),
             "svd12_wide": ("f8", 144), "solve6_wave1": ("f8", 6), "solve6_wave4": ("f8", 6), "row_sums": ("f8", 768),
             "epnp_split": ("f8", 6)}
OUT_TYPES.update({"lk_" + w: ("u4", 1) for w in LK_RAW})
DEVICE_ONLY = ["svd12_wide", "solve6_wave1", "solve6_wave4", "row_sums", "epnp_split", "fast_pair"]
ROW_SUMS_SENTINEL = -7.0
FAST_PAIR_TUPLES = 8


def _bytes(*parts):
    """records of mixed type: the parts' rows side by side as bytes"""
    return np.ascontiguousarray(np.concatenate([np.ascontiguousarray(p).view(np.uint8).reshape(len(p), -1) for p in parts], 1))


def device_check_inputs():
    """operation -> array of records (one row each), for every operation of device_check.hip"""
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    ins = {"math_cbrt": f64(np.concatenate([cbrt_args(), CBRT_EDGES])),
           "math_acos": f64(np.concatenate([acos_args(), ACOS_EDGES])),
           # (the bit-exact sets first, the non-finite arguments -- compared by class -- are the last three)
           "math_cos": f64(np.concatenate([cos_args(), trig_large_args(), TRIG_NONFINITE])),
           "math_sin": f64(np.concatenate([sin_args(), -sin_args(), trig_large_args(), TRIG_NONFINITE])),
           "math_lambda": lm_lambda_args()}
    ins["epnp5"] = np.concatenate([pnp_sets(5, 28, 21), pnp_sets(5, 300, 0)])
    ins["epnp_split"] = ins["epnp5"]
    ins["p3p4"] = pnp_sets(4, 300, 31)
    ins["p3p_deg4"] = deg4_coefficients()
    ins["rodrigues_v2m"] = rotation_vectors()
    ins["rodrigues_m2v"] = rotation_matrices()
    ins["triangulate"] = triangulation_records()
    ins["five_point"], ins["sampson"], ins["decompose"], ins["cheirality"] = essential_records()
    A, b = solve6_systems()
    ins["solve6"] = np.ascontiguousarray(np.concatenate([A.reshape(len(A), 36), b], 1))
    ins["solve6_wave1"] = ins["solve6_wave4"] = ins["solve6"]
    ins["svd12"] = svd12_matrices_more().reshape(-1, 144)
    ins["svd12_wide"] = ins["svd12"]
    ins["row_sums"] = row_sum_sets().reshape(-1, 256)
    for w in LK_RAW:
        ins["lk_" + w] = lk_raw_operands(w)
    top, bot, w = bilinear_operands()
    ins["lk_bilinear7_u8"] = ins["lk_blend7"] = _bytes(top, bot, w)
    dx, dy, packed, w = deriv_operands()
    ins["lk_bilinear7_deriv"] = _bytes(packed[0], packed[1], w)
    ins["lk_diff_dot"] = _bytes(*diff_dot_operands())
    ins["lk_scharr4"] = scharr_patches()
    ins["fast_pair"] = np.array([[FAST_PAIR_TUPLES]], np.int32)
    return ins


def write_inputs(directory, ins):
    import os
    for name, a in ins.items():
        np.ascontiguousarray(a).tofile(os.path.join(directory, name + ".in"))


def read_outputs(directory, ins, names):
    import os
    outs = {}
    for name in names:
        raw = np.fromfile(os.path.join(directory, name + ".out"), np.uint8)
        if name == "fast_pair":
            outs[name] = raw
            continue
        t, k = OUT_TYPES[name]
        a = raw.view(np.dtype(t)).reshape(-1, k)
        assert len(a) == len(ins[name]), (name, len(a), len(ins[name]))
        outs[name] = a
    return outs


def build_device_check(out_dir):
    """hipcc with the product's flags (visual_odom_amd/build.py FLAGS without what only a shared object needs): returns the
    program's path and the build's wall time in seconds"""
    import os
    import subprocess
    import time
    from visual_odom_amd.build import FLAGS, HIPCC
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "host_check", "device_check.hip")
    exe = os.path.join(out_dir, "device_check")
    t0 = time.time()
    subprocess.check_call([HIPCC] + [f for f in FLAGS if f != "-fPIC"] + ["-o", exe, src])
    return exe, time.time() - t0


def host_reference(host_check, ins, name):
    """the g++ build of the same entry point (host_check.cpp: hc_case) over the same records"""
    import ctypes as C
    t, k = OUT_TYPES[name]
    a = np.ascontiguousarray(ins[name])
    sizes = (C.c_int * 2)()
    assert host_check.hc_case_sizes(name.encode(), sizes) == 0, name
    n = len(a)
    assert a.nbytes == n * sizes[0] and np.dtype(t).itemsize * k == sizes[1], (name, a.nbytes, n, list(sizes))
    out = np.zeros((n, k), np.dtype(t))
    assert host_check.hc_case(name.encode(), a.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def first_difference(name, got, want, operands=None):
    """None if got and want hold the same bits (NaN payloads included); else a message naming the operation, the first differing
    case, its operands and both results in hex"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape)
    u = np.dtype("u%d" % g.dtype.itemsize)
    gb, wb = g.view(u).reshape(len(g), -1), w.view(u).reshape(len(w), -1)
    bad = np.nonzero((gb != wb).any(1))[0]
    if len(bad) == 0:
        return None
    i = int(bad[0])
    j = int(np.nonzero(gb[i] != wb[i])[0][0])
    msg = "%s: %d of %d cases differ; first: case %d, output %d: got %#x want %#x" % (name, len(bad), len(g), i, j, gb[i, j], wb[i, j])
    if operands is not None:
        op = np.ascontiguousarray(operands)[i]
        msg += "; operands " + (" ".join("%#x" % v for v in op.view(np.dtype("u%d" % op.dtype.itemsize)).ravel()[:16]))
    return msg
