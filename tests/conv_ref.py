"""Float64 reference of ONE launch of the conv front end (aprilx_run_conv_front): values, a tolerance per element, exact parts.

Plain numpy, written from the contract in the comment above conv12_kernel (csrc/kernels_misc.hip), not from the kernel bodies:

    x[m]    = the chunk of row m, [seg][mel]: given directly, or rows (tail[m] + r) mod ring_frames, r = 0 .. seg - 1, of slot
              slot_idx[m] of the feature ring [slots][ring_frames][mel]
    act1    = DoubleSwish(Conv2d(1 -> c0, 3 x 3, stride s0)(x) + b0)            DoubleSwish(y) = y sigma(y - 1)
    act2    = DoubleSwish(Conv2d(c0 -> c1, 3 x 3, stride s1)(act1) + b1)        no padding anywhere
    A3[m W3 + ow][ci 9 + i 3 + j] = act2[m][ci][i][ow s2 + j]                   i, j = 0, 1, 2: the im2col rows of the third conv

H2 is 3, or 4 where the third conv's stride still leaves one output row; rows i >= 3 of act2 are then computed and never read.
Every conv output is one fp32 chain over input channel, kernel row, kernel column, the bias added last.

Tolerance (per element of A3, the rules of tests/gemm_ref.py and nothing else)
------------------------------------------------------------------------------
    tol(y1)   = lin_factor(9) sum |x| |w0|                                      (x is exact: it is copied)
    act1      : gemm_ref.dswish_of(y1, tol(y1)) -- the EPI_BIAS_DSWISH expression 2 |dv/dy| tol_y + 4 hw; hw holds the bias add's
                rounding U |sum + bias|, so it is not added a second time
    tol(y2)   = lin_factor(9 c0) sum |act1| |w1|  +  sum |w1| tol(act1)         (the second term: the error carried in)
    act2      : dswish_of(y2, tol(y2))
    flush floor, both activations: + 2^-126 (1 + |y|) absolute.  A result below the smallest normal fp32 number may be flushed to
    zero, and DoubleSwish has two results that get there: the product y sigma (2^-126 absolute), and sigma itself, whose flush the
    product carries as |y| 2^-126 like any other error of sigma.  For y - 1 below -88.7 the true sigma is under 2^-128 while the
    written formula rcp(1 + exp2(..)) gives exactly 0 on any fp32 machine (exp2 overflows to inf; just above, the reciprocal is a
    denormal), so the computed activation is 0 where the true one is up to 89 x 2^-128 = 22 x 2^-126: with the floor at the product
    alone, the fp32 emulation of tests/test_conv_ref_cpu.py itself lies outside the tolerance by up to that factor (measured: 18.9; the kernels: 55.2)
    on the saturating case (weights x 4), which lives there.  The term is at most 2.4e-36 anywhere.

Exact parts: columns [9 c1, ldo) and rows >= M W3 keep the 0xFF fill; w0t / w1t are the numpy transposes bit for bit; im2col copies
bits, so an act2 value that appears at several (ow, j) must have the same bits everywhere (A3 is a gather of ONE act2 array).

`mut` names a deliberate error of the reference (tests/test_conv_ref_cpu.py: each must land outside the tolerance).
"""
import hashlib
import math

import numpy as np

import gemm_ref as R
from gemm_ref import lin_factor, dswish_of, err_ratio, bits, pattern

FLUSH = 2.0 ** -126
MUTANTS = ("swap_rc", "stride_origin", "ci_off", "no_bias", "sig_y", "wrap_off", "no_slot", "k_order")

# (seg, mel, strides, c0, c1) and what it reaches in the kernels (tests/conv_front_worker.py path_of)
GEOMETRIES = [
    (9, 80, (1, 2, 2), 8, 32),       # the product's shape: NP 114, two channel subsets side by side
    (9, 80, (1, 2, 2), 8, 12),       # 6 channels per workgroup, 3 per thread
    (9, 40, (1, 2, 2), 8, 16),       # NP 54: four channel subsets
    (9, 40, (1, 2, 2), 8, 12),       # three
    (9, 128, (1, 2, 2), 8, 32),      # NP 186: one subset of 192 positions
    (9, 200, (1, 2, 2), 4, 8),       # NP 294: more positions than threads, the multi-pass loop
    (11, 80, (1, 2, 2), 8, 32),      # H2 = 4
    (19, 80, (2, 2, 2), 8, 32),      # H2 = 4, s0 = 2
    (15, 50, (2, 2, 1), 8, 32),      # s2 = 1
    (7, 24, (1, 1, 1), 4, 7),        # all strides 1, a prime channel count: 7 per workgroup
    (9, 11, (1, 2, 2), 8, 8),        # W3 = 1
    (9, 48, (1, 2, 2), 8, 32),       # NP 66: the many-chunk form's lower edge
    (9, 49, (1, 2, 2), 8, 32),       # NP 69, odd widths
    (9, 89, (1, 2, 2), 8, 32),       # NP 129: just outside the many-chunk form
    (10, 64, (1, 2, 2), 8, 32),      # the many-chunk form with H1 = 8
]


class Spec(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def out_size(n, s):
    return (n - 3) // s + 1


def geometry(seg, mel, strides, c0, c1):
    """Sizes after each conv, the second conv's channels per workgroup of the grouped form (the largest divisor of c1 that is <= 8)
    and that form's dynamic shared memory, 4 (seg mel + c0 H1 W1 + cg H2 W2) bytes."""
    H1, W1 = out_size(seg, strides[0]), out_size(mel, strides[0])
    H2, W2 = out_size(H1, strides[1]), out_size(W1, strides[1])
    H3, W3 = out_size(H2, strides[2]), out_size(W2, strides[2])
    assert min(seg, mel, H1, W1, H2, W2) >= 3 and H3 == 1
    cg = max(k for k in range(1, 9) if c1 % k == 0)
    return Spec(H1=H1, W1=W1, H2=H2, W2=W2, W3=W3, NP=H2 * W2, cg=cg, lds=4 * (seg * mel + c0 * H1 * W1 + cg * H2 * W2))


def spec(name, geo, M, mode="rand", ring=None, seed=0):
    """mode: rand (x ~ U(-16, 8)) | floor (some frames constant -15.94, the log-mel floor; the first chunk all of them) | sat (weights
    x 4).  ring: None (x given chunk by chunk) or ring_frames."""
    seg, mel, strides, c0, c1 = geo
    s = Spec(name=name, seg=seg, mel=mel, strides=tuple(strides), c0=c0, c1=c1, M=M, mode=mode, ring=ring, seed=seed)
    s.update(geometry(seg, mel, strides, c0, c1))
    s.ldo = (9 * c1 + 63) // 64 * 64                     # K of the third conv's GEMM, as the engine lays the rows out
    s.out_rows = M * s.W3 + 3
    s.slots = M + 2 if ring else 0
    s.ring_frames = ring if ring else 32 * seg
    return s


class Case:
    def __init__(self, s):
        f32 = np.float32
        self.spec = s
        rng = np.random.default_rng([s.seed, R.hash_name(s.name)])
        uni = lambda shape, fan: (rng.uniform(-1.0, 1.0, shape) / math.sqrt(fan)).astype(f32)       # as synth_model draws them
        gain = f32(4.0 if s.mode == "sat" else 1.0)
        self.w0, self.b0 = uni((s.c0, 3, 3), 9) * gain, uni((s.c0,), 9) * gain
        self.w1, self.b1 = uni((s.c1, s.c0, 3, 3), 9 * s.c0) * gain, uni((s.c1,), 9 * s.c0) * gain
        self.x = self.ring = self.slot_idx = self.tail = None
        if s.ring:
            Rf = s.ring_frames
            self.ring = rng.uniform(-16.0, 8.0, (s.slots, Rf, s.mel)).astype(f32)
            self.slot_idx = R.injective(rng, s.M, s.slots)
            tails = [0, Rf - s.seg, Rf - s.seg + 1, Rf - 1]
            self.tail = np.array([tails[m % 4] for m in range(s.M)], np.int32)
            if s.M >= 3:                                  # one slot named by two rows, at different tails (rows 0 and 2)
                self.slot_idx[2] = self.slot_idx[0]
                assert self.tail[2] != self.tail[0] or Rf == s.seg
            self.tail = self.tail % Rf
        else:
            self.x = rng.uniform(-16.0, 8.0, (s.M, s.seg, s.mel)).astype(f32)
            if s.mode == "floor":
                self.x[rng.uniform(size=(s.M, s.seg)) < 0.5] = f32(-15.94)
                self.x[0] = f32(-15.94)


# ------------------------------------------------------------------ the mathematics
def gather(s, c, mut=None):
    """[M][seg][mel] float64: the chunk of every row."""
    if c.x is not None:
        return c.x.astype(np.float64)
    Rf = s.ring_frames
    r = c.tail[:, None].astype(np.int64) + np.arange(s.seg)[None, :]
    idx = r % Rf
    if mut == "wrap_off":                                 # the rows behind the ring's end come from one row further on
        idx = np.where(r >= Rf, (r - Rf + 1) % Rf, r)
    slot = np.arange(s.M) if mut == "no_slot" else c.slot_idx
    return c.ring[slot[:, None], idx].astype(np.float64)


def patches(a, stride, Ho, Wo, origin_stride=None):
    """a [M][C][H][W] -> [M][C][9][Ho][Wo]: element (i, j) of the 3 x 3 patch whose origin is (oh, ow) x origin_stride."""
    so = stride if origin_stride is None else origin_stride
    return np.stack([a[:, :, i:i + so * (Ho - 1) + 1:so, j:j + so * (Wo - 1) + 1:so] for i in range(3) for j in range(3)], axis=2)


def stage(a, tol_a, w, b, stride, Ho, Wo, mut, sigma_floor=True):
    """One conv + DoubleSwish: a [M][C][H][W] with tolerance tol_a (or None: exact), w [O][C][3][3] -> (act, tol) [M][O][Ho][Wo]."""
    C = a.shape[1]
    w64 = w.astype(np.float64).reshape(w.shape[0], C, 3, 3)
    if mut == "swap_rc":
        w64 = w64.transpose(0, 1, 3, 2)
    wk = w64.reshape(w.shape[0], C, 9)
    origin = 1 if (mut == "stride_origin" and C > 1) else None
    if mut == "ci_off" and C > 1:
        a = np.roll(a, -1, axis=1)
    P = patches(a, stride, Ho, Wo, origin)
    y = np.einsum("ock,mckhw->mohw", wk, P)
    T = np.einsum("ock,mckhw->mohw", np.abs(wk), np.abs(P))
    tol_y = lin_factor(9 * C) * T
    if tol_a is not None:
        tol_y = tol_y + np.einsum("ock,mckhw->mohw", np.abs(wk), patches(tol_a, stride, Ho, Wo, origin))
    if not (mut == "no_bias" and C > 1):
        y = y + b.astype(np.float64)[None, :, None, None]
    v, tol = dswish_of(y, tol_y, 0.0 if mut == "sig_y" else 1.0)
    return v, tol + FLUSH * (1.0 + (np.abs(y) if sigma_floor else 0.0))


def im2col(s, act2, mut=None):
    """act2 [M][c1][H2][W2] -> [M W3][9 c1]"""
    cols = (np.arange(s.W3)[:, None] * s.strides[2] + np.arange(3)[None, :])                       # [ow][j]
    g = act2[:, :, :3, :][:, :, :, cols]                                                            # [M][c1][i][ow][j]
    g = g.transpose(0, 3, 1, 4, 2) if mut == "k_order" else g.transpose(0, 3, 1, 2, 4)              # [M][ow][ci][i][j]
    return g.reshape(s.M * s.W3, 9 * s.c1)


def evaluate(s, c, mut=None, sigma_floor=True):
    """(A3 values, A3 tolerances), float64 [M W3][9 c1].  sigma_floor=False: the flush floor at the product alone (a figure the
    worker prints beside the saturating cases; nothing is judged with it)."""
    with np.errstate(over="ignore", under="ignore"):
        x = gather(s, c, mut)[:, None]
        a1, t1 = stage(x, None, c.w0[:, None], c.b0, s.strides[0], s.H1, s.W1, mut, sigma_floor)
        a2, t2 = stage(a1, t1, c.w1, c.b1, s.strides[1], s.H2, s.W2, mut, sigma_floor)
    return im2col(s, a2, mut), im2col(s, t2)


def transposes(c):
    """w0t [9][c0], w1t [c0 9][c1]"""
    c0, c1 = c.w0.shape[0], c.w1.shape[0]
    return np.ascontiguousarray(c.w0.reshape(c0, 9).T), np.ascontiguousarray(c.w1.reshape(c1, c0 * 9).T)


# ------------------------------------------------------------------ fp32 emulation of the stated chain (CPU tests)
def emulate32(s, c):
    """A3 as an fp32 machine computes it: per output one chain over input channel, kernel row, kernel column with the product and
    the sum rounded separately, the bias added last, DoubleSwish in fp32."""
    f32 = np.float32

    def conv32(a, w, b, stride, Ho, Wo):
        P = patches(a, stride, Ho, Wo)
        acc = np.zeros((a.shape[0], w.shape[0], Ho, Wo), f32)
        for ci in range(a.shape[1]):
            for k in range(9):
                prod = (P[:, ci, k][:, None] * w[None, :, ci, k // 3, k % 3][:, :, None, None]).astype(f32)
                acc = (acc + prod).astype(f32)
        y = (acc + b[None, :, None, None]).astype(f32)
        with np.errstate(over="ignore", under="ignore"):
            sg = (f32(1.0) / (f32(1.0) + np.exp(-(y - f32(1.0)), dtype=f32))).astype(f32)
        return (y * sg).astype(f32)

    x = gather(s, c).astype(f32)[:, None]
    a1 = conv32(x, c.w0[:, None], c.b0, s.strides[0], s.H1, s.W1)
    a2 = conv32(a1, c.w1, c.b1, s.strides[1], s.H2, s.W2)
    return im2col(s, a2)


# ------------------------------------------------------------------ where the values land, and the comparison
def render(s, A3):
    out = pattern((s.out_rows, s.ldo), np.float32)
    out[:s.M * s.W3, :9 * s.c1] = A3.astype(np.float32)
    return out


def duplicates_agree(s, out):
    """im2col copies bits: rebuild act2[m][ci][i][col] from the first (ow, j) that shows it and gather it again."""
    b = bits(np.ascontiguousarray(out[:s.M * s.W3, :9 * s.c1])).reshape(s.M, s.W3, s.c1, 3, 3)                    # [m][ow][ci][i][j]
    act = np.zeros((s.M, s.c1, 3, s.W2), np.uint32)
    for ow in reversed(range(s.W3)):
        for j in reversed(range(3)):
            act[:, :, :, ow * s.strides[2] + j] = b[:, ow, :, :, j]
    cols = (np.arange(s.W3)[:, None] * s.strides[2] + np.arange(3)[None, :])
    again = act[:, :, :, cols].transpose(0, 3, 1, 2, 4)
    return bool(np.array_equal(again, b))


def compare(s, c, ev, out, w0t=None, w1t=None):
    """-> dict(ratio = worst err / tol (inf for a NaN or a stray write), at, fill, dup, transposes): a case passes with ratio <= 1 and the rest True."""
    val, tol = ev
    out = np.asarray(out).reshape(s.out_rows, s.ldo)
    n, w = s.M * s.W3, 9 * s.c1
    got = out[:n, :w].astype(np.float64)
    ratio = err_ratio(np.abs(got - val), tol)
    ratio[~np.isfinite(got)] = np.inf
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    stray = bits(out) != bits(pattern(out.shape, np.float32))
    stray[:n, :w] = False
    res = dict(ratio=float(ratio[at]), at=tuple(int(i) for i in at), fill=not stray.any(), dup=duplicates_agree(s, out), transposes=True)
    if w0t is not None:
        e0, e1 = transposes(c)
        res["transposes"] = bool(np.array_equal(bits(np.asarray(w0t).reshape(e0.shape)), bits(e0)) and np.array_equal(bits(np.asarray(w1t).reshape(e1.shape)), bits(e1)))
    return res


def passes(res):
    return res["ratio"] <= 1.0 and res["fill"] and res["dup"] and res["transposes"]


def digest(out):
    return hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()
