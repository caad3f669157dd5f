"""Float64 reference of ONE GEMM launch (aprilx_run_gemm): layouts, epilogues, tolerance, comparison.

Plain numpy.  Nothing here is taken from csrc except what kernels.h and gemm_plan.h state in words: the two packed weight orders,
the epilogue formulas, the enumerators.  tests/test_gemm_ref_cpu.py checks this module against itself (round trips, an fp32
emulation of the canonical summation order, perturbations that must be rejected); tests/gemm_launch_worker.py compares the
kernels with it.

Tolerance (per output element, never a constant)
------------------------------------------------
Linear part.  A sum of K fp32 products, whatever its order, is judged with the probabilistic rounding bound with a factor of 4,

    tol_lin = 4 sqrt(K) 2^-24 sum_k |a_k| |w_k|        (a segment that is multiplied by a row scale is weighted by |scale|)

and never more than the worst-case bound (K + 8) 2^-23 sum |a| |w| that any fp32 accumulation meets (the factor 4 sqrt(K) 2^-24 is
below (K + 8) 2^-23 for every K; lin_factor() asserts it).  How the MFMA units round inside one instruction is not known; the
factor of 4 is for that.  With binary16 operands (wt == 1) the reference first rounds A and W to binary16 (round to nearest even,
numpy's astype), so the products are the ones the kernel forms and the same bound judges the fp32 accumulation.

Through an epilogue.  out = f(sums).  tol = 2 sum_j |df/ds_j| tol_lin_j + 4 hw, where the derivatives are the analytic ones of the
float64 epilogue and hw is the first-order bound of what the written fp32 formulas add:

  * every fp32 add / multiply: relative 2^-24 of its result (u below);
  * the CDNA ISA manual states 1 ulp for v_exp_f32, v_rcp_f32 and v_rsq_f32, i.e. relative 2^-23 = 2 u each;
  * fast_sigmoid(x) = rcp(1 + exp2(-1.4427 x)): the argument t = -1.4427 x carries two roundings (the constant, the product),
    2 u |t| absolute, which exp2 turns into relative ln2 |t| 2 u = 2 u |x|; exp2 itself 2 u; sigma depends on e = exp2(t) with
    relative sensitivity e / (1 + e) = 1 - sigma; the add 1 + e gives u, rcp 2 u:
        rel(sigma) <= 2 u ((1 - sigma)(1 + |x|) + 1.5)                                      (sig_rel)
  * fast_tanh(x) = 2 sigma(2 x) - 1: 2 x and 2 sigma are exact, the subtraction rounds once:
        abs(tanh) <= 2 sigma(2 x) rel(sigma)(2 x) + u |tanh x|                              (tanh_abs)
  * row scale (sum_G partials * inv_n + eps)^-1/2: the G partials are added in order (positive terms: relative <= G u), one
    multiply, one add, rsq 2 u; the square root halves the argument's error:
        rel(scale) <= 2 u + (G + 2) u / 2                                                   (scale_rel)
    inv_n and eps are taken as the fp32 values the launch receives.

Binary16 copies (out16, state16): the kernel rounds its fp32 result v; the reference knows v only as r +- tol, and rounding is
monotonic, so the stored value must lie in [rn16(r - tol), rn16(r + tol)]: the rounded reference, or its neighbour exactly where
the reference lies within its own tolerance of a rounding boundary.

Exact parts: every element the launch must not write still holds the 0xFF pattern it was filled with (rows >= M, columns in
[N, ldo), slots not named, rows with row_mask == 0, everything when run_flag != run_gen); c_state rows of unnamed slots hold their
input bits.  State rows are written at `slot`, never at `row`.
"""
import math
import numpy as np

EPI_PARTIAL, EPI_LSTM, EPI_BIAS_DSWISH, EPI_HR, EPI_RESID_SSQ, EPI_SLOT_STORE, EPI_XPART = range(7)
AOP_NONE, AOP_TANH_ADD = 0, 1
GM_SLAB, GM_FULLK, GM_TILE, GM_KW, GM_PP = range(5)
ROUTE_KSPLIT, ROUTE_STREAM, ROUTE_PP, ROUTE_PW, ROUTE_TILE, ROUTE_KW = range(6)
ROW_EPIS = (EPI_HR, EPI_RESID_SSQ, EPI_SLOT_STORE)
SSQ_COLS = 32
MAX_PLANES = 8
U = 2.0 ** -24
PAD = 16                      # ldo / lda / ldr exceed the width by this


# ------------------------------------------------------------------ packed weight orders (kernels.h)
def pack_x4(W):
    """Wp[((ntile*KB + kb)*64 + lane)*4 + j] = W[kb*16 + (lane>>4)*4 + j][ntile*16 + (lane&15)],  KB = K / 16."""
    K, N = W.shape
    assert K % 16 == 0 and N % 16 == 0
    v = W.reshape(K // 16, 4, 4, N // 16, 16)          # kb, lane>>4, j, ntile, lane&15
    return np.ascontiguousarray(v.transpose(3, 0, 1, 4, 2)).reshape(-1)


def unpack_x4(Wp, K, N):
    v = np.asarray(Wp).reshape(N // 16, K // 16, 4, 16, 4)      # ntile, kb, lane>>4, lane&15, j
    return np.ascontiguousarray(v.transpose(1, 2, 4, 0, 3)).reshape(K, N)


def pack_x32(W):
    """dst[((ntile*(K/32) + kb)*64 + lane)*8 + j] = W[kb*32 + (lane>>4)*8 + j][ntile*16 + (lane&15)]."""
    K, N = W.shape
    assert K % 32 == 0 and N % 16 == 0
    v = W.reshape(K // 32, 4, 8, N // 16, 16)
    return np.ascontiguousarray(v.transpose(3, 0, 1, 4, 2)).reshape(-1)


# ------------------------------------------------------------------ error model
def lin_factor(K):
    f, cap = 4.0 * math.sqrt(K) * U, (K + 8) * 2.0 * U
    assert f <= cap
    return f


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def sig_rel(x):
    return 2 * U * ((1.0 - sigmoid(x)) * (1.0 + np.abs(x)) + 1.5)


def tanh_abs(x):
    return 2.0 * sigmoid(2 * x) * sig_rel(2 * x) + U * np.abs(np.tanh(x))


def dswish_of(y, tol_y, a=1.0):
    """(value, tolerance) of DoubleSwish y sigma(y - a) behind a bias add, for y = sum + bias known to tol_y before that add's own
    rounding: 2 |dv/dy| tol_y + 4 hw, hw = what the fp32 add, the subtraction, fast_sigmoid and the product add (module docstring)."""
    sg = sigmoid(y - a)
    v = y * sg
    dy = np.abs(sg + y * sg * (1 - sg))
    hw = np.abs(v) * sig_rel(y - a) + dy * U * np.abs(y) + np.abs(y * sg * (1 - sg)) * U * np.abs(y - a) + U * np.abs(v)
    return v, 2 * dy * tol_y + 4 * hw


def scale_rel(G):
    return 2 * U + (G + 2) * U / 2


def row_scale(ssq, inv_n, eps):
    """(sum of the row's partials * inv_n + eps)^-1/2 with the fp32 inv_n / eps of the launch."""
    return 1.0 / np.sqrt(ssq.astype(np.float64).sum(axis=1) * float(np.float32(inv_n)) + float(np.float32(eps)))


# ------------------------------------------------------------------ cases
class Spec(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def spec(name, cls, epi, M, N, K, **kw):
    s = Spec(name=name, cls=cls, epi=epi, M=M, N=N, K=K, n=1, kz=1, K1=0, a_op=AOP_NONE, wt=0, waves=0xF, tile_ok=0, force=0,
             x_scale=False, aidx1=False, slot=None, mask=False, resid=True, p_add=False, joiner=None, run=True,
             out=True, out16=False, state16=False, tile_pin=(-1, 0, 0), kw_pin=(-1, 0), pp_pin=(-1, 0), expect={}, knobs="default")
    for k in kw:
        assert k in s, k
    s.update(kw)
    if s.slot is None:
        s.slot = epi in (EPI_LSTM, EPI_HR)
    s.K0 = K - s.K1
    s.hidden = N // 4 if epi == EPI_LSTM else 0
    s.width = s.hidden if epi == EPI_LSTM else N
    s.rows_alloc = (M + 255) // 256 * 256 + 256
    s.slots = 2 * M + 1                                  # slot 0 is never named
    s.ldo = s.width + PAD
    s.lda0, s.lda1, s.ldr, s.ldp, s.ld_state = s.K0 + PAD, s.K1 + PAD, N + PAD, N + PAD, N + PAD
    s.xg = (s.K0 if epi in (EPI_LSTM, EPI_XPART) else K) // SSQ_COLS
    s.rg = N // SSQ_COLS
    s.n_norm = 48
    s.eps_x, s.eps_r = 0.25, 0.125
    s.vocab = 5
    s.f16_rows = s.wt == 1 and s.tile_ok == 2
    return s


class Problem:
    pass


def injective(rng, M, slots):
    """Random injective map rows -> slots 1 .. slots-1, never the identity."""
    while True:
        m = (rng.permutation(slots - 1)[:M] + 1).astype(np.int32)
        if M == 1 or not np.array_equal(m, np.arange(M)):
            return m


def make_problem(s, rng):
    f32 = np.float32
    p = Problem()
    M, N, K, K0, K1 = s.M, s.N, s.K, s.K0, s.K1
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape).astype(f32)
    p.W = (u(K, N) * (3.0 / math.sqrt(K))).astype(f32)                      # pre-activations of order one
    p.wp = pack_x4(p.W)
    p.aidx0 = p.aidx0b = p.aidx1 = p.ctx = p.a0b = p.a1 = None
    p.same_idx_b = 1
    if s.joiner == "aidx0":                                                 # both addends by slot
        p.a0, p.a0b, p.aidx0 = u(s.slots, s.lda0), u(s.slots, s.lda0), injective(rng, M, s.slots)
    elif s.joiner == "aidx0b":                                              # a0 by row, the second addend by its own index
        p.a0, p.a0b, p.aidx0b, p.same_idx_b = u(M, s.lda0), u(s.slots, s.lda0), injective(rng, M, s.slots), 0
    elif s.joiner == "ctx":                                                 # second addend: table row ctx0 * vocab + ctx1 of the row's slot
        p.a0, p.a0b, p.aidx0 = u(s.slots, s.lda0), u(s.vocab * s.vocab, s.lda0), injective(rng, M, s.slots)
        p.ctx = np.zeros((s.slots, 4), np.int32)
        p.ctx[:, 0] = rng.integers(0, s.vocab, s.slots); p.ctx[:, 1] = rng.integers(0, s.vocab, s.slots); p.ctx[:, 2] = -1
    else:
        p.a0 = u(M, s.lda0)
    if K1 or s.epi == EPI_XPART:
        if s.aidx1:
            p.a1, p.aidx1 = u(s.slots, max(s.lda1, 1)), injective(rng, M, s.slots)
        else:
            p.a1 = u(M, max(s.lda1, 1))
    p.slot_idx = injective(rng, M, s.slots) if s.slot else None
    p.row_mask = None
    if s.mask:
        p.row_mask = (rng.uniform(size=M) < 0.6).astype(np.int32)
        if M > 1:
            p.row_mask[0], p.row_mask[-1] = 1, 0
    p.bias = u(N) if s.epi in (EPI_LSTM, EPI_BIAS_DSWISH, EPI_RESID_SSQ, EPI_SLOT_STORE) else None
    p.resid = u(M, s.ldr) if (s.epi == EPI_HR or (s.epi == EPI_RESID_SSQ and s.resid)) else None
    p.p_add = u(M, s.ldp) if s.p_add else None
    part = lambda G: (rng.uniform(0.5, 1.5, (M, G)) * (s.n_norm / G)).astype(f32)
    p.x_ssq = part(s.xg) if s.x_scale else None
    p.r_ssq = part(s.rg) if s.epi == EPI_HR else None
    p.c_state = u(s.slots, s.hidden) if s.epi == EPI_LSTM else None
    return p


class Case:
    def __init__(self, s, seed=0):
        self.spec = s
        rng = np.random.default_rng([seed, abs(hash_name(s.name))])
        self.probs = [make_problem(s, rng) for _ in range(s.n)]


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % (1 << 31)
    return h


# ------------------------------------------------------------------ the mathematics
def operands(s, p, mut=None):
    """Logical A segments [M][K0], [M][K1] and W[K][N] in float64, as the kernel's products see them."""
    f64 = np.float64
    rows = np.arange(s.M)
    r0 = p.aidx0 if p.aidx0 is not None else rows
    A0 = p.a0[r0, :s.K0].astype(f64)
    if s.a_op == AOP_TANH_ADD:
        j = r0 if p.same_idx_b else (p.aidx0b if p.aidx0b is not None else rows)
        if p.ctx is not None:
            j = p.ctx[j, 0] * s.vocab + p.ctx[j, 1]
        A0 = np.tanh(A0 + p.a0b[j, :s.K0].astype(f64))
    A1 = np.zeros((s.M, 0))
    if s.K1:
        r1 = p.aidx1 if (p.aidx1 is not None and mut != "a1_row") else rows
        A1 = p.a1[r1, :s.K1].astype(f64)
    W = p.W.astype(f64)
    if s.wt == 1 and mut != "fp32_operands":
        h = lambda x: x.astype(np.float32).astype(np.float16).astype(f64)
        A0, A1, W = h(A0), h(A1), h(W)
    if mut == "drop_block":
        A0 = A0.copy(); A0[:, 16:32] = 0.0
    if mut == "swap_k":
        W = W.copy(); W[[5, 38]] = W[[38, 5]]
    return A0, A1, W


def sums(s, p, mut=None):
    """The two half sums and their absolute-value sums: Sx over A segment 0, Sh over segment 1 (zeros where a half sits out)."""
    A0, A1, W = operands(s, p, mut)
    z = np.zeros((s.M, s.N))
    use_x, use_h = bool(s.waves & 0x3), bool(s.waves & 0xC) and s.K1 > 0
    if s.waves == 0xF:
        use_x, use_h = True, s.K1 > 0
    Sx, Tx = (A0 @ W[:s.K0], np.abs(A0) @ np.abs(W[:s.K0])) if use_x else (z, z)
    Sh, Th = (A1 @ W[s.K0:], np.abs(A1) @ np.abs(W[s.K0:])) if use_h else (z, z)
    Kx, Kh = (s.K0 if use_x else 0), (s.K1 if use_h else 0)
    if s.a_op == AOP_TANH_ADD:          # the fp32 tanh of the prologue: each a_k carries tanh_abs
        r0 = p.aidx0 if p.aidx0 is not None else np.arange(s.M)
        j = r0 if p.same_idx_b else (p.aidx0b if p.aidx0b is not None else np.arange(s.M))
        if p.ctx is not None:
            j = p.ctx[j, 0] * s.vocab + p.ctx[j, 1]
        x = p.a0[r0, :s.K0].astype(np.float64) + p.a0b[j, :s.K0].astype(np.float64)
        dA = tanh_abs(x) + U * np.abs(x)
        return Sx, Sh, Tx, Th, Kx + Kh, dA @ np.abs(W[:s.K0])
    return Sx, Sh, Tx, Th, Kx + Kh, z


def evaluate(s, p, mut=None, override=None):
    """Float64 values and tolerances of every buffer the launch writes: name -> (val [M][w], tol [M][w]).
    override = (Sx, Sh): the two half sums from elsewhere (the fp32 emulation), in place of the float64 ones."""
    Sx, Sh, Tx, Th, Ksum, pro = sums(s, p, mut)
    if override is not None:
        Sx, Sh = override
    f = lin_factor(Ksum)
    M, N = s.M, s.N
    xs = row_scale(p.x_ssq, 1.0 / s.n_norm, s.eps_x)[:, None] if p.x_ssq is not None else np.ones((M, 1))
    xrel = scale_rel(s.xg) if p.x_ssq is not None else 0.0
    bias = p.bias.astype(np.float64)[None, :] if p.bias is not None else np.zeros((1, N))
    out = {}
    if s.epi in (EPI_PARTIAL, EPI_XPART):
        acc = Sx * xs + Sh
        if mut == "scale_both":
            acc = (Sx + Sh) * xs
        out["planes" if s.epi == EPI_PARTIAL else "out"] = (acc, f * (Tx * xs + Th) + 4 * (pro + np.abs(Sx * xs) * (xrel + U)))
        return out
    if s.epi == EPI_LSTM:
        xin = p.p_add[:, :N].astype(np.float64) if p.p_add is not None else Sx * xs
        pre = (xin + Sh) + bias
        if mut == "scale_both":
            pre = (Sx + Sh) * xs + bias
        tl = f * (Tx * xs + Th)
        hw_pre = np.abs(xin) * (xrel + U) + U * (np.abs(xin + Sh) + np.abs(pre)) + U * np.abs(xin)
        g = pre.reshape(M, s.hidden, 4); tl = tl.reshape(M, s.hidden, 4); hp = hw_pre.reshape(M, s.hidden, 4)
        gi, gf, gg, go = (g[..., k] for k in ((1, 0, 2, 3) if mut == "swap_fi" else (0, 1, 2, 3)))
        c = p.c_state[p.slot_idx].astype(np.float64)
        si, sf, tg, so = sigmoid(gi), sigmoid(gf), np.tanh(gg), sigmoid(go)
        c_new = sf * c + si * tg
        tc = np.tanh(c_new)
        u_ = so * tc
        dci, dcf, dcg = np.abs(si * (1 - si) * tg), np.abs(sf * (1 - sf) * c), np.abs(si * (1 - tg * tg))
        duo, duc = np.abs(so * (1 - so) * tc), np.abs(so * (1 - tc * tc))
        lin_c = dci * tl[..., 0] + dcf * tl[..., 1] + dcg * tl[..., 2]
        lin_u = duo * tl[..., 3] + duc * lin_c
        hw_c = (dci * hp[..., 0] + dcf * hp[..., 1] + dcg * hp[..., 2] + np.abs(c) * sf * sig_rel(gf) + np.abs(tg) * si * sig_rel(gi)
                + si * tanh_abs(gg) + 3 * U * (np.abs(sf * c) + np.abs(si * tg)))
        hw_u = duo * hp[..., 3] + np.abs(tc) * so * sig_rel(go) + so * tanh_abs(c_new) + duc * hw_c + U * np.abs(u_)
        out["c_state"] = (c_new, 2 * lin_c + 4 * hw_c)
        out["out"] = (u_, 2 * lin_u + 4 * hw_u)
        return out
    acc, tl = Sx + Sh, f * (Tx + Th)
    if s.epi in ROW_EPIS:
        out["planes"] = (acc, tl)                        # the planes + row kernel form: the planes summed are the plain product
    if s.epi == EPI_BIAS_DSWISH:
        out["out"] = dswish_of(acc + bias, tl, 0.0 if mut == "sig_y" else 1.0)
    elif s.epi == EPI_HR:
        rs = row_scale(p.r_ssq, 1.0 / s.n_norm, s.eps_r)[:, None]
        x = p.resid[:, :N].astype(np.float64) * rs
        v = x + acc
        out["state"] = (acc, tl)
        out["out"] = (v, 2 * tl + 4 * (np.abs(x) * (scale_rel(s.rg) + U) + U * np.abs(v)))
    elif s.epi == EPI_RESID_SSQ:
        y = acc + bias
        hw = U * np.abs(y)
        if p.resid is not None:
            y = p.resid[:, :N].astype(np.float64) + y
            hw = hw + U * np.abs(y)
        ty = 2 * tl + 4 * hw
        out["out"] = (y, ty)
        sh = 4 if mut == "ssq_shift" else 0
        yy = np.roll(y, -sh, axis=1) if sh else y
        ss = (yy * yy).reshape(M, N // SSQ_COLS, SSQ_COLS).sum(axis=2)
        out["ssq"] = (ss, (2 * np.abs(y) * ty).reshape(M, N // SSQ_COLS, SSQ_COLS).sum(axis=2) + 4 * 7 * U * (y * y).reshape(M, N // SSQ_COLS, SSQ_COLS).sum(axis=2))
    elif s.epi == EPI_SLOT_STORE:
        v = acc * xs + bias
        out["out"] = (v, 2 * tl * xs + 4 * (np.abs(acc * xs) * (xrel + U) + U * np.abs(v)))
    return out


# ------------------------------------------------------------------ where the values land
def layout(s, p):
    """name -> (shape, dtype, target rows [M] of the value rows, written mask [M], width, base array or None)."""
    M = s.M
    rows = np.arange(M)
    act = np.ones(M, bool) if s.run else np.zeros(M, bool)
    L = {}
    if s.epi == EPI_PARTIAL:
        L["planes"] = ((MAX_PLANES, s.rows_alloc, s.N), np.float32, rows, act, s.N, None)
        return L
    orow, oact, R = rows, act, s.rows_alloc
    if s.epi == EPI_SLOT_STORE:
        if p.slot_idx is not None:
            orow, R = p.slot_idx, s.slots
        if p.row_mask is not None:
            oact = act & (p.row_mask != 0)
    if s.out:
        L["out"] = ((R, s.ldo), np.float32, orow, oact, s.width, None)
    if s.out16:
        L["out16"] = ((R, s.ldo), np.float16, orow, oact, s.width, None)
    if s.epi == EPI_HR:
        L["state"] = ((s.slots, s.ld_state), np.float32, p.slot_idx, act, s.N, None)
        if s.state16:
            L["state16"] = ((s.slots, s.ld_state), np.float16, p.slot_idx, act, s.N, None)
    if s.epi == EPI_LSTM:
        L["c_state"] = ((s.slots, s.hidden), np.float32, p.slot_idx, act, s.hidden, p.c_state)
    if s.epi == EPI_RESID_SSQ:
        L["ssq"] = ((s.rows_alloc, s.N // SSQ_COLS), np.float32, rows, act, s.N // SSQ_COLS, None)
    if s.epi in ROW_EPIS:
        L["planes"] = ((MAX_PLANES, s.rows_alloc, s.N), np.float32, rows, act, s.N, None)
    return L


VALUE_OF = {"out16": "out", "state16": "state"}


def pattern(shape, dtype):
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xFF, np.uint8).view(dtype).reshape(shape)


def render(s, p, ev, mut=None):
    """Buffers as a launch that computed exactly `ev` (in fp32) would leave them; the placement mutants of the CPU tests."""
    bufs = {}
    for name, (shape, dtype, rows, act, w, base) in layout(s, p).items():
        b = pattern(shape, dtype) if base is None else base.copy()
        val = ev[VALUE_OF.get(name, name)][0].astype(np.float32)
        if name == "planes":
            if s.epi == EPI_PARTIAL:
                b[0, rows[act], :w] = val[act]
        else:
            r = np.arange(s.M) if (mut == "state_row" and name in ("state", "c_state")) else rows
            a = np.ones(s.M, bool) if (mut == "bias_masked" and name == "out") else act
            v = val.copy()
            if mut == "bias_masked" and name == "out":
                v[~act] = p.bias[None, :]
            b[r[a], :w] = v[a].astype(dtype)
            if mut == "row_past_M" and name == "out":
                b[s.M, :w] = v[-1].astype(dtype)
        bufs[name] = b
    return bufs


def bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def err_ratio(err, tol):
    """err / tol; 0 where err is 0 (whatever the tolerance); inf wherever the quotient is not a finite number, so that no NaN can hide
    behind a comparison or an argmax."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / tol)
    r[~np.isfinite(r)] = np.inf
    return r


def compare(s, p, ev, bufs, plan_planes=None, rows_limit=None):
    """Per buffer: (worst err / tol, index of it).  A case passes at <= 1.  Elements that must not be written count as 0 when
    they hold their pattern (or input) bits and as inf otherwise.  plan_planes: the partial planes the launch wrote (a fused
    row-epilogue launch: 0, its planes stay untouched)."""
    res = {}
    if plan_planes is None:
        plan_planes = 1 if s.epi == EPI_PARTIAL else 0
    for name, (shape, dtype, rows, act, w, base) in layout(s, p).items():
        b = np.asarray(bufs[name]).reshape(shape)
        val, tol = ev[VALUE_OF.get(name, name)]
        if rows_limit is not None:
            act = act & (np.arange(s.M) < rows_limit)
        written = np.zeros(shape, bool)
        ratio = np.zeros(shape)
        if name == "planes" and plan_planes == 0:
            pass
        elif name == "planes":
            written[:plan_planes, rows[act], :w] = True
            got = b[:plan_planes].astype(np.float64).sum(axis=0)[rows[act], :w]
            r = err_ratio(np.abs(got - val[act]), tol[act])
            ratio[0, rows[act], :w] = r
        else:
            written[rows[act], :w] = True
            got = b[rows[act], :w].astype(np.float64)
            if dtype == np.float16:
                h = lambda x: x.astype(np.float16).astype(np.float64)
                lo, hi = h(val[act] - tol[act]), h(val[act] + tol[act])
                # the figure: how far the reference is from the reals that round to the stored value, in tolerances (0 = the
                # rounded reference itself); the verdict: the interval above
                g16 = b[rows[act], :w]
                inf16 = np.float16(np.inf)
                edge_lo = (got + np.nextafter(g16, -inf16).astype(np.float64)) / 2
                edge_hi = (got + np.nextafter(g16, inf16).astype(np.float64)) / 2
                dist = np.maximum(np.maximum(edge_lo - val[act], val[act] - edge_hi), 0.0)
                r = np.minimum(err_ratio(dist, tol[act]), 1.0)
                bad = ~((got >= lo) & (got <= hi))
                r[bad] = np.maximum(err_ratio(dist[bad], tol[act][bad]), 1.0 + 2.0 ** -20)
            else:
                r = err_ratio(np.abs(got - val[act]), tol[act])
            r[~np.isfinite(got)] = np.inf
            ratio[rows[act], :w] = r
        if rows_limit is None:
            ref_bits = bits(pattern(shape, dtype) if base is None else base.reshape(shape))
            stray = (bits(b) != ref_bits) & ~written
            ratio[stray] = np.inf
        i = np.unravel_index(np.argmax(ratio), shape)
        res[name] = (float(ratio[i]), tuple(int(x) for x in i))
    return res


def worst(res):
    return max(v[0] for v in res.values()) if res else 0.0


# ------------------------------------------------------------------ fp32 emulation of the canonical order (CPU tests)
def chain32(A, W):
    """One in-order fp32 chain per output: acc = fl32(acc + a_k w_k), the product exact (float64), one rounding per step."""
    acc = np.zeros((A.shape[0], W.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = (acc.astype(np.float64) + np.outer(A[:, k], W[k])).astype(np.float32)
    return acc


def slab32(A, W):
    c = [chain32(A[:, i * A.shape[1] // 4:(i + 1) * A.shape[1] // 4], W[i * W.shape[0] // 4:(i + 1) * W.shape[0] // 4]) for i in range(4)]
    return ((c[0] + c[1]) + c[2]) + c[3]


def emulate32(s, p, rows):
    """(Sx, Sh) of the first `rows` rows as an fp32 machine adds them: chunk chains, ((c0+c1)+c2)+c3, pairwise slab tree
    (kernels.h); the two-segment forms (kz = 1) give chunks 0, 1 to segment 0 and 2, 3 to segment 1; the fp16 tile forms run one
    chain over each segment."""
    A0, A1, W = operands(s, p)
    A0, A1 = A0[:rows], A1[:rows]
    z = np.zeros((rows, s.N), np.float32)
    if s.f16_rows and s.kz == 1:
        return (chain32(A0, W[:s.K0]) if s.waves & 3 else z), (chain32(A1, W[s.K0:]) if s.K1 and s.waves & 0xC else z)
    if s.K1 or s.epi == EPI_XPART:
        half = lambda A, Wh: chain32(A[:, :A.shape[1] // 2], Wh[:Wh.shape[0] // 2]) + chain32(A[:, A.shape[1] // 2:], Wh[Wh.shape[0] // 2:])
        return (half(A0, W[:s.K0]) if s.waves & 3 else z), (half(A1, W[s.K0:]) if s.K1 and s.waves & 0xC else z)
    ks = s.K // s.kz
    parts = [slab32(A0[:, i * ks:(i + 1) * ks], W[i * ks:(i + 1) * ks]) for i in range(s.kz)]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
    return parts[0], z
