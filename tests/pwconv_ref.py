"""Float64 references, error bounds, shape table and data kinds for the fp32 1x1-convolution / linear kernels of
csrc/pwconv.hip (pwconv_kernel, pwconv_small_kernel, linear_rows_kernel, pwconv_pack_kernel), and a numpy emulation of
the kernels' own arithmetic that tests/test_pwconv_reference_cpu.py holds to the same bounds.  torch on any device (the
GPU tests evaluate the float64 side on the device, in batch chunks); imports nothing from lion_amd.

u = 2^-24 is the unit roundoff of fp32 (pointwise_ref.U32).  gamma(n) = n u / (1 - n u) bounds the relative error of n
nested roundings."""
import math

import numpy as np
import torch

import pointwise_ref as pr

U32 = pr.U32
EXACT_MAX = 2 ** 24          # integers up to here are fp32 numbers
SMALL_L = 4096               # PW_SMALL_L: up to here pwconv_small_kernel runs, whatever the plan
LDS_MAX = 150 * 1024         # PW_LDS_MAX
WLDS_GRID = 2048             # launch_pw stages the weights in LDS from this many (column tile, sample) workgroups


def gamma(n):
    return n * U32 / (1.0 - n * U32)


# ---- the plan of the library, recomputed from its formulas (pw_lds / pw_plan / launch_pw of csrc/pwconv.hip) -------------

def pw_lds(cb, cin, pro=True, wlds=True):
    ksteps = (cin + 1) // 2
    return ((2 * ksteps * cb * 32 if wlds else 0) + (2 * cin if pro else 0) + 4 * cb * 32 * 2 + 3 * cb * 32) * 4


def pw_plan(cout, cin):
    """(CB, VB) of the large kernel: the widest channel tile that divides ceil32(Cout) and fits LDS; (0, 0): unsupported"""
    blocks = (cout + 31) // 32
    for cb, vb in ((8, 1), (4, 2), (2, 4), (1, 4)):
        if blocks % cb == 0 and pw_lds(cb, cin) <= LDS_MAX:
            return cb, vb
    return 0, 0


def path(cin, cout, L, B):
    """("small",) | ("large", CB, wlds) | ("none",) and the columns per statistics tile (0: unsupported)"""
    if L <= SMALL_L:
        return ("small",), 32
    cb, vb = pw_plan(cout, cin)
    if not cb:
        return ("none",), 0
    cols = 4 * vb * 32
    return ("large", cb, math.ceil(L / cols) * B >= WLDS_GRID), cols


def stats_depth(cols):
    """nested fp32 additions behind one tile sum.  Small kernel (32 columns): four DPP steps and the row pair.  Large
    kernel (cols = 128 VB): VB serial adds per lane, four DPP steps, the row pair, three LDS adds of the four waves."""
    return 5 if cols == 32 else cols // 128 + 4 + 1 + 3


S, ON, OFF = ("small",), True, False
# (Cin, Cout, L, B): expected path.  Cin = 1, 5: ksteps = 1, 3 -> the last waves of the small kernel get no k-step / the
# fourth none; Cin > 128: the operand group (64 / VB k-steps) of the large kernel loops; L = 4097 = 8 * 512 + 1: one live
# column in the last tile, waves 1..3 of its workgroup (and three of wave 0's four column blocks) wholly beyond L.
TABLE = {
    (1, 1, 1, 2): S, (5, 31, 31, 2): S, (2, 33, 32, 3): S, (3, 96, 33, 2): S, (35, 160, 4095, 2): S,
    (131, 64, 4096, 2): S, (259, 320, 77, 2): S, (6, 256, 300, 3): S, (9, 128, 1000, 2): S, (4, 32, 64, 2): S,
    (1200, 32, 4096, 1): S,
    # large kernel, weights from L2
    (131, 256, 4097, 2): ("large", 8, OFF), (4, 256, 4230, 3): ("large", 8, OFF),
    (259, 128, 4100, 2): ("large", 4, OFF), (7, 128, 4097, 3): ("large", 4, OFF),
    (300, 128, 4500, 2): ("large", 2, OFF), (320, 256, 4200, 2): ("large", 2, OFF), (3, 64, 4097, 3): ("large", 2, OFF),
    (5, 320, 4097, 2): ("large", 2, OFF), (2, 33, 5000, 2): ("large", 2, OFF),
    (1, 1, 4097, 3): ("large", 1, OFF), (35, 160, 4097, 2): ("large", 1, OFF), (3, 31, 4700, 2): ("large", 1, OFF),
    (6, 32, 5000, 3): ("large", 1, OFF),
    # large kernel, weights through LDS: >= 2048 workgroups per channel tile, Cin small
    (4, 256, 4097, 63): ("large", 8, ON), (5, 128, 4097, 121): ("large", 4, ON), (6, 33, 4097, 228): ("large", 2, ON),
    (3, 64, 4100, 228): ("large", 2, ON), (3, 31, 4097, 228): ("large", 1, ON), (4, 65, 4097, 228): ("large", 1, ON),
}
UNSUPPORTED = (1200, 32, 5000, 1)   # no 32-row weight tile of Cin = 1200 fits LDS; at L = 4096 (in TABLE) the small kernel runs it
# lion_pwconv_forward_max (OUT = 1, OUT = 2): L % 32 == 0, L > 4096, >= 2048 workgroups
MAX_TABLE = {
    (4, 256, 4128, 63): 8, (5, 128, 4128, 121): 4, (6, 64, 4128, 228): 2, (3, 32, 4128, 228): 1,
    (6, 33, 4128, 228): 2, (4, 65, 4128, 228): 1,
}
KINDS = ("unit", "rows", "cancel", "bias")


def check_table(lib):
    """every row takes the path the table says: the library's tile count is that of the path's tile width, the LDS rule
    is tiles * B >= 2048, and together the rows reach every kernel variant"""
    seen = set()
    for (cin, cout, L, B), want in TABLE.items():
        got, cols = path(cin, cout, L, B)
        assert got == want, (cin, cout, L, B, got)
        tiles = lib.lion_pwconv_stat_tiles(cout, cin, L)
        assert tiles == math.ceil(L / cols), (cin, cout, L, tiles)
        if got[0] == "large":
            cb, vb = pw_plan(cout, cin)
            assert cols == {1: 128, 2: 256, 4: 512}[vb] and got[2] == (tiles * B >= 2048)
            # the 32-column tiles of the small kernel and the 128 VB of this plan give different counts here
            assert tiles != math.ceil(L / 32) and all(tiles != math.ceil(L / c) for c in (128, 256, 512) if c != cols)
        seen.add(got)
    assert seen == {("small",)} | {("large", cb, on) for cb in (8, 4, 2, 1) for on in (True, False)}, seen
    for (cin, cout, L, B), cb in MAX_TABLE.items():
        assert path(cin, cout, L, B)[0] == ("large", cb, True) and L % 32 == 0 and L > SMALL_L
        assert lib.lion_pwconv_stat_tiles(cout, cin, L) * B >= 2048
    assert {cb for cb in MAX_TABLE.values()} == {8, 4, 2, 1}
    assert {32, 64, 128, 256} <= {k[1] for k in MAX_TABLE} and any(k[1] % 32 for k in MAX_TABLE)
    cin, cout, L, B = UNSUPPORTED
    assert lib.lion_pwconv_stat_tiles(cout, cin, L) == 0 and path(cin, cout, L, B)[0] == ("none",)
    assert (cin, cout, SMALL_L, B) in TABLE


# ---- data ---------------------------------------------------------------------------------------------------------------

def make_data(kind, cin, cout, L, B, seed, device="cpu"):
    """x f32[B, Cin, L], w f32[Cout, Cin], bias f32[Cout], pro = (A, Bs) f32[B, Cin].
    unit: Gaussian, |w| ~ 1/sqrt(Cin).  rows: input channels spread over 10^+-3, output channels over 10^+-2.
    cancel: the channels of the second (fourth) wave's K range of the small kernel repeat those of the first (third) with
    the weights negated, 30 x larger than the rest: the wave partials cancel to a thirtieth of their size.
    bias: |bias| = 64 sigma of the product, so sum y^2 >> the variance.
    int: small integers, every fp32 operation on them exact (see exact_ok)."""
    g = torch.Generator(device=device).manual_seed(seed)

    def randn(*s):
        return torch.randn(*s, generator=g, device=device, dtype=torch.float32)

    if kind == "int":
        def ri(lo, hi, *s):
            return torch.randint(lo, hi + 1, s, generator=g, device=device).float()
        return ri(-2, 2, B, cin, L), ri(-1, 1, cout, cin), ri(-3, 3, cout), None
    x, w, bias = randn(B, cin, L), randn(cout, cin) / math.sqrt(cin), randn(cout) * 0.1
    if kind == "rows":
        x = x * 10.0 ** (torch.rand(cin, generator=g, device=device) * 6 - 3)[None, :, None]
        w = w * 10.0 ** (torch.rand(cout, generator=g, device=device) * 4 - 2)[:, None]
    elif kind == "cancel":
        per = 2 * (((cin + 1) // 2 + 3) // 4)     # channels per wave of the small kernel
        for lo in (0, 2 * per):
            n = max(0, min(per, cin - lo - per))
            if n:
                x[:, lo + per:lo + per + n] = x[:, lo:lo + n]
                w[:, lo:lo + n] *= 30.0
                w[:, lo + per:lo + per + n] = -w[:, lo:lo + n]
        w = w + randn(cout, cin) / (30.0 * math.sqrt(cin))
    elif kind == "bias":
        bias = 64.0 * torch.sign(randn(cout))
    else:
        assert kind == "unit", kind
    pro = (randn(B, cin) * 0.5 + 1.0, randn(B, cin) * 0.3)
    return x.contiguous(), w.contiguous(), bias.contiguous(), pro


# ---- float64 references and bounds ---------------------------------------------------------------------------------------

def swish64(t):
    """pointwise_ref.swish64 on a float64 tensor of any device"""
    e = torch.exp(-t.abs())
    return torch.where(t >= 0, t / (1.0 + e), t * e / (1.0 + e))


def swish_bound(t, ref, arg_err):
    """pointwise_ref.swish_bound for an fp32 argument known only to within arg_err of the float64 t:
    (|t| + arg_err + 8) u (|swish64(t)| + 1.1 arg_err) + 1e-35"""
    return (t.abs() + arg_err + 8.0) * U32 * (ref.abs() + 1.1 * arg_err) + 1e-35


def operand64(x, pro):
    """the GEMM's activation operand in float64 and the bound delta of the kernel's error on it.  No prologue: x itself,
    delta = None (exact).  Prologue: swish64(x a + b); the kernel forms the argument in fp32, x*a+b either as a rounded
    product and a rounded sum or as one fma: at most 2u (|x a| + |b|) off; swish is 1.1-Lipschitz (max |swish'| = 1.0998),
    so that costs 1.1 x as much, and swish_fast on its fp32 argument errs by swish_bound."""
    x = x.double()
    if pro is None:
        return x, None
    a, b = pro[0].double()[:, :, None], pro[1].double()[:, :, None]
    xa = x * a
    t = xa + b
    s = swish64(t)
    arg = 2.0 * U32 * (xa.abs() + b.abs())
    return s, swish_bound(t, s, arg) + 1.1 * arg


C_EXTRA = 4   # the bias add, the second rounding a two-term MFMA step may make, and second-order terms of gamma(Cin)


def pwconv64(x, w, bias=None, pro=None):
    """(ref, bound) f64[B, Cout, L] of y = W act(x) + bias.
    |y - ref| <= (Cin + c) u (|W| @ |xin| + |bias|): the dot-product bound, which holds for ANY order of the Cin products
    and additions (Higham, Accuracy and Stability, 3.1) -- the serial chain of the large kernel as well as the four wave
    partials of the small one -- with c = C_EXTRA roundings on top.  With the prologue the kernel's operand is within
    delta of xin (operand64): the exact product moves by at most |W| @ delta, and the rounding term grows by
    (Cin + c) u |W| @ delta."""
    xin, delta = operand64(x, pro)
    w = w.double()
    cin = w.shape[1]
    ref = torch.einsum("oc,bcl->bol", w, xin)
    mag = torch.einsum("oc,bcl->bol", w.abs(), xin.abs())
    if bias is not None:
        ref = ref + bias.double()[None, :, None]
        mag = mag + bias.double().abs()[None, :, None]
    if delta is not None:
        wd = torch.einsum("oc,bcl->bol", w.abs(), delta)
        return ref, (cin + C_EXTRA) * U32 * (mag + wd) + wd
    return ref, (cin + C_EXTRA) * U32 * mag


def tile_stats64(ref, bound, cols):
    """(sums, bounds) f64[B, Cout, T, 2] per tile of `cols` columns: (sum y, sum y^2) of the float64 y and what the
    kernel's sums of ITS y may differ by.  With e the element bound and |y32| <= |ref| + e, d = stats_depth(cols):
      s1: sum e + gamma(d) sum |y32|                      (propagated error + the d nested additions)
      s2: sum (2 |ref| e + e^2) + gamma(d + 1) sum y32^2  (squaring doubles the relative error of y and rounds once more)
    Columns beyond L count as exact zeros."""
    B, C, L = ref.shape
    T = math.ceil(L / cols)
    pad = T * cols - L
    r = torch.nn.functional.pad(ref, (0, pad)).view(B, C, T, cols)
    e = torch.nn.functional.pad(bound, (0, pad)).view(B, C, T, cols)
    d = stats_depth(cols)
    ya = r.abs() + e
    s = torch.stack([r.sum(-1), (r * r).sum(-1)], -1)
    b = torch.stack([e.sum(-1) + gamma(d) * ya.sum(-1),
                     (2.0 * r.abs() * e + e * e).sum(-1) + gamma(d + 1) * (ya * ya).sum(-1)], -1)
    return s, b


def exact_ok(x, w, bias):
    """integer data on which every fp32 partial sum of the GEMM is exact in any order: sum |w| |x| + |bias| < 2^24"""
    mag = torch.einsum("oc,bcl->bol", w.double().abs(), x.double().abs()).max().item()
    return float(mag) + (0.0 if bias is None else bias.abs().max().item()) < EXACT_MAX


def max64(ref, bound, out_a, out_b):
    """(ref, bound) f64[B, Cout, L / 32] of max over each 32 columns of swish(y A + Bs) (OUT = 2).  Per element the
    argument (y A + Bs in fp32, fused or not) is off by |A| e_y + 2u (|y A| + |Bs|), swish is 1.1-Lipschitz, swish_fast
    adds swish_bound; max is 1-Lipschitz in the sup norm, so the largest element bound of the group bounds the max."""
    a, b = out_a.double()[:, :, None], out_b.double()[:, :, None]
    ya = ref * a
    t = ya + b
    s = swish64(t)
    arg = a.abs() * bound + 2.0 * U32 * ((ref.abs() + bound) * a.abs() + b.abs())
    e = swish_bound(t, s, arg) + 1.1 * arg
    B, C, L = ref.shape
    return s.view(B, C, L // 32, 32).amax(-1), e.view(B, C, L // 32, 32).amax(-1)


def act64(v, act, slope):
    if act == 1:
        return torch.relu(v)
    if act == 2:
        return torch.where(v > 0, v, v * slope)
    return v


def linear64(x, w, bias, act=0, slope=0.0):
    """(ref, bound) f64[B, O] of act(x W^T + bias): the dot-product bound of pwconv64 with K for Cin; relu and leaky relu
    (|slope| <= 1) are 1-Lipschitz, the slope product rounds once more (u |ref|).  Where the float64 sum is within the
    bound of 0 the two sides may take different branches: both branch values are within (1 + |slope|) x the bound of 0."""
    x, w = x.double(), w.double()
    pre = x @ w.t()
    mag = x.abs() @ w.abs().t()
    if bias is not None:
        pre, mag = pre + bias.double(), mag + bias.double().abs()
    e = (w.shape[1] + C_EXTRA) * U32 * mag
    ref = act64(pre, act, slope)
    return ref, e * (1.0 + abs(slope) if act == 2 else 1.0) + U32 * ref.abs()


def packed_layout(w):
    """lion_pwconv_pack_weights: [Cout, Cin] -> k-major [ceil2(Cin), ceil64(Cout)], zero padded"""
    cout, cin = w.shape
    out = torch.zeros(((cin + 1) // 2 * 2, (cout + 63) // 64 * 64), dtype=w.dtype, device=w.device)
    out[:cin, :cout] = w.t()
    return out


# ---- the kernels' arithmetic in fp32 numpy ---------------------------------------------------------------------------

F = np.float32


def _fma32(a, b, c):
    """fp32 fma: the product of two fp32 numbers is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def _swish_fast32(t):
    with np.errstate(over="ignore"):
        e = np.exp(-t).astype(F)
        return (t * (F(1) / (F(1) + e).astype(F)).astype(F)).astype(F)


def _row_tree32(v):
    """[..., 32] -> [...]: row16_sum_rn on both 16-lane rows (xor butterfly 1, 2, 4, 8), then the odd row + the even row"""
    for m in (1, 2, 4, 8):
        v = (v + v[..., np.arange(32) ^ m]).astype(F)
    return (v[..., 16] + v[..., 0]).astype(F)


def emulate_pwconv32(x, w, bias, pro, cols, fused_arg=False):
    """y f32[B, Cout, L] and tile sums f32[B, Cout, T, 2] as the kernels form them.  cols = 32: pwconv_small_kernel (the
    k-steps split over four waves, an fma chain each, ((w0 + w1) + w2) + w3, + bias); cols = 128 VB: pwconv_kernel (one
    fma chain over all of K, + bias; per lane VB serial adds, the row tree, then the four waves ((0 + w0) + w1) + w2) + w3).
    fused_arg: the prologue's x*a+b as one fma."""
    x, w = np.asarray(x, dtype=F), np.asarray(w, dtype=F)
    B, cin, L = x.shape
    cout = w.shape[0]
    if pro is not None:
        a, b = (np.asarray(p, dtype=F)[:, :, None] for p in pro)
        t = _fma32(x, np.broadcast_to(a, x.shape), np.broadcast_to(b, x.shape)) if fused_arg else ((x * a).astype(F) + b).astype(F)
        x = _swish_fast32(t)
    ksteps = (cin + 1) // 2
    per = (ksteps + 3) // 4 if cols == 32 else ksteps
    parts = []
    for lo in range(0, 4 * per if cols == 32 else per, per):
        acc = np.zeros((B, cout, L), F)
        for k in range(2 * min(lo, ksteps), min(2 * min(lo + per, ksteps), cin)):
            acc = _fma32(np.broadcast_to(w[None, :, k, None], acc.shape), np.broadcast_to(x[:, None, k, :], acc.shape), acc)
        parts.append(acc)
    y = parts[0]
    for p in parts[1:]:
        y = (y + p).astype(F)
    if bias is not None:
        y = (y + np.asarray(bias, dtype=F)[None, :, None]).astype(F)
    T = math.ceil(L / cols)
    yp = np.zeros((B, cout, T * cols), F)
    yp[..., :L] = y
    out = []
    for v in (yp, (yp * yp).astype(F)):
        if cols == 32:
            out.append(_row_tree32(v.reshape(B, cout, T, 32)))
            continue
        vb = cols // 128
        lanes = v.reshape(B, cout, T, 4, vb, 32)      # wave, column block, lane
        s = np.zeros(lanes.shape[:4] + (32,), F)
        for j in range(vb):
            s = (s + lanes[..., j, :]).astype(F)
        wv = _row_tree32(s)                            # [B, Cout, T, 4]
        tot = np.zeros(wv.shape[:3], F)
        for j in range(4):
            tot = (tot + wv[..., j]).astype(F)
        out.append(tot)
    return y, np.stack(out, -1)


def emulate_linear32(x, w, bias, act, slope):
    """linear_rows_kernel: the k-steps split over four waves, fma chains, ((w0 + w1) + w2) + w3, + bias, activation"""
    x, w = np.asarray(x, dtype=F), np.asarray(w, dtype=F)
    y, _ = emulate_pwconv32(x.T[None], w, bias, None, 32)
    v = y[0].T
    if act == 1:
        v = np.where(v > 0, v, F(0))
    elif act == 2:
        v = np.where(v > 0, v, (v * F(slope)).astype(F))
    return v.astype(F)
