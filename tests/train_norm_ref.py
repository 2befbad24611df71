"""Float64 references of the training norm kernels (csrc/norm_train.hip) and of the ordered CSR scatter
(csrc/scatter_csr.hip), and the error bounds their fp32 arithmetic is held to.  numpy on the CPU; imports nothing from
lion_amd.  Written from the formulas in the header comments of norm_train.hip and from lion_amd/train_ops.py:

    y  = act(A x + Bs),  A = rstd_g gw_c f_bc,  Bs = (gb_c - mean_g rstd_g gw_c) f_bc + b_bc
    da = gy act'(A x + Bs),  n = (x - mean) rstd,  dn = gw f da
    dx = rstd (dn - mean_g(dn) - n mean_g(dn n)) = A da + Q + R x

tests/test_train_norm_reference_cpu.py ties every function here to float64 autograd through the plain expression, and
every bound to the same expression evaluated in fp32 numpy.  u = U32 = 2^-24 as in tests/pointwise_ref.py."""
import math

import numpy as np

from pointwise_ref import U32, affine_arg32, gate_bound, row_sum_gamma, swish64, swish_bound  # noqa: F401  (re-exported)

TINY = 1e-35   # results below the normal range of fp32, where the hardware may flush to zero (as in swish_bound)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- activation -------------------------------------------------------------------------------------------------------

def sigmoid64(t):
    t = f64(t)
    e = np.exp(-np.abs(t))
    return np.where(t >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def act64(t, act):
    """act 0: identity, 1: swish"""
    return swish64(t) if act else f64(t)


def act_d64(t, act):
    """d act(t) / dt;  swish'(t) = s (1 + t (1 - s)),  s = sigmoid(t)"""
    t = f64(t)
    if not act:
        return np.ones_like(t)
    s = sigmoid64(t)
    return s * (1.0 + t * (1.0 - s))


def act_bound(t, act):
    """|act_f(t) - act64(t)| for the same fp32 t: the identity is exact, swish is swish_bound"""
    return swish_bound(t) if act else np.full(np.shape(t), TINY)


def act_d_bound(t, act):
    """|act_d(t) - act_d64(t)| for the same fp32 t, by the construction of swish_bound.  The kernel forms
    s = v_rcp_f32(1 + __expf(-t)) and then d = 1 - s, p = t d, q = 1 + p, r = s q, one rounding each.
      e = e^-t carries (|t| + 2) u relative (the rounded product in front of v_exp_f32, v_exp_f32 itself); it moves
      s = 1 / (1 + e) by e / (1 + e) = 1 - s of that; the rounding of 1 + e (u), v_rcp_f32 (2u) and one u of slack for the
      rounded constant:                      ds = ((1 - s)(|t| + 2) + 4) u     relative to s
      d = 1 - s:    absolute  e_d = s ds + u (1 - s)
      p = t d:      absolute  e_p = |t| e_d + u |t| (1 - s)
      q = 1 + p:    absolute  e_q = e_p + u |q|
      r = s q:      absolute  s e_q + |s q| ds + u |s q|
    Past t ~ 17 the true 1 - s is far below u while the computed one is off by e_d ~ 4u: |t| e_d is the whole bound there,
    an absolute 4 |t| u on a derivative of 1."""
    t = f64(t)
    if not act:
        return np.full(t.shape, TINY)
    s = sigmoid64(t)
    at = np.abs(t)
    ds = ((1.0 - s) * (at + 2.0) + 4.0) * U32
    q = 1.0 + t * (1.0 - s)
    e_d = s * ds + U32 * (1.0 - s)
    e_p = at * e_d + U32 * at * (1.0 - s)
    e_q = e_p + U32 * np.abs(q)
    return s * e_q + np.abs(s * q) * (ds + U32) + TINY


# ---- the [B, C] algebra of the GroupNorm fold ---------------------------------------------------------------------------

def _gmax(v, G):
    """largest entry over the channels of a group, spread back over them"""
    B, C = v.shape
    return np.repeat(v.reshape(B, G, C // G).max(-1), C // G, axis=1)


def _gsum(v, G):
    """sum over the channels of a group, spread back over them: [B, C] -> [B, C]"""
    B, C = v.shape
    return np.repeat(v.reshape(B, G, C // G).sum(-1), C // G, axis=1)


def fold_fwd64(s1, s2, gw, gb, fac, bias, G, L, eps):
    """row sums s1 = sum x, s2 = sum x^2 [B, C] -> (A, Bs, mean, rstd) [B, C]; fac / bias [B, C] or None (1 and 0).
    mean_g and the biased variance of the group from the sums, clamped at 0 as GroupNorm's cannot be negative."""
    s1, s2, gw, gb = f64(s1), f64(s2), f64(gw), f64(gb)
    B, C = s1.shape
    cnt = float(C // G) * float(L)
    f = np.ones((B, C)) if fac is None else np.broadcast_to(f64(fac), (B, C))
    b = np.zeros((B, C)) if bias is None else np.broadcast_to(f64(bias), (B, C))
    mean = _gsum(s1, G) / cnt
    var = np.maximum(_gsum(s2, G) / cnt - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    A = rstd * gw * f
    Bs = (gb - mean * rstd * gw) * f + b
    return A, Bs, mean, rstd


def fold_fwd_terms(s1, s2, gw, gb, fac, bias, G, L, eps):
    """the largest term of Bs (the only output of the forward fold that is a sum)"""
    A, Bs, mean, rstd = fold_fwd64(s1, s2, gw, gb, fac, bias, G, L, eps)
    B, C = A.shape
    f = np.ones((B, C)) if fac is None else np.broadcast_to(f64(fac), (B, C))
    b = np.zeros((B, C)) if bias is None else np.broadcast_to(f64(bias), (B, C))
    return np.maximum(np.maximum(np.abs(f64(gb)), np.abs(mean * rstd * f64(gw))) * np.abs(f), np.abs(b))


def fold_bwd64(S1, S2, mean, rstd, gw, gb, fac, G, L, A=None, xs1=None, gate=None, qse=None):
    """row sums S1 = sum da, S2 = sum da x [B, C] -> dict of Q, R, dfac, dbias, pw [B, C, 3], Aout, and `terms`: per
    output the largest of the terms it is a sum of.
        T = sum da n = rstd (S2 - mean S1);  M1 = mean_g(dn) = sum_g gw f S1 / cnt;  M2 = mean_g(dn n) = sum_g gw f T / cnt
        dx = A da - rstd M1 - rstd^2 (x - mean) M2   =>   q = -rstd M1 + rstd^2 mean M2,  R = -rstd^2 M2
        d fac = gw T + gb S1,  d bias = S1,  per-sample terms of d gw, d gb: f T, f S1
        pw[..., 2] = sum over the row of dx = A S1 + L q + R sum x          (A and xs1 = sum x given, else 0)
    With an SE gate g behind the AdaGN the upstream gradient was du = g gy + qse: dx = (A g) gy + (A qse + q) + R x, so
    Q = q + A qse and Aout = A g."""
    S1, S2, m, rs, w, o = (f64(v) for v in (S1, S2, mean, rstd, gw, gb))
    B, C = S1.shape
    cnt = float(C // G) * float(L)
    f = np.ones((B, C)) if fac is None else np.broadcast_to(f64(fac), (B, C))
    T = rs * (S2 - m * S1)
    Tabs = rs * np.maximum(np.abs(S2), np.abs(m * S1))
    M1, M2 = _gsum(w * f * S1, G) / cnt, _gsum(w * f * T, G) / cnt
    M1abs, M2abs = _gmax(np.abs(w * f * S1), G) / cnt, _gmax(np.abs(w * f) * Tabs, G) / cnt
    q = -rs * M1 + rs * rs * m * M2
    qabs = np.maximum(rs * M1abs, rs * rs * np.abs(m) * M2abs)
    R = -rs * rs * M2
    out = {"R": R, "dfac": w * T + o * S1, "dbias": S1.copy()}
    terms = {"R": rs * rs * M2abs, "dfac": np.maximum(np.abs(w) * Tabs, np.abs(o * S1)), "dbias": np.abs(S1)}
    pw = np.zeros((B, C, 3))
    pwabs = np.zeros((B, C, 3))
    pw[..., 0], pw[..., 1] = f * T, f * S1
    pwabs[..., 0], pwabs[..., 1] = np.abs(f) * Tabs, np.abs(f * S1)
    if A is not None and xs1 is not None:
        a, xs = f64(A), f64(xs1)
        pw[..., 2] = a * S1 + float(L) * q + R * xs
        pwabs[..., 2] = np.maximum(np.maximum(np.abs(a * S1), float(L) * qabs), terms["R"] * np.abs(xs))
    out["pw"], terms["pw"] = pw, pwabs
    if gate is not None:
        a = f64(A)
        out["Q"], terms["Q"] = q + a * f64(qse), np.maximum(qabs, np.abs(a * f64(qse)))
        out["Aout"], terms["Aout"] = a * f64(gate), np.abs(a * f64(gate))
    else:
        out["Q"], terms["Q"] = q, qabs
    out["terms"] = terms
    return out


def algebra_bound(ref, terms):
    """the [B, C] kernels work in double from the given inputs and round once to fp32: 2u |ref| (one rounding, and one u
    of slack), plus 1e-12 of the largest term of the expression for what the double cancellation inside it can lose
    (2^-53 per operation, up to a few hundred operations in a group sum: 1e-12 is ample)"""
    return 2.0 * U32 * np.abs(ref) + 1e-12 * terms + TINY


# ---- elementwise passes and row sums -----------------------------------------------------------------------------------

def apply_fwd64(x, A, Bs, act):
    """(t, y): the fp32 argument t = fl(fl(x A) + Bs) per row and act64(t)"""
    t = affine_arg32(x, np.asarray(A)[:, None], np.asarray(Bs)[:, None])
    return t, act64(t, act)


def bwd_terms64(x, gy, A, Bs, act, mask=None):
    """(t, d, e_d): d = gy' act'(t) in float64 with gy' = fl(gy * mask) when a dropout mask (0 or fl(1 / keep)) is given, and
    the bound of the fp32 d: |gy'| act_d_bound(t) + u |d| for the product"""
    x32, g32 = np.asarray(x, dtype=np.float32), np.asarray(gy, dtype=np.float32)
    t = affine_arg32(x32, np.asarray(A)[:, None], np.asarray(Bs)[:, None])
    if mask is not None:
        g32 = (g32 * np.asarray(mask, dtype=np.float32)).astype(np.float32)
    g = g32.astype(np.float64)
    d = g * act_d64(t, act)
    return t, d, np.abs(g) * act_d_bound(t, act) + U32 * np.abs(d)


def bwd_stats64(x, gy, A, Bs, act, mask=None):
    """S = {sum da, sum da x} per row [rows, 2] and its bound: row_sum_gamma(L) sum |term| for the summation plus the
    per-term bound summed over the row (the second sum: times |x|, and one more u for the product d x)"""
    _, d, e_d = bwd_terms64(x, gy, A, Bs, act, mask)
    xx = f64(x)
    L = xx.shape[1]
    g = row_sum_gamma(L)
    S = np.stack([d.sum(1), (d * xx).sum(1)], 1)
    bound = np.stack([g * np.abs(d).sum(1) + e_d.sum(1),
                      g * np.abs(d * xx).sum(1) + (e_d * np.abs(xx) + U32 * np.abs(d * xx)).sum(1)], 1)
    return S, bound + TINY


def bwd_apply64(x, gy, A, Bs, Q, R, act, mask=None):
    """dx = A da + Q + R x and its bound per element: |A| e_d for the activation's derivative, and one u per further
    rounded operation -- A * d, R * x, the two additions, and one of slack: 5 -- relative to |A d| + |Q| + |R x|"""
    _, d, e_d = bwd_terms64(x, gy, A, Bs, act, mask)
    xx = f64(x)
    a, q, r = (f64(v)[:, None] for v in (A, Q, R))
    ref = a * d + q + r * xx
    mag = np.abs(a * d) + np.abs(q) + np.abs(r * xx)
    return ref, np.abs(a) * e_d + 5.0 * U32 * mag + TINY


# ---- the max over U neighbours -------------------------------------------------------------------------------------------

def first_argmax(v):
    """index of the FIRST maximal entry along the last axis"""
    v = np.asarray(v)
    U = v.shape[-1]
    is_max = v == v.max(-1, keepdims=True)
    return np.where(is_max, np.arange(U), U).min(-1)


def max_fwd64(x, A, Bs, act):
    """x [rows, M, U] -> (t [rows, M, U], y [rows, M, U] = act64(t), best [rows, M] = first arg-max of y)"""
    t = affine_arg32(x, np.asarray(A)[:, None, None], np.asarray(Bs)[:, None, None])
    y = act64(t, act)
    return t, y, first_argmax(y)


def max_bwd64(x, gy, A, Bs, Q, R, act, best):
    """(S [rows, 2], S bound, dx [rows, M, U], dx bound): da = gy act'(t*) at the arg-max x*, 0 elsewhere"""
    x32 = np.asarray(x, dtype=np.float32)
    rows, M, U = x32.shape
    xs = np.take_along_axis(x32, best[..., None], -1)[..., 0]           # [rows, M]
    _, d, e_d = bwd_terms64(xs, gy, A, Bs, act)
    xsd = xs.astype(np.float64)
    g = row_sum_gamma(M)
    S = np.stack([d.sum(1), (d * xsd).sum(1)], 1)
    Sb = np.stack([g * np.abs(d).sum(1) + e_d.sum(1),
                   g * np.abs(d * xsd).sum(1) + (e_d * np.abs(xsd) + U32 * np.abs(d * xsd)).sum(1)], 1) + TINY
    a, q, r = (f64(v)[:, None, None] for v in (A, Q, R))
    xx = x32.astype(np.float64)
    hot = np.arange(U)[None, None, :] == best[..., None]
    ad = np.where(hot, a * d[..., None], 0.0)
    dx = ad + q + r * xx
    mag = np.abs(ad) + np.abs(q) + np.abs(r * xx)
    dxb = np.where(hot, np.abs(a) * e_d[..., None], 0.0) + 5.0 * U32 * mag + TINY
    return S, Sb, dx, dxb


# ---- serial and lane-strided sums ----------------------------------------------------------------------------------------

def serial_sum32(v):
    """fp32 sum along axis 0 in ascending order, acc = 0 first (pw_batch_sum_kernel)"""
    v = np.asarray(v, dtype=np.float32)
    acc = np.zeros(v.shape[1:], dtype=np.float32)
    for k in range(v.shape[0]):
        acc = (acc + v[k]).astype(np.float32)
    return acc


def rows_dot2_64(g, v, ws, C):
    """S[row] = {sum_p g[row, p] ws[row // C, p], sum_p g[row, p] v[row, p]} and the bound: a lane adds ceil(N / 64) fused
    terms (one rounding each), then 6 shuffle steps"""
    g, v, ws = f64(g), f64(v), f64(ws)
    rows, N = g.shape
    w = ws[np.arange(rows) // C]
    gam = (math.ceil(N / 64) + 6) * U32
    S = np.stack([(g * w).sum(1), (g * v).sum(1)], 1)
    return S, np.stack([gam * np.abs(g * w).sum(1), gam * np.abs(g * v).sum(1)], 1) + TINY


# ---- SE gate -------------------------------------------------------------------------------------------------------------

def se_fwd64(s, w1, w2):
    """channel means s [B, C] -> (h [B, Cr], g [B, C]) = relu(s W1^T), sigmoid(h W2^T); w1 [Cr, C], w2 [C, Cr]"""
    s, w1, w2 = f64(s), f64(w1), f64(w2)
    h = np.maximum(s @ w1.T, 0.0)
    return h, sigmoid64(h @ w2.T)


def se_n1(C):
    return math.ceil(C / 64) + 6      # a lane's serial fused sum, then the 6 butterfly steps


def se_fwd_bounds(A, Bs, chmean, w1, w2):
    """(bound of h, bound of g) for means s = A chmean + Bs (GN false: A = 1, Bs = 0, chmean = the fp32 quotient).
    h: the first dot product as in gate_bound, (n1 + 4) u sum |w1| (|A chmean| + |Bs|).  g: gate_bound."""
    A, Bs, cm, w1a = f64(A), f64(Bs), f64(chmean), np.abs(f64(w1))
    C, Cr = w1a.shape[1], w1a.shape[0]
    e_h = (se_n1(C) + 4) * U32 * ((np.abs(A * cm) + np.abs(Bs)) @ w1a.T) + TINY
    return e_h, gate_bound(A, Bs, cm, w1, w2, n1=se_n1(C), n2=Cr).numpy()


def se_bwd64(S, g, h, mean, w1, w2, L, A=None, Bs=None, xs1=None):
    """the gate's backward and its bounds, propagated like gate_bound.  S [B, C, 2] = {sum gy, sum gy x}.
        dg = S2 (GN false)  |  A S2 + Bs S1 (GN true: sum gy u with u = A x + Bs)
        dpre2 = dg g (1 - g);  dpre1 = (dpre2 W2) [h > 0];  Q = (dpre1 W1) / L
        Sp = {g S1 + L Q, g S2 + Q sum x} (GN true);  dW2 = dpre2^T h,  dW1 = dpre1^T mean
    dpre2: the rounding of dg to fp32 (GN only; relative to |A S2| + |Bs S1|: it may cancel), of 1 - g, and two products:
    3 or 4 u to first order, doubled for the terms of second order and for the slack every bound here carries.
    dpre1: n1 + 1 roundings in the lane-strided fused sum and butterfly, and dpre2's error through |W2|.
    Q: Cr + 1 roundings of the serial fused sum, dpre1's error through |W1|, all over L, and u for the division.
    Sp: evaluated in double from the fp32 Q and rounded once: 2u of the terms plus Q's error times L or |sum x|.
    dW: serial fused sums over the batch, (B + 1) u sum_b |term|, plus the factors' errors."""
    S, g, h, mean, w1, w2 = (f64(v) for v in (S, g, h, mean, w1, w2))
    B, C = g.shape
    Cr = w1.shape[0]
    S1, S2 = S[..., 0], S[..., 1]
    gn = A is not None
    if gn:
        A, Bs, xs1 = f64(A), f64(Bs), f64(xs1)
        dg, dgabs = A * S2 + Bs * S1, np.abs(A * S2) + np.abs(Bs * S1)
    else:
        dg, dgabs = S2, np.abs(S2)
    dpre2 = dg * g * (1.0 - g)
    e2 = 2.0 * (4.0 if gn else 3.0) * U32 * dgabs * g * (1.0 - g) + TINY
    live = h > 0
    dpre1 = np.where(live, dpre2 @ w2, 0.0)
    e1 = np.where(live, (se_n1(C) + 1) * U32 * (np.abs(dpre2) @ np.abs(w2)) + e2 @ np.abs(w2), 0.0) + TINY
    Q = (dpre1 @ w1) / float(L)
    eQ = ((Cr + 1) * U32 * (np.abs(dpre1) @ np.abs(w1)) + e1 @ np.abs(w1)) / float(L) + U32 * np.abs(Q) + TINY
    out = {"dpre2": (dpre2, e2), "dpre1": (dpre1, e1), "Q": (Q, eQ)}
    if gn:
        Sp = np.stack([g * S1 + float(L) * Q, g * S2 + Q * xs1], -1)
        eSp = np.stack([2 * U32 * (np.abs(g * S1) + float(L) * np.abs(Q)) + float(L) * eQ,
                        2 * U32 * (np.abs(g * S2) + np.abs(Q * xs1)) + eQ * np.abs(xs1)], -1) + TINY
        out["Sp"] = (Sp, eSp)
    dw2 = dpre2.T @ h
    e_dw2 = (B + 1) * U32 * (np.abs(dpre2).T @ np.abs(h)) + e2.T @ np.abs(h) + TINY
    dw1 = dpre1.T @ mean
    e_dw1 = (B + 1) * U32 * (np.abs(dpre1).T @ np.abs(mean)) + e1.T @ np.abs(mean) + TINY
    out["dw2"], out["dw1"] = (dw2, e_dw2), (dw1, e_dw1)
    return out


# ---- dropout: Philox4x32-10 ----------------------------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr uint32-valued [n, 4], key (k0, k1) -> uint32 [n, 4]  (Salmon et al. 2011, ten rounds)"""
    c = np.asarray(ctr).astype(np.uint64)
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[:, 0]
        p1 = np.uint64(0xCD9E8D57) * c[:, 2]
        c = np.stack([((p1 >> s32) ^ c[:, 1] ^ k0) & _M32, p1 & _M32, ((p0 >> s32) ^ c[:, 3] ^ k1) & _M32, p0 & _M32], 1)
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c.astype(np.uint32)


DROP_STREAM = 0x44524F50   # "DROP": the third counter word of the dropout stream


def drop_threshold(keep):
    """thr = keep * 2^32 saturated at 2^32 - 1, from the fp32 keep the entry points receive"""
    t = float(np.float32(keep)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def drop_word(e, seed):
    """the 32-bit word that decides element e (any integer array): word e & 3 of
    philox(counter = (e >> 2 as lo, hi, DROP_STREAM, 0), key = seed lo, hi) -- one Philox call per element"""
    e = np.asarray(e, dtype=np.uint64).reshape(-1)
    quad = e >> np.uint64(2)
    ctr = np.stack([quad & _M32, quad >> np.uint64(32), np.full(e.shape, DROP_STREAM, np.uint64), np.zeros(e.shape, np.uint64)], 1)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return r[np.arange(e.size), (e & np.uint64(3)).astype(np.int64)]


def keep_mask(numel, seed, keep):
    """bool [numel]: element e is kept -- one Philox call per quad of elements"""
    quads = (numel + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    ctr = np.stack([q & _M32, q >> np.uint64(32), np.full(quads, DROP_STREAM, np.uint64), np.zeros(quads, np.uint64)], 1)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return r.reshape(-1)[:numel].astype(np.int64) < drop_threshold(keep)


def drop_scale(keep):
    """fl(1 / keep)"""
    return np.float32(1.0) / np.float32(keep)


# ---- ordered scatter -----------------------------------------------------------------------------------------------------

def scatter_in_order32(gy, idx, w, S, bins):
    """gy f32 [B, C, S], idx int [B, E], w f32 [B, E] or None -> f32 [B, C, bins]: the entries of each bin added in ASCENDING
    entry order in fp32, acc = 0 first, acc = fl(acc + fl(w[e] gy[c, e mod S])) (fl(acc + gy[...]) without w); idx clamped
    to [0, bins).  Vectorised over bins by entry rank: step r adds the r-th entry of every bin that has one."""
    gy = np.asarray(gy, dtype=np.float32)
    idx = np.asarray(idx)
    B, C = gy.shape[:2]
    E = idx.shape[1]
    src = np.arange(E) % S
    out = np.zeros((B, C, bins), dtype=np.float32)
    for b in range(B):
        bin_of = np.clip(idx[b].astype(np.int64), 0, bins - 1)
        order = np.argsort(bin_of, kind="stable")               # by bin, ascending entry inside a bin
        sb = bin_of[order]
        start = np.concatenate([[0], np.cumsum(np.bincount(bin_of, minlength=bins))])
        rank = np.arange(E) - start[sb]
        by_rank = np.argsort(rank, kind="stable")
        cut = np.concatenate([[0], np.cumsum(np.bincount(rank))])
        term = gy[b][:, src]
        if w is not None:
            term = (term * np.asarray(w, dtype=np.float32)[b][None, :]).astype(np.float32)
        acc = out[b]
        for r in range(len(cut) - 1):
            sel = by_rank[cut[r]:cut[r + 1]]
            e, tb = order[sel], sb[sel]
            acc[:, tb] = (acc[:, tb] + term[:, e]).astype(np.float32)
    return out


# ---- the inputs of the GPU cases (seeded, host-made), shared with the CPU test that holds the bounds to fp32 numpy ----------

PLANTED_T = (-100.0, -88.0, -20.0, 30.0, 0.0)   # arguments planted in every row that has room: expf overflows below -88.7


def elementwise_case(rows, L, seed):
    """x, gy [rows, L], A, Bs, Q, R [rows] in fp32: A of both signs with one exact 0 (from three rows on), and A x + Bs
    spanning [-100, 30] through planted elements"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((rows, L)) * 3).astype(np.float32)
    A = (rng.uniform(0.5, 1.5, rows) * np.where((np.arange(rows) + seed) % 2, -1.0, 1.0)).astype(np.float32)
    if rows >= 3:
        A[rows - 1] = 0.0
    Bs = rng.standard_normal(rows).astype(np.float32)
    for k, tv in enumerate(PLANTED_T[:max(L - 1, 1)]):
        ok = A != 0
        x[ok, (7 * k + 1) % L] = ((tv - Bs[ok]) / A[ok]).astype(np.float32)
    gy = rng.standard_normal((rows, L)).astype(np.float32)
    Q = (rng.standard_normal(rows) * 0.3).astype(np.float32)
    R = (rng.standard_normal(rows) * 0.3).astype(np.float32)
    return x, gy, A, Bs, Q, R


def fold_case(B, C, G, L, seed, strided=False):
    """row sums of real data (float64) and the GroupNorm / AdaGN parameters: dict of s1, s2 [B, C] (float64), gw, gb [C],
    proj [B, 2C] (fac = proj[:, :C], bias = proj[:, C:]), and backward row sums S [B, C, 2], qse, gate, all fp32"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((B, C, L)) * 1.3 + 0.4).astype(np.float32).astype(np.float64)
    return {"s1": x.sum(-1), "s2": (x * x).sum(-1),
            "gw": (rng.uniform(0.5, 1.5, C)).astype(np.float32), "gb": (rng.uniform(-0.5, 0.5, C)).astype(np.float32),
            "proj": (rng.standard_normal((B, 2 * C)) * 0.3 + np.concatenate([np.ones(C), np.zeros(C)])).astype(np.float32),
            "S": (rng.standard_normal((B, C, 2)) * np.sqrt(L)).astype(np.float32),
            "qse": (rng.standard_normal((B, C)) * 0.1).astype(np.float32),
            "gate": rng.uniform(0.1, 0.9, (B, C)).astype(np.float32)}


def se_case(B, C, Cr, L, seed):
    """SE gate inputs in fp32 (xstats float64): stats / xstats [B, C, 2] row sums, A, Bs, w1 [Cr, C], w2 [C, Cr], and for the
    backward S [B, C, 2], g in (0, 1), h >= 0 with exact zeros in every second column, mean"""
    rng = np.random.default_rng(seed)
    xs = np.stack([rng.standard_normal((B, C)) * L * 0.5, rng.uniform(1, 2, (B, C)) * L], -1)
    h = np.maximum(rng.standard_normal((B, Cr)), 0.0).astype(np.float32)
    h[:, 1::2] = 0.0
    return {"xstats": xs, "stats": xs.astype(np.float32),
            "A": rng.standard_normal((B, C)).astype(np.float32), "Bs": (rng.standard_normal((B, C)) * 0.5).astype(np.float32),
            "w1": (rng.standard_normal((Cr, C)) / np.sqrt(C)).astype(np.float32),
            "w2": (rng.standard_normal((C, Cr)) / np.sqrt(Cr)).astype(np.float32),
            "S": (rng.standard_normal((B, C, 2)) * np.sqrt(L)).astype(np.float32),
            "g": rng.uniform(0.05, 0.95, (B, C)).astype(np.float32), "h": h,
            "mean": rng.standard_normal((B, C)).astype(np.float32)}


def max_case(rows, M, U, act, seed):
    """x [rows, M, U], gy [rows, M], A (both signs), Bs, Q, R.  Centre m is padded the way ball query pads: its first
    1 + m % U slots are distinct hits, the rest copies of the FIRST hit.  In centres m % 3 == 0 the first hit is the
    group's maximum, so the maximum occurs U - m % U times (1 .. U) and the first of them must win; in centres m % 3 == 1
    it stands in the last distinct slot only (the last slot of the group when m % U == U - 1); in the others anywhere.
    The arguments t = A x + Bs sit on a grid of spacing 0.1 in [0.5, 8] (right of the minimum of swish, where it
    increases): two different activations differ by far more than twice swish_bound, so the arg-max of the reference is
    unambiguous.  A negative A turns the arg-max of x into its arg-min."""
    rng = np.random.default_rng(seed)
    A = (rng.uniform(0.5, 1.5, rows) * np.where((np.arange(rows) + seed) % 2, -1.0, 1.0)).astype(np.float32)
    Bs = rng.standard_normal(rows).astype(np.float32)
    t = np.empty((rows, M, U))
    for m in range(M):
        n = 1 + m % U                                             # distinct hits
        lv = rng.permuted(np.tile(np.arange(70)[None, :], (rows, 1)), axis=1)[:, :n] * 0.1 + 0.5   # distinct levels <= 7.4
        if m % 3 == 0:
            lv[:, 0] = 8.0                                        # the first hit is the maximum: every copy ties with it
        elif m % 3 == 1:
            lv[:, n - 1] = 8.0                                    # the maximum in the last distinct slot only
        t[:, m, :n] = lv
        t[:, m, n:] = lv[:, :1]
    x = ((t - Bs[:, None, None]) / A[:, None, None]).astype(np.float32)
    # the copies must be copies of x bit for bit
    for m in range(M):
        x[:, m, 1 + m % U:] = x[:, m, :1]
    gy = rng.standard_normal((rows, M)).astype(np.float32)
    Q = (rng.standard_normal(rows) * 0.3).astype(np.float32)
    R = (rng.standard_normal(rows) * 0.3).astype(np.float32)
    return x, gy, A, Bs, Q, R


def max_case_is_unambiguous(t, y, act):
    """the condition on the inputs of the max tests: in every group, any two DIFFERENT activations among the largest differ by
    more than twice the activation's bound (ties are exact copies, bit for bit)"""
    b = act_bound(t, act)
    top = y.max(-1, keepdims=True)
    below = np.where(y < top, y, -np.inf)
    second = below.max(-1)
    sep = top[..., 0] - second                                    # inf where the whole group ties
    return bool(np.all(sep > 2.0 * b.max(-1)))
