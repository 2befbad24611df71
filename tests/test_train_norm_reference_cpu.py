"""CPU: the float64 references of tests/train_norm_ref.py against independent formulations -- float64 autograd through the
plain expression, np.add.at, the Random123 known answers -- and their error bounds against the same expressions evaluated
in plain fp32 numpy on the inputs of the GPU cases, which must stay within HALF of every bound (a condition on the bound,
not a measurement)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_norm_ref as tr

f32 = np.float32


def close(got, want, rtol=1e-10, scale=None):
    """scale: the magnitude the error is relative to where `want` itself is a sum that cancels"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max() if scale is None else scale
    assert np.abs(got - want).max() <= rtol * max(scale, 1e-30), np.abs(got - want).max()


def half(got32, ref, bound, what):
    ratio = float((np.abs(np.asarray(got32, dtype=np.float64) - ref) / bound).max())
    print(f"{what}: fp32 numpy / bound = {ratio:.3f}")
    assert ratio <= 0.5, (what, ratio)


def leaves(B, C, L, seed, U=None):
    g = torch.Generator().manual_seed(seed)
    shape = (B, C, L) if U is None else (B, C, L, U)
    mk = lambda *s, scale=1.0, off=0.0: (torch.randn(*s, generator=g, dtype=torch.float64) * scale + off).requires_grad_(True)
    return mk(*shape, scale=1.4, off=0.6), mk(C, scale=0.3, off=1.0), mk(C, scale=0.3), mk(B, C, scale=0.3, off=1.0), mk(B, C, scale=0.3), g


def npy(t):
    return t.detach().numpy()


def fold_and_act(x, gw, gb, f, b, G, eps, act):
    """forward by the reference pieces from the float64 rows x [B, C, L]: (A, Bs, mean, rstd, t, y)"""
    xs = npy(x)
    L = xs.shape[2]
    A, Bs, mean, rstd = tr.fold_fwd64(xs.sum(-1), (xs * xs).sum(-1), npy(gw), npy(gb), npy(f), npy(b), G, L, eps)
    t = A[..., None] * xs + Bs[..., None]
    return A, Bs, mean, rstd, t, tr.act64(t, act)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("G,cpg", [(1, 1), (1, 4), (2, 3), (8, 1), (8, 3), (8, 4), (2, 4)])
def test_fold_activation_and_backward_fold_are_group_norm_autograd(G, cpg, act):
    B, C, L, eps = 3, G * cpg, 37, 1e-5
    x, gw, gb, f, b, g = leaves(B, C, L, 10 * G + cpg + act)
    u = F.group_norm(x, G, gw, gb, eps) * f[:, :, None] + b[:, :, None]
    y = u * torch.sigmoid(u) if act else u
    gy = torch.randn(B, C, L, generator=g, dtype=torch.float64)
    y.backward(gy)
    A, Bs, mean, rstd, t, yr = fold_and_act(x, gw, gb, f, b, G, eps, act)
    close(yr, npy(y))
    xs, gyn = npy(x), gy.numpy()
    da = gyn * tr.act_d64(t, act)
    r = tr.fold_bwd64(da.sum(-1), (da * xs).sum(-1), mean, rstd, npy(gw), npy(gb), npy(f), G, L, A=A, xs1=xs.sum(-1))
    dx = A[..., None] * da + r["Q"][..., None] + r["R"][..., None] * xs
    close(dx, npy(x.grad))
    close(r["pw"][..., 0].sum(0), npy(gw.grad))
    close(r["pw"][..., 1].sum(0), npy(gb.grad))
    close(r["dfac"], npy(f.grad))
    close(r["dbias"], npy(b.grad))
    close(r["pw"][..., 2].sum(0), npy(x.grad).sum((0, 2)), scale=np.abs(npy(x.grad)).sum((0, 2)).max())
    # without A / xs1 the by-product is zero; without fac it is 1
    r0 = tr.fold_bwd64(da.sum(-1), (da * xs).sum(-1), mean, rstd, npy(gw), npy(gb), None, G, L)
    assert np.all(r0["pw"][..., 2] == 0.0)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("G,cpg,U", [(1, 3, 8), (2, 4, 16), (8, 1, 8)])
def test_max_over_neighbours_is_amax_autograd(G, cpg, U, act):
    B, C, M, eps = 2, G * cpg, 9, 1e-5
    x, gw, gb, f, b, g = leaves(B, C, M, 7 * G + U + act, U=U)
    u = F.group_norm(x, G, gw, gb, eps) * f[:, :, None, None] + b[:, :, None, None]
    y = (u * torch.sigmoid(u) if act else u).amax(-1)
    gy = torch.randn(B, C, M, generator=g, dtype=torch.float64)
    y.backward(gy)
    A, Bs, mean, rstd, t, ya = fold_and_act(x.reshape(B, C, M * U), gw, gb, f, b, G, eps, act)
    ya = ya.reshape(B, C, M, U)
    best = tr.first_argmax(ya)
    close(np.take_along_axis(ya, best[..., None], -1)[..., 0], npy(y))
    xs = npy(x)
    xstar = np.take_along_axis(xs, best[..., None], -1)[..., 0]
    da = gy.numpy() * tr.act_d64(A[..., None] * xstar + Bs[..., None], act)
    r = tr.fold_bwd64(da.sum(-1), (da * xstar).sum(-1), mean, rstd, npy(gw), npy(gb), npy(f), G, M * U)
    hot = np.arange(U) == best[..., None]
    dx = np.where(hot, (A[..., None] * da)[..., None], 0.0) + r["Q"][..., None, None] + r["R"][..., None, None] * xs
    close(dx, npy(x.grad))
    close(r["pw"][..., 0].sum(0), npy(gw.grad))
    close(r["dfac"], npy(f.grad))


def test_first_argmax_takes_the_first_of_equal_maxima():
    v = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, 1.0, 2.0, 7.0], [-1.0, -1.0, -3.0, -1.0]])
    assert tr.first_argmax(v).tolist() == [1, 0, 3, 0]


def se_leaves(C, Cr, g):
    mk = lambda *s: (torch.randn(*s, generator=g, dtype=torch.float64) / np.sqrt(s[1])).requires_grad_(True)
    return mk(Cr, C), mk(C, Cr)


@pytest.mark.parametrize("C,Cr", [(8, 1), (12, 3), (64, 5)])
def test_se_gate_pair_is_se3d_autograd(C, Cr):
    """GN false: y = x sigmoid(W2 relu(W1 mean(x)));  dx = g gy + Q"""
    B, L = 3, 21
    g = torch.Generator().manual_seed(C + Cr)
    x = (torch.randn(B, C, L, generator=g, dtype=torch.float64) + 0.4).requires_grad_(True)
    w1, w2 = se_leaves(C, Cr, g)
    y = x * torch.sigmoid(torch.relu(x.mean(-1) @ w1.t()) @ w2.t())[:, :, None]
    gy = torch.randn(B, C, L, generator=g, dtype=torch.float64)
    y.backward(gy)
    xs, gyn = npy(x), gy.numpy()
    mean = xs.sum(-1) / L
    h, gate = tr.se_fwd64(mean, npy(w1), npy(w2))
    close(gate[..., None] * xs, npy(y))
    S = np.stack([gyn.sum(-1), (gyn * xs).sum(-1)], -1)
    r = tr.se_bwd64(S, gate, h, mean, npy(w1), npy(w2), L)
    close(gate[..., None] * gyn + r["Q"][0][..., None], npy(x.grad))
    close(r["dw1"][0], npy(w1.grad))
    close(r["dw2"][0], npy(w2.grad))
    assert "Sp" not in r


@pytest.mark.parametrize("G,cpg,Cr", [(1, 4, 1), (2, 3, 4), (8, 1, 3), (8, 4, 5)])
def test_gate_behind_adagn_is_autograd_through_both(G, cpg, Cr):
    """GN true: y = g u, u = GroupNorm(x) f + b, g from the channel means of u; the backward fold takes the gate in"""
    B, C, L, eps = 3, G * cpg, 19, 1e-5
    x, gw, gb, f, b, g = leaves(B, C, L, G + cpg + Cr)
    w1, w2 = se_leaves(C, Cr, g)
    u = F.group_norm(x, G, gw, gb, eps) * f[:, :, None] + b[:, :, None]
    y = u * torch.sigmoid(torch.relu(u.mean(-1) @ w1.t()) @ w2.t())[:, :, None]
    gy = torch.randn(B, C, L, generator=g, dtype=torch.float64)
    y.backward(gy)
    A, Bs, mean, rstd, t, _ = fold_and_act(x, gw, gb, f, b, G, eps, 0)
    xs, gyn = npy(x), gy.numpy()
    xs1 = xs.sum(-1)
    um = A * (xs1 / L) + Bs
    h, gate = tr.se_fwd64(um, npy(w1), npy(w2))
    close((gate * A)[..., None] * xs + (gate * Bs)[..., None], npy(y))
    S = np.stack([gyn.sum(-1), (gyn * xs).sum(-1)], -1)
    r = tr.se_bwd64(S, gate, h, um, npy(w1), npy(w2), L, A=A, Bs=Bs, xs1=xs1)
    Sp, qse = r["Sp"][0], r["Q"][0]
    du = gate[..., None] * gyn + qse[..., None]
    close(Sp, np.stack([du.sum(-1), (du * xs).sum(-1)], -1), rtol=1e-9)
    k = tr.fold_bwd64(Sp[..., 0], Sp[..., 1], mean, rstd, npy(gw), npy(gb), npy(f), G, L, A=A, xs1=xs1, gate=gate, qse=qse)
    dx = k["Aout"][..., None] * gyn + k["Q"][..., None] + k["R"][..., None] * xs
    close(dx, npy(x.grad), rtol=1e-9)
    close(k["pw"][..., 0].sum(0), npy(gw.grad), rtol=1e-9)
    close(k["pw"][..., 1].sum(0), npy(gb.grad), rtol=1e-9)
    close(k["pw"][..., 2].sum(0), npy(x.grad).sum((0, 2)), rtol=1e-9, scale=np.abs(npy(x.grad)).sum((0, 2)).max())
    close(k["dfac"], npy(f.grad), rtol=1e-9)
    close(k["dbias"], npy(b.grad), rtol=1e-9)
    close(r["dw1"][0], npy(w1.grad), rtol=1e-9)
    close(r["dw2"][0], npy(w2.grad), rtol=1e-9)


# ---- Philox ------------------------------------------------------------------------------------------------------------

def test_host_philox_known_answer():
    """Random123 kat_vectors, the ones tests/test_chain_gpu.py::test_philox_known_answer holds"""
    assert [hex(v) for v in tr.philox4x32_10(np.zeros((1, 4), np.uint32), (0, 0))[0]] == \
        ['0x6627e8d5', '0xe169c58d', '0xbc57ac4c', '0x9b00dbd8']
    ones = np.full((1, 4), 0xFFFFFFFF, np.uint32)
    assert [hex(v) for v in tr.philox4x32_10(ones, (0xFFFFFFFF, 0xFFFFFFFF))[0]] == \
        ['0x408f276d', '0x41c83b0e', '0xa20bc7c6', '0x6d5451fd']
    pi = np.array([[0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]], np.uint32)
    assert [hex(v) for v in tr.philox4x32_10(pi, (0xa4093822, 0x299f31d0))[0]] == \
        ['0xd16cfe09', '0x94fdcceb', '0x5001e420', '0x24126ea1']


@pytest.mark.parametrize("seed", [0, 1, 2 ** 32, 0x7E3779B97F4A7C15])
def test_keep_mask_quad_form_and_single_element_form_agree(seed):
    n = 1027
    for keep in (0.5, 0.9, 1.0):
        quad = tr.keep_mask(n, seed, keep)
        single = tr.drop_word(np.arange(n), seed).astype(np.int64) < tr.drop_threshold(keep)
        assert np.array_equal(quad, single)
        assert abs(quad.mean() - keep) < 0.06
    assert tr.drop_threshold(1.0) == 0xFFFFFFFF and tr.drop_threshold(0.5) == 2 ** 31
    # the key's upper word matters, and so does the stream word
    assert not np.array_equal(tr.keep_mask(n, 1, 0.5), tr.keep_mask(n, 1 + 2 ** 32, 0.5))
    first = tr.philox4x32_10(np.array([[0, 0, tr.DROP_STREAM, 0]]), (seed & 0xFFFFFFFF, seed >> 32))[0]
    assert np.array_equal(tr.drop_word(np.arange(4), seed), first)


# ---- ordered scatter ---------------------------------------------------------------------------------------------------

def scatter_inputs(B, C, S, E, bins, seed):
    rng = np.random.default_rng(seed)
    idx = rng.integers(-2, bins + 2, (B, E)).astype(np.int32)
    idx[:, : E // 2] = min(3, bins - 1)              # one long bin
    return (rng.standard_normal((B, C, S)).astype(f32), idx, rng.uniform(0, 1, (B, E)).astype(f32))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("B,C,S,E,bins", [(2, 3, 50, 50, 7), (1, 2, 33, 99, 9), (1, 1, 4000, 4000, 5)])
def test_scatter_in_order32_against_add_at(B, C, S, E, bins, weighted):
    gy, idx, w = scatter_inputs(B, C, S, E, bins, E + bins)
    got = tr.scatter_in_order32(gy, idx, w if weighted else None, S, bins)
    assert got.dtype == np.float32 and got.shape == (B, C, bins)
    src = np.arange(E) % S
    for b in range(B):
        tb = np.clip(idx[b], 0, bins - 1)
        term = gy[b].astype(np.float64)[:, src] * (w[b].astype(np.float64)[None, :] if weighted else 1.0)
        n = np.bincount(tb, minlength=bins)
        for c in range(C):
            ref, mag = np.zeros(bins), np.zeros(bins)
            np.add.at(ref, tb, term[c])
            np.add.at(mag, tb, np.abs(term[c]))
            assert np.all(np.abs(got[b, c] - ref) <= (n + 1) * tr.U32 * mag + 1e-30)
    # a serial Python loop over one sample and channel, entry by entry
    acc = np.zeros(bins, dtype=f32)
    for e in range(E):
        t = f32(w[0, e] * gy[0, 0, e % S]) if weighted else gy[0, 0, e % S]
        k = min(max(int(idx[0, e]), 0), bins - 1)
        acc[k] = f32(acc[k] + t)
    assert np.array_equal(got[0, 0], acc)


def test_reversing_one_long_bin_changes_bits():
    """the bit-exact GPU test can see an order bug: the same entries of one bin in descending order round differently"""
    S = E = 4000
    gy, idx, w = scatter_inputs(1, 4, S, E, 5, 1)
    fwd = tr.scatter_in_order32(gy, idx, w, S, 5)
    long_bin = np.flatnonzero(np.clip(idx[0], 0, 4) == 3)
    assert long_bin.size >= E // 2
    perm = np.arange(E)
    perm[long_bin] = long_bin[::-1]                  # entry e now carries what entry perm[e] carried
    rev = tr.scatter_in_order32(gy[:, :, perm], idx[:, perm], w[:, perm], S, 5)
    assert np.array_equal(rev[..., [0, 1, 2, 4]], fwd[..., [0, 1, 2, 4]])
    assert not np.array_equal(rev[..., 3], fwd[..., 3])
    assert np.abs(rev[..., 3].astype(np.float64) - fwd[..., 3]).max() <= 1e-3


# ---- the bounds hold plain fp32 numpy with a factor of two to spare ------------------------------------------------------

def swish32(t):
    t = np.asarray(t, dtype=f32)
    with np.errstate(over="ignore"):
        return (t * (f32(1) / (f32(1) + np.exp(-t)))).astype(f32)


def act_d32(t, act):
    t = np.asarray(t, dtype=f32)
    if not act:
        return np.ones_like(t)
    with np.errstate(over="ignore"):
        s = (f32(1) / (f32(1) + np.exp(-t))).astype(f32)
    return (s * (f32(1) + t * (f32(1) - s))).astype(f32)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("rows,L", [(1, 1), (3, 5), (130, 4), (3, 1027), (3, 2050), (1, 1024)])
def test_elementwise_and_row_sum_bounds_hold_fp32_numpy(rows, L, act):
    x, gy, A, Bs, Q, R = tr.elementwise_case(rows, L, 100 * L + rows)
    t, y = tr.apply_fwd64(x, A, Bs, act)
    if L > 5 and rows > 1:
        assert t.min() <= -100.0 + 1e-3 and t.max() >= 30.0 - 1e-3 and np.any(A == 0) and np.any(A < 0) and np.any(A > 0)
    if act:
        half(swish32(t), y, tr.act_bound(t, act), f"swish rows={rows} L={L}")
    half(act_d32(t, act), tr.act_d64(t, act), tr.act_d_bound(t, act), f"act_d rows={rows} L={L} act={act}")
    for mask in (None, np.where(tr.keep_mask(rows * L, 5, 0.9).reshape(rows, L), tr.drop_scale(0.9), f32(0))):
        g = gy if mask is None else (gy * mask).astype(f32)
        d = (g * act_d32(t, act)).astype(f32)
        S, Sb = tr.bwd_stats64(x, gy, A, Bs, act, mask)
        S32 = np.stack([d.sum(1, dtype=f32), (d * x).astype(f32).sum(1, dtype=f32)], 1)
        half(S32, S, Sb, f"bwd_stats rows={rows} L={L} act={act} drop={mask is not None}")
        ref, b = tr.bwd_apply64(x, gy, A, Bs, Q, R, act, mask)
        dx = (((A[:, None] * d).astype(f32) + Q[:, None]).astype(f32) + (R[:, None] * x).astype(f32)).astype(f32)
        half(dx, ref, b, f"bwd_apply rows={rows} L={L} act={act} drop={mask is not None}")


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("U", [8, 64])
def test_max_case_inputs_and_bounds(U, act):
    rows, M = 5, 257
    x, gy, A, Bs, Q, R = tr.max_case(rows, M, U, act, U + act)
    t, y, best = tr.max_fwd64(x, A, Bs, act)
    assert tr.max_case_is_unambiguous(t, y, act)
    ties = (y == y.max(-1, keepdims=True)).sum(-1)
    assert set(range(1, U + 1)) <= set(ties.reshape(-1).tolist())          # every multiplicity of the maximum
    assert np.any((best == U - 1) & (ties == 1))                           # ... and the last slot alone
    assert np.any(A < 0) and np.any(A > 0)
    y32 = swish32(t) if act else t
    assert np.array_equal(tr.first_argmax(y32), best)
    S, Sb, dx, dxb = tr.max_bwd64(x, gy, A, Bs, Q, R, act, best)
    xs = np.take_along_axis(x, best[..., None], -1)[..., 0]
    d = (gy * act_d32(np.take_along_axis(t, best[..., None], -1)[..., 0], act)).astype(f32)
    half(np.stack([d.sum(1, dtype=f32), (d * xs).astype(f32).sum(1, dtype=f32)], 1), S, Sb, f"max bwd_stats U={U} act={act}")
    hot = np.arange(U) == best[..., None]
    base = (Q[:, None, None] + (R[:, None, None] * x).astype(f32)).astype(f32)
    dx32 = np.where(hot, (base + (A[:, None] * d).astype(f32)[..., None]).astype(f32), base)
    half(dx32, dx, dxb, f"max bwd_apply U={U} act={act}")


@pytest.mark.parametrize("C,G", [(8, 8), (24, 8), (40, 8), (64, 1), (1000, 8), (1024, 32)])
def test_fold_bounds_hold_the_double_result_rounded_once(C, G):
    B, L = 5, 64
    k = tr.fold_case(B, C, G, L, C + G)
    fac, bias = k["proj"][:, :C], k["proj"][:, C:]
    ref = tr.fold_fwd64(k["s1"], k["s2"], k["gw"], k["gb"], fac, bias, G, L, 1e-5)
    terms = tr.fold_fwd_terms(k["s1"], k["s2"], k["gw"], k["gb"], fac, bias, G, L, 1e-5)
    for name, r, tm in zip(("A", "Bs", "mean", "rstd"), ref, (0.0, terms, 0.0, 0.0)):
        half(r.astype(f32), r, tr.algebra_bound(r, tm), f"fold {name} C={C} G={G}")
    A32, _, mean32, rstd32 = (v.astype(f32) for v in ref)
    r = tr.fold_bwd64(k["S"][..., 0], k["S"][..., 1], mean32, rstd32, k["gw"], k["gb"], fac, G, L, A=A32, xs1=k["s1"],
                      gate=k["gate"], qse=k["qse"])
    for name in ("Q", "R", "dfac", "dbias", "pw", "Aout"):
        half(r[name].astype(f32), r[name], tr.algebra_bound(r[name], r["terms"][name]), f"bwd_fold {name} C={C} G={G}")


@pytest.mark.parametrize("B", [1, 17, 33])
def test_param_grads_serial_sum_bound(B):
    rng = np.random.default_rng(B)
    pw = rng.standard_normal((B, 257, 3)).astype(f32)
    got = tr.serial_sum32(pw)
    half(got, pw.astype(np.float64).sum(0), (B + 1) * tr.U32 * np.abs(pw).astype(np.float64).sum(0), f"param_grads B={B}")


@pytest.mark.parametrize("N", [1, 65, 1000])
def test_rows_dot2_bound(N):
    rng = np.random.default_rng(N)
    C, rows = 3, 6
    g, v = rng.standard_normal((rows, N)).astype(f32), rng.standard_normal((rows, N)).astype(f32)
    ws = rng.uniform(0.5, 1, (3, N)).astype(f32)
    S, b = tr.rows_dot2_64(g, v, ws, C)
    w = ws[np.arange(rows) // C]
    half(np.stack([(g * w).astype(f32).sum(1, dtype=f32), (g * v).astype(f32).sum(1, dtype=f32)], 1), S, b, f"rows_dot2 N={N}")
    other = tr.rows_dot2_64(g, v, ws, 2)[0]
    assert not np.allclose(other[:, 0], S[:, 0])      # the divisor of the row index shows


@pytest.mark.parametrize("C,Cr,B", [(8, 1, 1), (64, 5, 9), (1000, 3, 7), (1024, 128, 8)])
def test_se_gate_bounds_hold_fp32_numpy(C, Cr, B):
    L = 512
    k = tr.se_case(B, C, Cr, L, C + Cr + B)
    w1, w2 = k["w1"], k["w2"]
    for gn in (False, True):
        if gn:
            A, Bs, cm = k["A"], k["Bs"], k["xstats"][..., 0] / L
            s32 = (A.astype(np.float64) * cm + Bs).astype(f32)
        else:
            s32 = (k["stats"][..., 0] / f32(L)).astype(f32)
            A, Bs, cm = np.ones_like(s32), np.zeros_like(s32), s32
        s = A.astype(np.float64) * cm + Bs
        h, g = tr.se_fwd64(s, w1, w2)
        e_h, e_g = tr.se_fwd_bounds(A, Bs, cm, w1, w2)
        h32 = np.maximum(s32 @ w1.T, f32(0)).astype(f32)
        g32 = (f32(1) / (f32(1) + np.exp(-(h32 @ w2.T).astype(f32)))).astype(f32)
        half(h32, h, e_h, f"se h C={C} Cr={Cr} GN={gn}")
        half(g32, g, e_g, f"se g C={C} Cr={Cr} GN={gn}")
        kw = dict(A=k["A"], Bs=k["Bs"], xs1=k["xstats"][..., 0]) if gn else {}
        r = tr.se_bwd64(k["S"], k["g"], k["h"], k["mean"], w1, w2, L, **kw)
        S1, S2, gg = k["S"][..., 0], k["S"][..., 1], k["g"]
        dg = (k["A"].astype(np.float64) * S2 + k["Bs"].astype(np.float64) * S1).astype(f32) if gn else S2
        d2 = ((dg * gg).astype(f32) * (f32(1) - gg)).astype(f32)
        d1 = np.where(k["h"] > 0, (d2 @ w2).astype(f32), f32(0))
        q = ((d1 @ w1).astype(f32) / f32(L)).astype(f32)
        half(d2, *r["dpre2"], f"se dpre2 C={C} GN={gn}")
        half(d1, *r["dpre1"], f"se dpre1 C={C} GN={gn}")
        half(q, *r["Q"], f"se Q C={C} GN={gn}")
        half((d2.T @ k["h"]).astype(f32), *r["dw2"], f"se dw2 C={C} GN={gn}")
        half((d1.T @ k["mean"]).astype(f32), *r["dw1"], f"se dw1 C={C} GN={gn}")
        if gn:
            sp = np.stack([gg.astype(np.float64) * S1 + float(L) * q, gg.astype(np.float64) * S2 + q * k["xstats"][..., 0]], -1)
            half(sp.astype(f32), *r["Sp"], f"se Sp C={C}")
