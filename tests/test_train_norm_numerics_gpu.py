"""-m gpu: the training norm kernels (csrc/norm_train.hip), each entry point on its own through the C ABI with inputs made
on the host, against the float64 references and derived bounds of tests/train_norm_ref.py, at the lengths, channel counts
and batch sizes where their code takes another path.  Every case is a few MB at the most.  The rejection cases are
return codes taken on the host before any launch (read off the entry points)."""
import numpy as np
import pytest
import torch

import train_norm_ref as tr
from test_pointwise_numerics_gpu import dev, host, within

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = tr.f64
EINVAL, EUNSUPPORTED = -1, -2
CG = [(8, 8), (24, 8), (40, 8), (64, 1), (1000, 8), (1024, 32)]
SEEDS = [0, 1, 2 ** 32, 0x7E3779B97F4A7C15]      # the last with its upper word set, as torch.int64.random_() seeds have


def call(name, *args):
    from lion_amd import _lib
    _lib.call(name, *args)


def rc(name, *args):
    """the entry point's return code, unchecked; tensors stand for their pointers, integers pass as raw pointers"""
    from lion_amd import _lib
    argv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    return getattr(_lib.load(), name)(*argv, torch.cuda.current_stream().cuda_stream)


def out(*shape, dtype=torch.float32):
    """an output buffer full of NaN: whatever the kernel leaves unwritten shows"""
    return torch.full(shape, float("nan"), device="cuda", dtype=dtype)


# ---- a. lion_row_stats64 -----------------------------------------------------------------------------------------------

def row_stats64(x):
    rows, L = x.shape
    st = out(rows, 2, dtype=torch.float64)
    call("lion_row_stats64", dev(x), rows, L, st)
    return host(st)


def pivot_of(x):
    """the kernel's pivot: the mean of the row's first min(L, 256) elements, in fp32"""
    return x[:, :min(x.shape[1], 256)].astype(np.float64).mean(1).astype(f32).astype(np.float64)


@pytest.mark.parametrize("L", [1, 3, 4, 5, 255, 256, 1023, 1024, 1028, 4097])
def test_row_stats64_against_float64_sums(L):
    """the bound is on the shifted sums, t1 = sum (x - x0) and t2 = sum (x - x0)^2 in fp32, carried through the double
    hand-over s1 = t1 + n x0, s2 = t2 + 2 x0 t1 + n x0^2 (whose own roundings, 2^-53 each, get 2^-50 of the terms)"""
    for rows in (1, 3, 130):
        rng = np.random.default_rng(1000 * rows + L)
        x = (rng.standard_normal((rows, L)) * 1.5 + 3.0).astype(f32)
        got = row_stats64(x)
        d = x.astype(np.float64)
        x0 = pivot_of(x)
        sh = d - x0[:, None]
        g = tr.row_sum_gamma(L)
        e1, e2 = g * np.abs(sh).sum(1), g * (sh * sh).sum(1)
        dbl1 = 2.0 ** -50 * (np.abs(sh).sum(1) + L * np.abs(x0)) + tr.TINY
        dbl2 = 2.0 ** -50 * ((sh * sh).sum(1) + 2 * np.abs(x0) * np.abs(sh).sum(1) + L * x0 * x0) + tr.TINY
        within(got[:, 0], d.sum(1), e1 + dbl1, f"row_stats64 s1 rows={rows} L={L}")
        within(got[:, 1], (d * d).sum(1), e2 + 2 * np.abs(x0) * e1 + dbl2, f"row_stats64 s2 rows={rows} L={L}")


@pytest.mark.parametrize("L", [1001, 4096, 32768])
def test_row_stats64_variance_does_not_depend_on_where_an_outlier_sits(L):
    """N(0, 1) rows whose first element lies within one standard deviation of the row mean, one element set to 1000, placed
    at index 0, 1, L / 2 and L - 1 in turn: the variance recovered from the two sums, s2 / L - (s1 / L)^2 in double, stays
    within 4 row_sum_gamma(L) of the float64 variance wherever it sits -- 2 for a pivot within one standard deviation of the
    mean, (1 + d^2 / var), times 2 for slack.
    Measured on an MI355X, worst of 4 rows, error / bound with the outlier at index 0:
        L        pivot = the row's first element    pivot = mean of the first min(L, 256) elements
        1001                  8.29                                   0.019
        4096                 25.5                                    0.010
        32768                46.6                                    0.005
    (1.6e-3 of the variance at L = 32768); the other three placements are at 0.002 .. 0.027 of the bound."""
    rows = 4
    rng = np.random.default_rng(L)
    base = rng.standard_normal((rows, L)).astype(f32)
    for pos in (0, 1, L // 2, L - 1):
        x = base.copy()
        x[:, pos] = 1000.0
        d = x.astype(np.float64)
        var = d.var(1)
        if pos:
            assert np.all(np.abs(d[:, 0] - d.mean(1)) <= np.sqrt(var))
        got = row_stats64(x)
        v = got[:, 1] / L - (got[:, 0] / L) ** 2
        within(v, var, 4 * tr.row_sum_gamma(L) * var, f"row_stats64 variance L={L} outlier at {pos}")


# ---- b. lion_gn_train_fold, lion_gn_train_fold64 -----------------------------------------------------------------------

def fac_bias(mode, k, B, C):
    """(fac tensor, stride, bias tensor, stride, fac numpy, bias numpy)"""
    proj = k["proj"]
    if mode == "absent":
        return None, 0, None, 0, None, None
    if mode == "dense":
        return dev(proj[:, :C]), C, dev(proj[:, C:]), C, proj[:, :C], proj[:, C:]
    if mode == "halves":
        p = dev(proj)
        return p[:, :C], 2 * C, p[:, C:], 2 * C, proj[:, :C], proj[:, C:]
    p = dev(proj[:1])                                              # one row for every sample: stride 0
    return p[:, :C], 0, p[:, C:], 0, proj[:1, :C], proj[:1, C:]


def run_fold(name, stats, k, mode, B, C, G, L, eps=1e-5):
    fac, fs, bias, bs, fn, bn = fac_bias(mode, k, B, C)
    o = [out(B, C) for _ in range(4)]
    call(name, stats, dev(k["gw"]), dev(k["gb"]), fac, fs, bias, bs, B, C, G, L, eps, *o)
    return [host(v) for v in o], fn, bn


@pytest.mark.parametrize("mode", ["absent", "dense", "halves", "row"])
@pytest.mark.parametrize("C,G", CG)
def test_gn_train_fold_both_forms_against_float64(C, G, mode):
    L = 64
    for B in (1, 5):
        k = tr.fold_case(B, C, G, L, 10 * C + G + B)
        st64 = np.stack([k["s1"], k["s2"]], -1)
        for name, st in (("lion_gn_train_fold64", st64), ("lion_gn_train_fold", st64.astype(f32))):
            got, fn, bn = run_fold(name, dev(st), k, mode, B, C, G, L)
            s = st.astype(np.float64)
            ref = tr.fold_fwd64(s[..., 0], s[..., 1], k["gw"], k["gb"], fn, bn, G, L, 1e-5)
            terms = tr.fold_fwd_terms(s[..., 0], s[..., 1], k["gw"], k["gb"], fn, bn, G, L, 1e-5)
            for what, g, r, tm in zip(("A", "Bs", "mean", "rstd"), got, ref, (0.0, terms, 0.0, 0.0)):
                within(g, r, tr.algebra_bound(r, tm), f"{name} {what} B={B} C={C} G={G} {mode}")


def test_gn_train_fold_of_a_constant_group_has_rstd_one_over_sqrt_eps():
    B, C, G, L, eps = 2, 24, 8, 64, 1e-5
    k = tr.fold_case(B, C, G, L, 3)
    k["s1"][:, 3:6] = 1.5 * L                                       # group 1 (channels 3..5) is the constant 1.5
    k["s2"][:, 3:6] = 2.25 * L
    want = 1.0 / np.sqrt(float(f32(eps)))
    for name, cast in (("lion_gn_train_fold64", np.float64), ("lion_gn_train_fold", f32)):
        (A, Bs, mean, rstd), fn, bn = run_fold(name, dev(np.stack([k["s1"], k["s2"]], -1).astype(cast)), k, "dense", B, C, G, L, eps)
        assert np.array_equal(rstd[:, 3:6], np.full((B, 3), f32(want)))
        assert np.array_equal(mean[:, 3:6], np.full((B, 3), f32(1.5)))
        ref = want * f64(k["gw"][3:6]) * f64(fn[:, 3:6])
        within(A[:, 3:6], ref, tr.algebra_bound(ref, 0.0), name + " A of a constant group")


def test_gn_train_fold_rejects_more_than_1024_channels():
    B, C, G, L = 1, 1025, 1, 4
    k = tr.fold_case(B, C, G, L, 0)
    o = [out(B, C) for _ in range(4)]
    for name, dt in (("lion_gn_train_fold64", np.float64), ("lion_gn_train_fold", f32)):
        st = dev(np.stack([k["s1"], k["s2"]], -1).astype(dt))
        assert rc(name, st, dev(k["gw"]), dev(k["gb"]), None, 0, None, 0, B, C, G, L, 1e-5, *o) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in o)


# ---- c. lion_affine_act, _bwd_stats, _bwd_apply and their dropout forms ---------------------------------------------------

LENGTHS = [1, 3, 4, 5, 1023, 1024, 1027, 1028, 2050]


def run_elementwise(x, gy, A, Bs, Q, R, act, seed=None, keep=None):
    rows, L = x.shape
    dx_, dg, dA, dB, dQ, dR = (dev(v) for v in (x, gy, A, Bs, Q, R))
    y, S, dxo = out(rows, L), out(rows, 2), out(rows, L)
    if seed is None:
        call("lion_affine_act", dx_, dA, dB, rows, L, act, y)
        call("lion_affine_act_bwd_stats", dx_, dg, dA, dB, rows, L, act, S)
        call("lion_affine_act_bwd_apply", dx_, dg, dA, dB, dQ, dR, rows, L, act, dxo)
    else:
        sd = torch.tensor([seed], dtype=torch.int64).cuda()
        call("lion_affine_act_dropout", dx_, dA, dB, rows, L, act, sd, keep, y)
        call("lion_affine_act_dropout_bwd_stats", dx_, dg, dA, dB, rows, L, act, sd, keep, S)
        call("lion_affine_act_dropout_bwd_apply", dx_, dg, dA, dB, dQ, dR, rows, L, act, sd, keep, dxo)
    return host(y), host(S), host(dxo)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("L", LENGTHS)
def test_affine_act_and_its_backward_passes_against_float64(L, act):
    """float4 path (L % 4 == 0) and scalar tails, odd lengths over more than one workgroup per row (1027, 2050); A of both
    signs and an exact 0; arguments down to -100, where __expf overflows and swish and its derivative must come out 0"""
    for rows in (1, 3, 130):
        case = tr.elementwise_case(rows, L, 100 * L + rows)
        x, gy, A, Bs, Q, R = case
        y, S, dx = run_elementwise(*case, act)
        t, yr = tr.apply_fwd64(x, A, Bs, act)
        tag = f"rows={rows} L={L} act={act}"
        if act:
            within(y, yr, tr.act_bound(t, act), "affine_act " + tag)
        else:
            assert np.array_equal(y, t), "affine_act " + tag      # the identity returns the fp32 argument itself
        Sr, Sb = tr.bwd_stats64(x, gy, A, Bs, act)
        within(S, Sr, Sb, "affine_act_bwd_stats " + tag)
        dr, db = tr.bwd_apply64(x, gy, A, Bs, Q, R, act)
        within(dx, dr, db, "affine_act_bwd_apply " + tag)


@pytest.mark.parametrize("keep", [0.5, 0.9, 1.0])
@pytest.mark.parametrize("L", LENGTHS)
def test_affine_act_dropout_mask_is_the_philox_stream(L, keep):
    """the zeroed elements ARE the complement of the host Philox keep mask (elements whose dropout-free value is 0 aside),
    kept ones the dropout-free value times fl(1 / keep) to one rounding, and both backward passes use the same mask"""
    scale = tr.drop_scale(keep)
    for rows in (1, 3, 130):
        for act in (0, 1):
            case = tr.elementwise_case(rows, L, 100 * L + rows)
            x, gy, A, Bs, Q, R = case
            y0 = run_elementwise(*case, act)[0]
            for seed in SEEDS:
                tag = f"rows={rows} L={L} act={act} keep={keep} seed={seed:#x}"
                y, S, dx = run_elementwise(*case, act, seed, keep)
                kept = tr.keep_mask(rows * L, seed, keep).reshape(rows, L)
                nz = y0 != 0
                assert np.array_equal((y == 0)[nz], ~kept[nz]), "mask " + tag
                assert np.array_equal(y[kept], (y0 * scale).astype(f32)[kept]), "kept values " + tag
                assert np.all(y[~kept] == 0), "dropped values " + tag
                mask = np.where(kept, scale, f32(0))
                Sr, Sb = tr.bwd_stats64(x, gy, A, Bs, act, mask)
                within(S, Sr, Sb, "affine_act_dropout_bwd_stats " + tag)
                dr, db = tr.bwd_apply64(x, gy, A, Bs, Q, R, act, mask)
                within(dx, dr, db, "affine_act_dropout_bwd_apply " + tag)


@pytest.mark.parametrize("keep", [0.0, 1.5])
def test_affine_act_dropout_rejects_a_keep_outside_0_1(keep):
    rows, L = 2, 8
    x, gy, A, Bs, Q, R = (dev(v) for v in tr.elementwise_case(rows, L, 1))
    sd = torch.tensor([1], dtype=torch.int64).cuda()
    y, S = out(rows, L), out(rows, 2)
    assert rc("lion_affine_act_dropout", x, A, Bs, rows, L, 1, sd, keep, y) == EINVAL
    assert rc("lion_affine_act_dropout_bwd_stats", x, gy, A, Bs, rows, L, 1, sd, keep, S) == EINVAL
    assert rc("lion_affine_act_dropout_bwd_apply", x, gy, A, Bs, Q, R, rows, L, 1, sd, keep, y) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(S).all()


# ---- d. lion_affine_act_max and its backward ----------------------------------------------------------------------------

@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("U", [8, 16, 32, 64])
def test_affine_act_max_and_its_backward_take_the_first_maximum(U, act):
    """all four instantiations; groups padded with copies of their first hit, the maximum 1 .. U times in a group and in its
    last slot alone; dx carries A da at the FIRST maximal position and nowhere else, Q + R x everywhere"""
    for M in (1, 255, 256, 257):
        for rows in (1, 5):
            x, gy, A, Bs, Q, R = tr.max_case(rows, M, U, act, 100 * U + M + rows)
            t, yf, best = tr.max_fwd64(x, A, Bs, act)
            assert tr.max_case_is_unambiguous(t, yf, act)
            tag = f"U={U} M={M} rows={rows} act={act}"
            dx_, dg, dA, dB, dQ, dR = (dev(v) for v in (x, gy, A, Bs, Q, R))
            y, S, dxo = out(rows, M), out(rows, 2), out(rows, M, U)
            call("lion_affine_act_max", dx_, dA, dB, rows, M, U, act, y)
            call("lion_affine_act_max_bwd_stats", dx_, dg, dA, dB, rows, M, U, act, S)
            call("lion_affine_act_max_bwd_apply", dx_, dg, dA, dB, dQ, dR, rows, M, U, act, dxo)
            pick = lambda v: np.take_along_axis(v, best[..., None], -1)[..., 0]
            if act:
                within(host(y), pick(yf), pick(tr.act_bound(t, act)), "affine_act_max " + tag)
            else:
                assert np.array_equal(host(y), pick(t)), "affine_act_max " + tag
            Sr, Sb, dr, db = tr.max_bwd64(x, gy, A, Bs, Q, R, act, best)
            within(host(S), Sr, Sb, "affine_act_max_bwd_stats " + tag)
            got = host(dxo)
            within(got, dr, db, "affine_act_max_bwd_apply " + tag)
            hot = np.arange(U) == best[..., None]
            base = (Q[:, None, None] + (R[:, None, None] * x).astype(f32)).astype(f32)
            assert np.array_equal(got[~hot], base[~hot]), "Q + R x off the arg-max " + tag


def test_affine_act_max_rejections_are_taken_on_the_host():
    """U outside {8, 16, 32, 64}; more than 65535 rows (blockIdx.y) for the forward and the apply; an x that is not 16-byte
    aligned -- every one a return code before any launch"""
    rows, M, U = 2, 4, 8
    x, gy, A, Bs, Q, R = (dev(v) for v in tr.max_case(rows, M, U, 1, 0))
    x12 = torch.zeros(rows, M, 12, device="cuda")
    y, S, dxo, d12 = out(rows, M), out(rows, 2), out(rows, M, U), out(rows, M, 12)
    assert rc("lion_affine_act_max", x12, A, Bs, rows, M, 12, 1, y) == EUNSUPPORTED
    assert rc("lion_affine_act_max_bwd_stats", x12, gy, A, Bs, rows, M, 12, 1, S) == EUNSUPPORTED
    assert rc("lion_affine_act_max_bwd_apply", x12, gy, A, Bs, Q, R, rows, M, 12, 1, d12) == EUNSUPPORTED
    assert rc("lion_affine_act_max", x, A, Bs, 65536, M, U, 1, y) == EUNSUPPORTED
    assert rc("lion_affine_act_max_bwd_apply", x, gy, A, Bs, Q, R, 65536, M, U, 1, dxo) == EUNSUPPORTED
    assert x.data_ptr() % 16 == 0
    off = x.data_ptr() + 4
    assert rc("lion_affine_act_max", off, A, Bs, rows, M - 1, U, 1, y) == EUNSUPPORTED
    assert rc("lion_affine_act_max_bwd_stats", off, gy, A, Bs, rows, M - 1, U, 1, S) == EUNSUPPORTED
    assert rc("lion_affine_act_max_bwd_apply", off, gy, A, Bs, Q, R, rows, M - 1, U, 1, dxo) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in (y, S, dxo, d12))


# ---- e. lion_gn_train_bwd_fold -------------------------------------------------------------------------------------------

def run_bwd_fold(k, B, C, G, L, dmode, with_a, with_gate):
    """-> (dict of outputs, the untouched part of the [B, 2C] gradient buffer or None, reference)"""
    s = np.stack([k["s1"], k["s2"]], -1)
    fac = k["proj"][:, :C]
    A64, _, mean64, rstd64 = tr.fold_fwd64(k["s1"], k["s2"], k["gw"], k["gb"], fac, k["proj"][:, C:], G, L, 1e-5)
    A, mean, rstd = A64.astype(f32), mean64.astype(f32), rstd64.astype(f32)
    Q, R, pw, Aout = out(B, C), out(B, C), out(B, C, 3), out(B, C)
    p = dev(k["proj"])
    rest = None
    if dmode == "absent":
        dfac = dbias = None
        ds = 0
    elif dmode == "dense":
        dfac, dbias, ds = out(B, C), out(B, C), C
    elif dmode == "halves":
        d = out(B, 2 * C)
        dfac, dbias, ds = d[:, :C], d[:, C:], 2 * C
    else:                                                           # only d fac, in the first half of a [B, 2C] buffer
        d = out(B, 2 * C)
        dfac, dbias, ds, rest = d[:, :C], None, 2 * C, d[:, C:]
    call("lion_gn_train_bwd_fold", dev(k["S"]), dev(mean), dev(rstd), dev(k["gw"]), dev(k["gb"]), p[:, :C], 2 * C, B, C, G, L,
         Q, R, dfac, dbias, ds, pw, dev(A) if with_a else None, dev(s) if with_a else None,
         dev(k["gate"]) if with_gate else None, dev(k["qse"]) if with_gate else None, Aout if with_gate else None)
    ref = tr.fold_bwd64(k["S"][..., 0], k["S"][..., 1], mean, rstd, k["gw"], k["gb"], fac, G, L,
                        A=A if with_a else None, xs1=k["s1"] if with_a else None,
                        gate=k["gate"] if with_gate else None, qse=k["qse"] if with_gate else None)
    got = {"Q": Q, "R": R, "pw": pw, "dfac": dfac, "dbias": dbias, "Aout": Aout if with_gate else None}
    return {n: host(v) for n, v in got.items() if v is not None}, rest, ref


@pytest.mark.parametrize("dmode", ["absent", "dense", "halves", "first half"])
@pytest.mark.parametrize("C,G", CG)
def test_gn_train_bwd_fold_against_float64(C, G, dmode):
    L = 64
    for B in (1, 5):
        k = tr.fold_case(B, C, G, L, 10 * C + G + B)
        for with_a, with_gate in ((False, False), (True, False), (True, True)):
            got, rest, ref = run_bwd_fold(k, B, C, G, L, dmode, with_a, with_gate)
            tag = f"B={B} C={C} G={G} d={dmode} A={with_a} gate={with_gate}"
            for n, v in got.items():
                within(v, ref[n], tr.algebra_bound(ref[n], ref["terms"][n]), f"gn_train_bwd_fold {n} {tag}")
            if not with_a:
                assert np.all(got["pw"][..., 2] == 0)
            if rest is not None:
                assert torch.isnan(rest).all(), "the other half of the gradient buffer was written " + tag


def test_gn_train_bwd_fold_rejections():
    B, C, G, L = 2, 8, 8, 4
    k = tr.fold_case(B, C, G, L, 0)
    ones = np.ones((B, C), f32)
    S, gw, gb, gate = (dev(k[n]) for n in ("S", "gw", "gb", "gate"))
    m, r, fac, A = (dev(ones) for _ in range(4))
    Q, R, d, pw, Aout = out(B, C), out(B, C), out(B, 2 * C), out(B, C, 3), out(B, C)
    xs = dev(np.ones((B, C, 2)))
    args = lambda dstride, qse: (S, m, r, gw, gb, fac, C, B, C, G, L, Q, R, d[:, :C], d[:, C:], dstride, pw, A, xs, gate, qse, Aout)
    assert rc("lion_gn_train_bwd_fold", *args(C - 1, gate)) == EINVAL           # d_stride < C
    assert rc("lion_gn_train_bwd_fold", *args(2 * C, None)) == EINVAL           # a gate without qse
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in (Q, R, d, pw, Aout))


# ---- f. lion_gn_train_param_grads ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_gn_train_param_grads_is_the_serial_ascending_sum(B):
    for C in (1, 255, 256, 257):
        rng = np.random.default_rng(1000 * B + C)
        pw = rng.standard_normal((B, C, 3)).astype(f32)
        want = tr.serial_sum32(pw)
        for with_dxs in (False, True):
            dgw, dgb, dxs = out(C), out(C), out(C)
            call("lion_gn_train_param_grads", dev(pw), B, C, dgw, dgb, dxs if with_dxs else None)
            assert np.array_equal(host(dgw), want[:, 0]) and np.array_equal(host(dgb), want[:, 1]), (B, C)
            if with_dxs:
                assert np.array_equal(host(dxs), want[:, 2]), (B, C)
            else:
                assert torch.isnan(dxs).all()
        ref = pw.astype(np.float64).sum(0)
        within(want, ref, (B + 1) * tr.U32 * np.abs(pw).astype(np.float64).sum(0) + tr.TINY, f"param_grads serial sum B={B} C={C}")


# ---- g. lion_rows_dot2 -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_rows_dot2_against_float64(N):
    """row counts that are no multiple of the 4 waves of a workgroup; ws is indexed by row / C"""
    for B, C in ((1, 1), (1, 3), (3, 1), (2, 2), (5, 1), (2, 3), (5, 3), (10, 13)):
        rows = B * C
        rng = np.random.default_rng(100 * rows + N + C)
        g, v = rng.standard_normal((rows, N)).astype(f32), rng.standard_normal((rows, N)).astype(f32)
        ws = rng.uniform(0.2, 1.0, (B, N)).astype(f32)
        S = out(rows, 2)
        call("lion_rows_dot2", dev(g), dev(v), dev(ws), B, C, N, S)
        ref, b = tr.rows_dot2_64(g, v, ws, C)
        within(host(S), ref, b, f"rows_dot2 B={B} C={C} N={N}")


# ---- h. the SE gate kernels -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gn", [False, True])
@pytest.mark.parametrize("C", [8, 64, 1000, 1024])
def test_se_gate_forward_and_backward_against_float64(C, gn):
    L = 512
    for Cr in (1, 3, 4, 5, 128):
        for B in (1, 7, 8, 9):                                       # around the weight-gradient kernel's unroll of 8
            k = tr.se_case(B, C, Cr, L, 1000 * C + 10 * Cr + B)
            tag = f"C={C} Cr={Cr} B={B} GN={gn}"
            w1, w2 = dev(k["w1"]), dev(k["w2"])
            mean, h, g, zero, A2, B2 = out(B, C), out(B, Cr), out(B, C), out(B, C), out(B, C), out(B, C)
            if gn:
                call("lion_gn_se_gate_fwd", dev(k["xstats"]), dev(k["A"]), dev(k["Bs"]), w1, w2, B, C, Cr, L, mean, h, g, A2, B2)
                A, Bs, cm = k["A"], k["Bs"], k["xstats"][..., 0] / L
                sa = np.abs(f64(A) * cm) + np.abs(f64(Bs))
                mean_b = 2 * tr.U32 * sa
            else:
                call("lion_se_gate_fwd", dev(k["stats"]), w1, w2, B, C, Cr, L, mean, h, g, zero)
                cm = f64(k["stats"][..., 0]) / L
                A, Bs = np.ones((B, C), f32), np.zeros((B, C), f32)
                mean_b = 2 * tr.U32 * np.abs(cm)
                assert np.all(host(zero) == 0), "zero " + tag
            s = f64(A) * cm + f64(Bs)
            hr, gr = tr.se_fwd64(s, k["w1"], k["w2"])
            e_h, e_g = tr.se_fwd_bounds(A, Bs, cm, k["w1"], k["w2"])
            within(host(mean), s, mean_b + tr.TINY, "se_gate_fwd mean " + tag)
            within(host(h), hr, e_h, "se_gate_fwd h " + tag)
            within(host(g), gr, e_g, "se_gate_fwd g " + tag)
            if gn:
                gg = host(g)
                for got, src, what in ((host(A2), k["A"], "A2"), (host(B2), k["Bs"], "B2")):
                    assert np.array_equal(got, (gg * src).astype(f32)), f"{what} is one rounding of g times its factor " + tag
                    within(got, gr * src, e_g * np.abs(src) + tr.U32 * np.abs(gr * src) + tr.TINY, f"gn_se_gate_fwd {what} " + tag)
            # backward, from host-made g / h (exact zeros in h) / mean
            dpre2, dpre1, Q, dw1, dw2, Sp = out(B, C), out(B, Cr), out(B, C), out(Cr, C), out(C, Cr), out(B, C, 2)
            gd, hd, md, Sd = dev(k["g"]), dev(k["h"]), dev(k["mean"]), dev(k["S"])
            if gn:
                call("lion_gn_se_gate_bwd", Sd, dev(k["xstats"]), dev(k["A"]), dev(k["Bs"]), gd, hd, md, w1, w2, B, C, Cr, L,
                     Sp, dpre2, dpre1, Q, dw1, dw2)
                r = tr.se_bwd64(k["S"], k["g"], k["h"], k["mean"], k["w1"], k["w2"], L, A=k["A"], Bs=k["Bs"], xs1=k["xstats"][..., 0])
                within(host(Sp), *r["Sp"], "gn_se_gate_bwd Sp " + tag)
            else:
                call("lion_se_gate_bwd", Sd, gd, hd, md, w1, w2, B, C, Cr, L, dpre2, dpre1, Q, dw1, dw2)
                r = tr.se_bwd64(k["S"], k["g"], k["h"], k["mean"], k["w1"], k["w2"], L)
            for n, v in (("dpre2", dpre2), ("dpre1", dpre1), ("Q", Q), ("dw1", dw1), ("dw2", dw2)):
                within(host(v), *r[n], f"se_gate_bwd {n} " + tag)
            assert np.all(host(dpre1)[k["h"] == 0] == 0)


@pytest.mark.parametrize("C,Cr", [(1025, 4), (64, 129)])
def test_se_gate_kernels_reject_what_their_lds_arrays_cannot_hold(C, Cr):
    B, L = 1, 8
    k = tr.se_case(B, C, Cr, L, 0)
    d = {n: dev(v) for n, v in k.items()}
    o = [out(B, C), out(B, Cr), out(B, C), out(B, C), out(B, C), out(Cr, C), out(C, Cr), out(B, C, 2)]
    mean, h, g, a2, b2, dw1, dw2, Sp = o
    assert rc("lion_se_gate_fwd", d["stats"], d["w1"], d["w2"], B, C, Cr, L, mean, h, g, a2) == EUNSUPPORTED
    assert rc("lion_gn_se_gate_fwd", d["xstats"], d["A"], d["Bs"], d["w1"], d["w2"], B, C, Cr, L, mean, h, g, a2, b2) == EUNSUPPORTED
    assert rc("lion_se_gate_bwd", d["S"], d["g"], d["h"], d["mean"], d["w1"], d["w2"], B, C, Cr, L, mean, h, g, dw1, dw2) == EUNSUPPORTED
    assert rc("lion_gn_se_gate_bwd", d["S"], d["xstats"], d["A"], d["Bs"], d["g"], d["h"], d["mean"], d["w1"], d["w2"], B, C, Cr, L,
              Sp, mean, h, g, dw1, dw2) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(torch.isnan(v).all() for v in o)
