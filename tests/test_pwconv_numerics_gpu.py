"""-m gpu: the fp32 1x1-convolution and linear kernels of csrc/pwconv.hip (pwconv_kernel with its four channel tiles, the
weights through LDS or from L2, the three output modes; pwconv_small_kernel; linear_rows_kernel; pwconv_pack_kernel),
called as the project calls them, at the shapes of tests/pwconv_ref.py's table: exactly on small integers -- which pins the
layout of y and of every tile of the GroupNorm sums -- and against float64 under the derived bounds of that module on four
kinds of data.  The float64 side runs on the device in batch chunks; no case holds more than about 1 GB."""
import math
from types import SimpleNamespace

import pytest
import torch

import pwconv_ref as pw

pytestmark = pytest.mark.gpu

NAN = float("nan")


def lib():
    from lion_amd import _lib
    return _lib.load()


def conv_of(w, bias):
    conv = torch.nn.Conv1d(w.shape[1], w.shape[0], 1, bias=bias is not None).cuda()
    with torch.no_grad():
        conv.weight.copy_(w[:, :, None])
        if bias is not None:
            conv.bias.copy_(bias)
    return conv


def run(x, conv, pro=None, want_stats=True):
    from lion_amd import fused_ops
    with torch.no_grad():
        return fused_ops.pwconv_fused(x, conv, pro, want_stats=want_stats, split=False)


def forward_max(x, conv, pro, out=None):
    """lion_pwconv_forward_max: pass 1 (out None) -> the tile sums, pass 2 (out = (A, Bs)) -> [B, Cout, L / 32]; None
    where the library reports the shape unsupported"""
    from lion_amd import _lib, fused_ops
    B, cin, L = x.shape
    cout = conv.out_channels
    wp = fused_ops.pw_packed_weight(conv.weight)
    bias = None if conv.bias is None else conv.bias.detach()
    pa, pb = (None, None) if pro is None else pro
    if out is None:
        res = torch.full((B, cout, max(lib().lion_pwconv_stat_tiles(cout, cin, L), 1), 2), NAN, device="cuda")
        ok = _lib.call("lion_pwconv_forward_max", x, wp, bias, B, cin, cout, L, pa, pb, None, None, res, None, unsupported_ok=True)
    else:
        res = torch.full((B, cout, L // 32), NAN, device="cuda")
        ok = _lib.call("lion_pwconv_forward_max", x, wp, bias, B, cin, cout, L, pa, pb, out[0], out[1], None, res,
                       unsupported_ok=True)
    return res if ok else None


def chunks(B, cout, L):
    """batch slices of at most 4 M output elements: the float64 side of a 268 MB output never exists as a whole"""
    n = max(1, (1 << 22) // (cout * L))
    return [slice(lo, min(B, lo + n)) for lo in range(0, B, n)]


def worst(got, ref, bound):
    assert bool(torch.isfinite(got).all())
    return float(((got.double() - ref).abs() / bound).max())


def within(ratios, what):
    """the worst error / bound ratio per quantity, printed before it is held to 1"""
    print(what + ": worst error / bound " + ", ".join(f"{k} = {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)


def sub(pro, sl):
    return None if pro is None else (pro[0][sl], pro[1][sl])


# ---- 1. the table ---------------------------------------------------------------------------------------------------

def test_shape_table_reaches_every_path_of_the_kernels():
    """the small kernel, CB = 8 / 4 / 2 / 1 with the weights through LDS and from L2, and both passes of the activated
    maximum at all four channel tiles -- from lion_pwconv_stat_tiles and the tiles * B >= 2048 rule"""
    from lion_amd import fused_ops
    pw.check_table(lib())
    cin, cout, L, B = pw.UNSUPPORTED
    assert not fused_ops.pw_supported(conv_of(torch.zeros(cout, cin), None), torch.zeros(B, cin, L, device="cuda"))
    assert fused_ops.pw_supported(conv_of(torch.zeros(cout, cin), None), torch.zeros(B, cin, pw.SMALL_L, device="cuda"))


# ---- 2. exact on small integers ---------------------------------------------------------------------------------------

def check_exact(x, w, bias, y, st, cols):
    for sl in chunks(x.shape[0], w.shape[0], x.shape[2]):
        ref, _ = pw.pwconv64(x[sl], w, bias)
        assert torch.equal(y[sl].double(), ref)
        if st is not None:
            s, _ = pw.tile_stats64(ref, torch.zeros_like(ref), cols)
            assert s.abs().max().item() < pw.EXACT_MAX        # the data keeps its promise: every tile sum is an fp32 integer
            assert torch.equal(st[sl].double(), s)


@pytest.mark.parametrize("cin,cout,L,B", list(pw.TABLE) + list(pw.MAX_TABLE))
def test_integers_are_exact_in_every_tile(cin, cout, L, B):
    """integer weights, inputs and bias with sum |w| |x| + |bias| < 2^24 and every tile's sum y^2 < 2^24: fp32 arithmetic
    is exact in any order, so y and EACH tile of the sums equal integer arithmetic -- the tile index and channel row of
    every sum, zeros from masked columns, nothing from padded channel rows, and (where the two-pass form runs) the sums
    of OUT = 1 equal to those of OUT = 0."""
    x, w, bias, _ = pw.make_data("int", cin, cout, L, B, cin * 1000 + cout + L, device="cuda")
    assert pw.exact_ok(x[:1], w, bias)
    cols = pw.path(cin, cout, L, B)[1]
    for b in (bias, None):
        conv = conv_of(w, b)
        y, st = run(x, conv)
        assert tuple(st.shape) == (B, cout, math.ceil(L / cols), 2)
        check_exact(x, w, b, y, st, cols)
        y2, st2 = run(x, conv, want_stats=False)
        assert st2 is None and torch.equal(y, y2)
        del y2
        if (cin, cout, L, B) in pw.MAX_TABLE:
            st1 = forward_max(x, conv, None)
            assert st1 is not None and torch.equal(st1, st)


# ---- 3. float64 under derived bounds ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", pw.KINDS)
@pytest.mark.parametrize("cin,cout,L,B", list(pw.TABLE))
def test_against_float64(cin, cout, L, B, kind):
    """y per element and s1 / s2 per tile within pwconv64's / tile_stats64's bounds, with and without the prologue (and,
    on the unit data, without the bias); y does not depend on whether the sums are asked for"""
    x, w, bias, pro = pw.make_data(kind, cin, cout, L, B, cin * 1000 + cout + L, device="cuda")
    cols = pw.path(cin, cout, L, B)[1]
    for p in (None, pro):
        for b in ((bias, None) if kind == "unit" else (bias,)):
            conv = conv_of(w, b)
            y, st = run(x, conv, p)
            y2, _ = run(x, conv, p, want_stats=False)
            assert torch.equal(y, y2)
            del y2
            r = {"y": 0.0, "s1": 0.0, "s2": 0.0}
            for sl in chunks(B, cout, L):
                ref, bound = pw.pwconv64(x[sl], w, b, sub(p, sl))
                sref, sbound = pw.tile_stats64(ref, bound, cols)
                r["y"] = max(r["y"], worst(y[sl], ref, bound))
                r["s1"] = max(r["s1"], worst(st[sl][..., 0], sref[..., 0], sbound[..., 0]))
                r["s2"] = max(r["s2"], worst(st[sl][..., 1], sref[..., 1], sbound[..., 1]))
            within(r, f"pwconv {kind} {(cin, cout, L, B)} pro={p is not None} bias={b is not None}")


# ---- 4. the activated maximum -----------------------------------------------------------------------------------------

def out_affine(B, cout, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B, cout, generator=g, device="cuda") * 0.5 + 1.0, torch.randn(B, cout, generator=g, device="cuda") * 0.3)


@pytest.mark.parametrize("use_pro", [False, True])
@pytest.mark.parametrize("cin,cout,L,B", list(pw.MAX_TABLE))
def test_activated_max_against_float64_and_the_stored_path(cin, cout, L, B, use_pro):
    """lion_pwconv_forward_max: pass 1's sums == those of the storing kernel bit for bit and within the float64 bounds;
    pass 2 == lion_affine_swish_max on the stored y bit for bit (CB = 8, 4, 2, 1) and within max64's bound"""
    from lion_amd import fused_ops
    x, w, bias, pro = pw.make_data("unit", cin, cout, L, B, cin + cout + L, device="cuda")
    p = pro if use_pro else None
    conv = conv_of(w, bias)
    oa, ob = out_affine(B, cout, cout + L)
    y, st = run(x, conv, p)
    st1 = forward_max(x, conv, p)
    got = forward_max(x, conv, p, (oa, ob))
    assert st1 is not None and got is not None
    assert torch.equal(st1, st)
    with torch.no_grad():
        stored = fused_ops.affine_swish(y.view(B, cout, L // 32, 32), oa, ob, reduce_max=True)
    assert torch.equal(got, stored)
    del y, stored
    cols = pw.path(cin, cout, L, B)[1]
    r = {"max": 0.0, "s1": 0.0, "s2": 0.0}
    for sl in chunks(B, cout, L):
        ref, bound = pw.pwconv64(x[sl], w, bias, sub(p, sl))
        m, e = pw.max64(ref, bound, oa[sl], ob[sl])
        sref, sbound = pw.tile_stats64(ref, bound, cols)
        r["max"] = max(r["max"], worst(got[sl], m, e))
        r["s1"] = max(r["s1"], worst(st1[sl][..., 0], sref[..., 0], sbound[..., 0]))
        r["s2"] = max(r["s2"], worst(st1[sl][..., 1], sref[..., 1], sbound[..., 1]))
    within(r, f"forward_max {(cin, cout, L, B)} pro={use_pro}")


def make_adagn(cout, seed):
    from lion_amd.models.adagn import AdaGN
    torch.manual_seed(seed)
    cfg = SimpleNamespace(latent_pts=SimpleNamespace(style_dim=128, ada_mlp_init_scale=1.0))
    return AdaGN(2, cfg, cout).cuda()


@pytest.mark.parametrize("cin,cout,L,B", [k for k in pw.MAX_TABLE if k[1] % 8 == 0])
def test_max_recompute_equals_the_stored_path_bit_for_bit(cin, cout, L, B):
    """fused_ops.pwconv_max_recompute (sums, fold, activated maximum) == conv stored, folded, lion_affine_swish_max, at
    every channel tile (tests/test_fold_se_gpu.py has CB = 2 and 1 only)"""
    from lion_amd import fused_ops
    x, w, bias, pro = pw.make_data("unit", cin, cout, L, B, cin + cout, device="cuda")
    x = x.view(B, cin, L // 32, 32)
    conv, gn = conv_of(w, bias), make_adagn(cout, cout)
    style = torch.randn(B, 128, device="cuda")
    with torch.no_grad():
        got = fused_ops.pwconv_max_recompute(x, conv, gn, style, pro)
        y, st = fused_ops.pwconv_fused(x, conv, pro, split=False)
        f, g = gn.affine(style)
        A, Bs, _ = fused_ops.groupnorm_fold(st, gn.norm, f, g, L)
        want = fused_ops.affine_swish(y, A, Bs, reduce_max=True)
    assert got is not None and tuple(got.shape) == (B, cout, L // 32)
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,M,U,why", [(228, 125, 33, "L % 32 != 0"), (1, 128, 32, "L <= 4096"), (4, 129, 32, "grid below 2048")])
def test_max_recompute_declines_what_the_kernel_does_not_take(B, M, U, why):
    """LION_EUNSUPPORTED from the library, None from pwconv_max_recompute, and shared_mlp(reduce_max=True) gives the
    stored path's result with the switch on"""
    from lion_amd import fused_ops
    cin, cout, L = 6, 64, M * U
    x, w, bias, _ = pw.make_data("unit", cin, cout, L, B, L, device="cuda")
    conv, gn = conv_of(w, bias), make_adagn(cout, L)
    style = torch.randn(B, 128, device="cuda")
    assert forward_max(x, conv, None) is None, why
    x4 = x.view(B, cin, M, U)
    saved, orig, calls = fused_ops.MAX_RECOMPUTE, fused_ops.pwconv_max_recompute, []
    try:
        with torch.no_grad():
            assert orig(x4, conv, gn, style, None) is None, why
            fused_ops.MAX_RECOMPUTE = False
            want = fused_ops.shared_mlp(x4, [conv], [gn], style, reduce_max=True)
            fused_ops.MAX_RECOMPUTE = True
            fused_ops.pwconv_max_recompute = lambda *a, **k: calls.append(orig(*a, **k)) or calls[-1]
            got = fused_ops.shared_mlp(x4, [conv], [gn], style, reduce_max=True)
    finally:
        fused_ops.MAX_RECOMPUTE, fused_ops.pwconv_max_recompute = saved, orig
    assert calls == ([None] if U == 32 else [])      # attempted and declined (shared_mlp itself asks for 32 neighbours)
    assert torch.equal(got, want)
    assert tuple(got.shape) == (B, cout, M) and bool(torch.isfinite(got).all())


# ---- 5. containment of non-finite values ------------------------------------------------------------------------------

# odd and even Cin, a ragged last tile: the small kernel (70 = 2 * 32 + 6) and the large one (4100 = 8 * 512 + 4)
NAN_CASES = [(5, 33, 70, 3), (4, 64, 70, 3), (5, 33, 4100, 3), (4, 32, 4100, 3), (7, 128, 4100, 2), (6, 256, 4100, 2)]


def same(a, b):
    """bit-identical, NaN included"""
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("use_pro", [False, True])
@pytest.mark.parametrize("cin,cout,L,B", NAN_CASES)
def test_nan_stays_in_its_column_and_its_sample(cin, cout, L, B, use_pro):
    """both kernels load columns beyond L from column L - 1 and the padding of an odd Cin from channel Cin - 1, and select
    zero afterwards: a NaN there reaches what depends on it and nothing else"""
    x, w, bias, pro = pw.make_data("unit", cin, cout, L, B, cin + L, device="cuda")
    p = pro if use_pro else None
    conv = conv_of(w, bias)
    cols = pw.path(cin, cout, L, B)[1]
    T = math.ceil(L / cols)
    y0, st0 = run(x, conv, p)
    assert bool(torch.isfinite(y0).all()) and bool(torch.isfinite(st0).all())
    # column L - 1 of every sample and channel
    xn = x.clone()
    xn[:, :, L - 1] = NAN
    y, st = run(xn, conv, p)
    assert same(y[:, :, :L - 1], y0[:, :, :L - 1]) and bool(torch.isnan(y[:, :, L - 1]).all())
    assert same(st[:, :, :T - 1], st0[:, :, :T - 1]) and bool(torch.isnan(st[:, :, T - 1]).all())
    # channel Cin - 1 of sample 1: every output of that sample, nothing of the others
    xn = x.clone()
    xn[1, cin - 1] = NAN
    y, st = run(xn, conv, p)
    assert bool(torch.isnan(y[1]).all()) and bool(torch.isnan(st[1]).all())
    for b in (0,) + tuple(range(2, B)):
        assert same(y[b], y0[b]) and same(st[b], st0[b])
    # one element of channel Cin - 1: its column of that sample and that column's tile
    xn = x.clone()
    xn[1, cin - 1, cols] = NAN
    y, st = run(xn, conv, p)
    keep = torch.ones(L, dtype=torch.bool, device="cuda")
    keep[cols] = False
    assert same(y[:, :, keep], y0[:, :, keep]) and bool(torch.isnan(y[1, :, cols]).all()) and same(y[0, :, cols], y0[0, :, cols])
    tk = torch.ones(T, dtype=torch.bool, device="cuda")
    tk[1] = False
    assert same(st[:, :, tk], st0[:, :, tk]) and bool(torch.isnan(st[1, :, 1]).all()) and same(st[0, :, 1], st0[0, :, 1])


@pytest.mark.parametrize("cin,cout,L,B", NAN_CASES[:1] + NAN_CASES[2:3])
def test_saturated_prologue_is_finite_and_at_its_limit(cin, cout, L, B):
    """prologue arguments of +-100 and +-1e4 (x = +-1, a = 100 | 1e4, b = 0): swish_fast is at its float64 limit, 0 or t,
    e^-t overflowing or not, and y within the bound"""
    x, w, bias, _ = pw.make_data("unit", cin, cout, L, B, 11, device="cuda")
    x = torch.sign(x) + (x == 0)
    a = torch.tensor([100.0, 1e4], device="cuda")[torch.arange(B * cin, device="cuda") % 2].view(B, cin)
    pro = (a, torch.zeros_like(a))
    xin, _ = pw.operand64(x, pro)
    t = x.double() * a.double()[:, :, None]
    assert bool(((xin - torch.where(t > 0, t, torch.zeros_like(t))).abs() <= 1e-30).all())
    y, st = run(x, conv_of(w, bias), pro)
    ref, bound = pw.pwconv64(x, w, bias, pro)
    cols = pw.path(cin, cout, L, B)[1]
    sref, sbound = pw.tile_stats64(ref, bound, cols)
    within({"y": worst(y, ref, bound), "s1": worst(st[..., 0], sref[..., 0], sbound[..., 0]),
            "s2": worst(st[..., 1], sref[..., 1], sbound[..., 1])}, f"saturated prologue {(cin, cout, L, B)}")


# ---- 6. the linear kernel and the pack kernel ---------------------------------------------------------------------

def pack(w):
    from lion_amd import _lib
    cout, cin = w.shape
    wp = torch.full((lib().lion_pwconv_packed_floats(cout, cin),), NAN, device="cuda")
    _lib.call("lion_pwconv_pack_weights", w.contiguous(), cout, cin, wp)
    return wp


def linear(x, wp, bias, O, act, slope):
    from lion_amd import _lib
    B, K = x.shape
    y = torch.full((B, O), NAN, device="cuda")
    _lib.call("lion_linear_forward", x, wp, bias, B, K, O, act, slope, y)
    return y


LIN_B, LIN_K, LIN_O = (1, 31, 32, 33, 70), (1, 2, 3, 129), (1, 31, 33, 64, 65)   # K = 1, 2, 3: fewer k-steps than waves


@pytest.mark.parametrize("act,slope", [(0, 0.0), (1, 0.0), (2, 0.25), (2, 0.0), (2, -0.0)])
def test_linear_integers_are_exact(act, slope):
    """integer x, W, bias (|sum| <= 2 K + 3, exact in fp32); slopes with exact products; a zero row of W with a zero
    (and a negative zero) bias puts the pre-activation exactly at 0, where the leaky branch gives 0 whatever the slope"""
    g = torch.Generator(device="cuda").manual_seed(act)
    for K in LIN_K:
        for O in LIN_O:
            w = torch.randint(-1, 2, (O, K), generator=g, device="cuda").float()
            bias = torch.randint(-3, 4, (O,), generator=g, device="cuda").float()
            w[O // 2], bias[O // 2] = 0.0, 0.0 if O % 2 else -0.0
            wp = pack(w)
            for B in LIN_B:
                x = torch.randint(-2, 3, (B, K), generator=g, device="cuda").float()
                for b in (bias, None):
                    pre = x.double() @ w.double().t() + (0.0 if b is None else b.double())
                    got = linear(x, wp, b, O, act, slope)
                    assert torch.equal(got.double(), pw.act64(pre, act, slope)), (B, K, O)
                    assert bool((got[:, O // 2] == 0).all())


@pytest.mark.parametrize("act", [0, 1, 2])
def test_linear_against_float64(act):
    g = torch.Generator(device="cuda").manual_seed(100 + act)
    r = 0.0
    for K in LIN_K:
        for O in LIN_O:
            w = torch.randn(O, K, generator=g, device="cuda") / math.sqrt(K)
            w = w * 10.0 ** (torch.rand(O, generator=g, device="cuda") * 4 - 2)[:, None]     # rows of disparate magnitudes
            bias = torch.randn(O, generator=g, device="cuda") * 0.1
            wp = pack(w)
            for B in LIN_B:
                x = torch.randn(B, K, generator=g, device="cuda")
                for b in (bias, None):
                    ref, bound = pw.linear64(x, w, b, act, 0.1)
                    r = max(r, worst(linear(x, wp, b, O, act, 0.1), ref, bound))
    within({"y": r}, f"linear act={act}")


@pytest.mark.parametrize("cout,cin", [(1, 1), (31, 3), (33, 2), (64, 5), (65, 129), (96, 35), (320, 259)])
def test_packed_weights_are_the_documented_layout(cout, cin):
    """[Cout, Cin] -> k-major [ceil2(Cin), ceil64(Cout)], the padding zero, element for element"""
    w = (torch.arange(cout * cin, device="cuda", dtype=torch.float32) + 1.0).view(cout, cin)
    want = pw.packed_layout(w)
    got = pack(w)
    assert got.numel() == want.numel() == (cin + 1) // 2 * 2 * ((cout + 63) // 64 * 64)
    assert torch.equal(got.view_as(want), want)
