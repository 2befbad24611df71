"""-m gpu: the skinny (32-column) GEMM of the global denoiser, csrc/skinny.hip, through its C entry points at the channel
counts where its code takes another path -- one k-step, idle waves, a partly filled round of 16 k-steps, a second and a
third round, every number of k-splits -- with 1 to 8 input partials, against an exact integer evaluation and against
float64 with a bound per output element.  Then the module that routes to it, at widths the kernel does not take."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

# (Cin, Cout) -> (k-splits KS, k-steps per wave, rounds of 16 k-steps) the kernel takes there
TABLE = {
    (1, 32): (1, 4, 1), (2, 32): (1, 4, 1), (3, 32): (1, 4, 1), (7, 32): (1, 4, 1),  # one k-step, 15 of 16 waves idle, odd last k
    (9, 64): (1, 4, 1),                                                           # the 8-k chunk boundary
    (33, 32): (1, 4, 1), (65, 32): (1, 4, 1),                                     # some waves idle
    (129, 32): (1, 8, 1),                                                         # half-filled round
    (257, 64): (1, 12, 1),                                                        # 3/4-filled round
    (510, 32): (1, 16, 1), (511, 32): (2, 8, 1),                                  # the first split boundary
    (513, 32): (2, 12, 1),                                                        # idle waves in the second split
    (1025, 64): (4, 12, 1),
    (2049, 32): (8, 12, 1),
    (4099, 32): (8, 20, 2), (4100, 32): (8, 20, 2),                               # second round, 4 live steps of 16
    (1099, 4128): (1, 36, 3),                                                     # three rounds, the last partly filled
}
SHAPES = sorted(TABLE)
BATCH = {1: 32, 3: 70}   # nb -> batch; 70 samples leave columns 70..95 of the third slab as padding
KS_IN = (1, 2, 3, 4, 5, 8)
EPS = 2.0 ** -23

# |got - ref| <= TOL * M per output element, M the sum of the absolute products behind it (see gemm_refs).
# TOL is 8 x the worst ratio that a plain fp32 torch evaluation of the same expression reaches against float64 on the
# same inputs, where that is below the project's 1e-5 (8 x: the kernel sums in another order, sixteen waves x k-splits).
# Measured on the MI355X over test_gemm_against_float64's cases (err / M, worst over shapes and options):
#                          fp32 torch   kernel
#     unit                 3.08e-7      1.72e-7
#     row-disparity        3.01e-7      1.80e-7
#     cancelling-partials  1.86e-7      8.86e-8
#     relu-edge            1.62e-7      9.05e-8
# (the kernel's ratio falls with Cin, 1.5e-7 at Cin = 1 to 1.4e-8 at Cin = 4100; torch's stays between 6e-8 and 3.1e-7)
TOL = 8 * 3.084e-7
# lion_skinny_finish alone: the project's bound.  At most 9 sequential fp32 additions per element, <= 9 * 2^-24 = 5.4e-7 of
# the sum of their magnitudes in the worst case; measured worst 1.9e-7 (mode 0) and 0.33 of the mode-1 bound, in which the
# last rounding's eps * |resid| is the larger part.  (test_gemm_se_finish_against_float64, on TOL: 0.41 of its bound.)
FINISH_TOL = 1e-5


def lib():
    from lion_amd import _lib
    return _lib.load()


def plan(cin, cout):
    """lion_skinny_splits and the k-steps per wave / rounds of skinny_gemm_kernel, recomputed from their formulas"""
    tiles, ksteps = cout // 32, (cin + 1) // 2
    ks = 1
    while ks < 8 and tiles * ks * 2 <= 256 and ksteps // (ks * 2 * 16) >= 8:
        ks *= 2
    per = ((ksteps + ks * 16 - 1) // (ks * 16) + 3) & ~3
    return ks, per, (per + 15) // 16


def test_shape_table_reaches_every_path_of_the_kernel():
    """keeps the table on the partly filled and the repeated rounds if the split heuristics change"""
    for (cin, cout), want in TABLE.items():
        assert plan(cin, cout) == want, (cin, cout, plan(cin, cout))
        assert lib().lion_skinny_splits(cin, cout) == want[0], (cin, cout)
    assert lib().lion_skinny_splits(510, 32) == 1 and lib().lion_skinny_splits(511, 32) == 2
    pers = {p for _, p, _ in TABLE.values()}
    assert {4, 8, 12, 16, 20} <= pers, pers
    assert max(r for _, _, r in TABLE.values()) >= 2
    assert {k for k, _, _ in TABLE.values()} == {1, 2, 4, 8}
    assert lib().lion_skinny_splits(2048, 256) == 8   # SE.fc[0] of the released model: eight partials into the next layer


# ---- the entry points, called as the C header declares them -----------------------------------------------------------

def pack(w):
    from lion_amd import _lib
    cout, cin = w.shape
    wp = torch.empty(lib().lion_skinny_packed_floats(cout, cin), device="cuda", dtype=torch.float32)
    _lib.call("lion_skinny_pack_weights", w.contiguous(), cout, cin, wp)
    return wp


def gemm(pin, bias_in, act_in, addT, wp, cout):
    from lion_amd import _lib
    ks_in, nb, cin, _ = pin.shape
    out = torch.full((lib().lion_skinny_splits(cin, cout), nb, cout, 32), float("nan"), device="cuda")
    _lib.call("lion_skinny_gemm", pin, ks_in, bias_in, act_in, addT, wp, nb, cin, cout, out)
    return out


def finish(A, bias_a, Bp=None, resid=None):
    from lion_amd import _lib
    ks_a, nb, c, _ = A.shape
    y = torch.full((nb, c, 32), float("nan"), device="cuda")
    _lib.call("lion_skinny_finish", A, ks_a, bias_a, Bp, 0 if Bp is None else Bp.shape[0], resid, nb, c,
              0 if Bp is None else 1, y)
    return y


def gemm_se_finish(pin, bias_in, act_in, wp, cout, A, bias_a, resid):
    from lion_amd import _lib
    ks_in, nb, cin, _ = pin.shape
    y = torch.full((nb, cout, 32), float("nan"), device="cuda")
    _lib.call("lion_skinny_gemm_se_finish", pin, ks_in, bias_in, act_in, wp, nb, cin, cout, A, A.shape[0], bias_a, resid, y)
    return y


def channel_major(rows):
    """[B, C] -> [nb, C, 32], the batch zero-padded (the torch formulation)"""
    from lion_amd import fused_ops
    return fused_ops.to_channel_major(rows)


def operand(pin, bias_in, act_in, addT, dtype):
    x = pin.to(dtype).sum(0)
    if bias_in is not None:
        x = x + bias_in.to(dtype)[None, :, None]
    if act_in:
        x = torch.relu(x)
    return x if addT is None else x + addT.to(dtype)


def gemm_refs(w, pin, bias_in, act_in, addT, bias):
    """W (act(sum_q pin + bias_in) + add) + bias in float64, the same in fp32 torch, and M[o, b] = sum_k |w[o, k]|
    (sum_q |pin_q[k, b]| + |bias_in[k]| + |add[k, b]|) + |bias[o]|"""
    def mm(w_, x_):
        return torch.einsum("ok,nkb->nob", w_, x_)
    ref = mm(w.double(), operand(pin, bias_in, act_in, addT, torch.float64)) + bias.double()[None, :, None]
    ref32 = mm(w, operand(pin, bias_in, act_in, addT, torch.float32)) + bias[None, :, None]
    mag = pin.double().abs().sum(0)
    if bias_in is not None:
        mag = mag + bias_in.double().abs()[None, :, None]
    if addT is not None:
        mag = mag + addT.double().abs()
    M = mm(w.double().abs(), mag) + bias.double().abs()[None, :, None]
    return ref, ref32, M


def gen_for(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()) & 0x7fffffff)


# ---- 1. integers: every product and sum exact, no tolerance ---------------------------------------------------------

def ints(gen, *shape):
    return torch.randint(-2, 3, shape, device="cuda", generator=gen).float()


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_gemm_of_small_integers_is_exact(cin, cout, nb):
    """weights, partials, biases and the added tensor are integers in [-2, 2]: every fp32 product and partial sum is an
    integer below 2^24 (|sum| <= 4100 * 2 * 20), exact in any order, so lion_skinny_gemm + lion_skinny_finish must equal
    the integer evaluation bit for bit -- any dropped, doubled or misplaced k shows.  The matrix product of the reference
    runs on float64 holding integers below 2^53, the element-wise part on int64."""
    gen = gen_for(cin, cout, nb)
    B = BATCH[nb]
    w = ints(gen, cout, cin)
    wp = pack(w)
    bias = ints(gen, cout)
    bias_in = ints(gen, cin)
    addT = channel_major(ints(gen, B, cin))
    pin8 = torch.stack([channel_major(ints(gen, B, cin)) for _ in range(max(KS_IN))])
    for ks_in in KS_IN:
        pin = pin8[:ks_in].contiguous()
        for act_in in (0, 1):
            for bi in (None, bias_in):
                for ad in (None, addT):
                    x = pin.long().sum(0)
                    if bi is not None:
                        x = x + bi.long()[None, :, None]
                    if act_in:
                        x = x.clamp(min=0)
                    if ad is not None:
                        x = x + ad.long()
                    ref = (torch.einsum("ok,nkb->nob", w.double(), x.double()) + bias.double()[None, :, None]).long()
                    got = finish(gemm(pin, bi, act_in, ad, wp, cout), bias)
                    tag = (cin, cout, nb, ks_in, act_in, bi is not None, ad is not None)
                    assert torch.equal(got, ref.float()), (tag, int((got != ref.float()).sum()))
                    assert torch.equal(got.long(), ref), tag


# ---- 2. float64 with a bound per element -----------------------------------------------------------------------------

DATA = ("unit", "row-disparity", "cancelling-partials", "relu-edge")
# (ks_in, act_in, bias_in, addT): every ks_in of the integer test, the options thinner
OPTIONS = ((1, 0, False, False), (2, 1, True, True), (3, 1, True, False), (4, 0, True, True), (5, 1, True, True),
           (8, 1, True, False), (8, 0, False, True))


def float_case(cin, cout, nb, ks_in, with_bias_in, with_add, data, gen):
    B = BATCH[nb]

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen)
    w = rn(cout, cin)
    if data == "row-disparity":   # rows of the weights over eight decades
        w = w * (10.0 ** torch.linspace(-4, 4, cout, device="cuda"))[:, None]
    bias = rn(cout) * w.abs().amax(1)
    bias_in = rn(cin) if with_bias_in else None
    parts = [rn(B, cin) for _ in range(ks_in)]
    if data == "cancelling-partials":   # partials of size 1e3 whose sum is O(1)
        parts = [1e3 * p for p in parts]
        parts[-1] = rn(B, cin) - sum(parts[:-1])
    if data == "relu-edge":   # the sum under the ReLU within a few ulp of zero, on both sides
        s = sum(p.double() for p in parts[:-1]) + bias_in.double()[None, :]
        j = torch.randint(-3, 4, (B, cin), device="cuda", generator=gen)
        parts[-1] = (-s).float() * (1.0 + j.float() * EPS)
    pin = torch.stack([channel_major(p) for p in parts])
    addT = channel_major(rn(B, cin)) if with_add else None
    return w, bias, bias_in, pin, addT


def float_cases(cin, cout, nb):
    for data in DATA:
        for ks_in, act_in, with_bias_in, with_add in OPTIONS:
            if data == "cancelling-partials" and ks_in < 2:
                continue
            if data == "relu-edge" and not (act_in and with_bias_in):
                continue
            gen = gen_for(cin, cout, nb, data, ks_in, act_in)
            yield (data, ks_in, act_in, with_bias_in, with_add), float_case(cin, cout, nb, ks_in, with_bias_in, with_add, data, gen)


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_gemm_against_float64(cin, cout, nb):
    """lion_skinny_gemm + lion_skinny_finish (mode 0) within TOL of the float64 evaluation, measured per output element
    against the sum of the absolute products behind that element -- a wrong row next to a large one, or a wrong column
    of the padding, is not hidden by a maximum over the tensor"""
    worst_k = worst_t = 0.0
    for tag, (w, bias, bias_in, pin, addT) in float_cases(cin, cout, nb):
        act_in = tag[2]
        ref, ref32, M = gemm_refs(w, pin, bias_in, act_in, addT, bias)
        got = finish(gemm(pin, bias_in, act_in, addT, pack(w), cout), bias)
        assert torch.isfinite(got).all(), tag
        rk = ((got.double() - ref).abs() / M).max().item()
        rt = ((ref32.double() - ref).abs() / M).max().item()
        print(f"skinny gemm {cin}x{cout} nb={nb} {tag}: kernel {rk:.3e} fp32-torch {rt:.3e}")
        worst_k, worst_t = max(worst_k, rk), max(worst_t, rt)
        assert rk <= TOL, (tag, rk, rt)
    print(f"skinny gemm {cin}x{cout} nb={nb} WORST: kernel {worst_k:.3e} fp32-torch {worst_t:.3e}")


# ---- 3. the GEMM with the block's tail in its epilogue ----------------------------------------------------------------

GATES = (100.0, -100.0, 200.0, -200.0)   # pre-activations of the sigmoid in output rows 0..3


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("cin,cout", [(256, 2048), (8, 64), (33, 32), (129, 96)])
def test_gemm_se_finish_against_float64(cin, cout, nb):
    """y = resid + relu(sum_q A[q] + bias_a) * sigmoid(W act(sum_q pin[q] + bias_in)) against float64 with the bound of
    the GEMM test carried through the tail: |relu(a)| * 0.25 * err_g + err_a + eps * |resid| (0.25 bounds the slope of the
    sigmoid).  Four rows of W hold one entry only, on an operand row of ones: gate pre-activations of exactly +-100 and
    +-200, where expf overflows or underflows and the gate must come out as 0 or 1, not as NaN.  And the same launch
    against lion_skinny_gemm + lion_skinny_finish (mode 1), which it must equal bit for bit."""
    assert lib().lion_skinny_splits(cin, cout) == 1
    gen = gen_for(cin, cout, nb, "se")

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen)
    w = rn(cout, cin)
    w[:4] = 0.0
    w[:4, 0] = torch.tensor(GATES, device="cuda")
    wp = pack(w)
    pin8, A8 = rn(8, nb, cin, 32), rn(8, nb, cout, 32)
    pin8[:, :, 0] = 0.0
    pin8[0, :, 0] = 1.0          # operand row 0 is 1 with either act_in
    bias_in, bias_a, resid = rn(cin), rn(cout), rn(nb, cout, 32)
    bias_in[0] = 0.0
    zero = torch.zeros(cout, device="cuda")
    worst = 0.0
    for ks_in in (1, 2, 4, 5, 8):
        pin = pin8[:ks_in].contiguous()
        for act_in in (0, 1):
            for bi in (None, bias_in):
                g64, _, Mg = gemm_refs(w, pin, bi, act_in, None, zero)
                assert torch.equal(g64[:, :4, :], torch.tensor(GATES, device="cuda").double()[None, :, None].expand(nb, 4, 32))
                two = gemm(pin, bi, act_in, None, wp, cout)
                for ks_a in (1, 4, 8):
                    A = A8[:ks_a].contiguous()
                    for ba in (None, bias_a):
                        a64 = A.double().sum(0) + (0.0 if ba is None else ba.double()[None, :, None])
                        Ma = A.double().abs().sum(0) + (0.0 if ba is None else ba.double().abs()[None, :, None])
                        ref = resid.double() + torch.relu(a64) * torch.sigmoid(g64)
                        bound = torch.relu(a64) * 0.25 * TOL * Mg + TOL * Ma + EPS * resid.double().abs()
                        got = gemm_se_finish(pin, bi, act_in, wp, cout, A, ba, resid)
                        tag = (cin, cout, nb, ks_in, act_in, bi is not None, ks_a, ba is not None)
                        assert torch.isfinite(got).all(), tag
                        r = ((got.double() - ref).abs() / bound).max().item()
                        worst = max(worst, r)
                        assert r <= 1.0, (tag, r)
                        assert torch.equal(got, finish(A, ba, two, resid)), tag
    print(f"skinny se_finish {cin}x{cout} nb={nb}: worst error / bound {worst:.3f}")


# ---- 4. the finish kernel alone -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("C", [1, 7, 33])
def test_finish_alone_against_float64(C, nb):
    """lion_skinny_finish takes any C: element counts that are no multiple of its 256-thread blocks, up to 8 partials on
    both inputs, both modes"""
    gen = gen_for(C, nb, "finish")

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen)
    A8, B8, bias, resid = rn(8, nb, C, 32), rn(8, nb, C, 32), rn(C), rn(nb, C, 32)
    worst0 = worst1 = 0.0
    for ks_a in (1, 2, 5, 8):
        A = A8[:ks_a].contiguous()
        for ba in (None, bias):
            a64 = A.double().sum(0) + (0.0 if ba is None else ba.double()[None, :, None])
            Ma = A.double().abs().sum(0) + (0.0 if ba is None else ba.double().abs()[None, :, None])
            r0 = ((finish(A, ba).double() - a64).abs() / Ma).max().item()
            worst0 = max(worst0, r0)
            assert r0 <= FINISH_TOL, (C, nb, ks_a, "mode 0", r0)
            for ks_b in (1, 3, 8):
                Bp = B8[:ks_b].contiguous()
                g64, Mg = Bp.double().sum(0), Bp.double().abs().sum(0)
                ref = resid.double() + torch.relu(a64) * torch.sigmoid(g64)
                bound = torch.relu(a64) * 0.25 * FINISH_TOL * Mg + FINISH_TOL * Ma + EPS * resid.double().abs()
                r1 = ((finish(A, ba, Bp, resid).double() - ref).abs() / bound).max().item()
                worst1 = max(worst1, r1)
                assert r1 <= 1.0, (C, nb, ks_a, ks_b, "mode 1", r1)
    print(f"skinny finish C={C} nb={nb}: mode 0 worst error / M {worst0:.3e}, mode 1 worst error / bound {worst1:.3f}")


# ---- 5. a NaN stays in its column ------------------------------------------------------------------------------------

def only_column_differs(got, clean, slab, col):
    """column (slab, col) of got is NaN in every row, everything else is clean's bit for bit"""
    keep = torch.ones(got.shape[0], 1, 32, dtype=torch.bool, device="cuda")
    keep[slab, 0, col] = False
    keep = keep.expand_as(got)
    return bool(torch.isnan(got[slab, :, col]).all()) and torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("act_in", [0, 1])
@pytest.mark.parametrize("cin,cout,nb", [(3, 32, 1), (33, 32, 3), (513, 32, 1), (4099, 32, 3), (1099, 4128, 1)])
def test_nan_in_the_last_input_channel_stays_in_its_column(cin, cout, nb, act_in):
    """k = Cin - 1 of an odd Cin is the element that lanes beyond the end re-read (the min(kc, Cin - 1) clamp) before
    their operand is zeroed: a NaN there must reach its own batch column through the one live lane and no other column
    through the dead ones.  With act_in = 1 it passes the ReLU first, which keeps it as torch's does (written as
    v > 0 ? v : 0 the ReLU returned 0 there, and the column came out finite)."""
    gen = gen_for(cin, cout, nb, "nan")
    w = torch.randn(cout, cin, device="cuda", generator=gen)
    bias = torch.randn(cout, device="cuda", generator=gen)
    pin = torch.randn(2, nb, cin, 32, device="cuda", generator=gen)
    wp = pack(w)
    clean = finish(gemm(pin, None, act_in, None, wp, cout), bias)
    assert torch.isfinite(clean).all()
    slab, col = nb - 1, 5
    pin[1, slab, cin - 1, col] = float("nan")
    got = finish(gemm(pin, None, act_in, None, wp, cout), bias)
    assert only_column_differs(got, clean, slab, col)


def test_nan_under_the_relu_of_the_tail_reaches_the_output():
    """relu(sum_q A[q] + bias_a) of the block's tail keeps a NaN too: one element of the output, in lion_skinny_finish and
    in the epilogue of lion_skinny_gemm_se_finish alike"""
    cin, cout, nb = 33, 64, 3
    gen = gen_for("nan tail")
    w = torch.randn(cout, cin, device="cuda", generator=gen)
    pin = torch.randn(2, nb, cin, 32, device="cuda", generator=gen)
    A = torch.randn(4, nb, cout, 32, device="cuda", generator=gen)
    bias_a = torch.randn(cout, device="cuda", generator=gen)
    resid = torch.randn(nb, cout, 32, device="cuda", generator=gen)
    wp = pack(w)
    clean = gemm_se_finish(pin, None, 1, wp, cout, A, bias_a, resid)
    assert torch.isfinite(clean).all()
    A[2, 1, 40, 7] = float("nan")
    one = torch.zeros_like(clean, dtype=torch.bool)
    one[1, 40, 7] = True
    for got in (gemm_se_finish(pin, None, 1, wp, cout, A, bias_a, resid),
                finish(A, bias_a, gemm(pin, None, 1, None, wp, cout), resid)):
        assert torch.isnan(got[one]).all() and torch.equal(got[~one], clean[~one])


# ---- 6. the packed-weight cache ------------------------------------------------------------------------------------------

def test_skinny_conv_sees_an_in_place_weight_update():
    from lion_amd import fused_ops
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(65, 64, 1).cuda()
    x = torch.randn(1, 65, 32, device="cuda")
    with torch.no_grad():
        first = fused_ops.skinny_conv(x, conv)
        conv.weight.mul_(2)
        second = fused_ops.skinny_conv(x, conv)
    assert first.abs().max().item() > 0
    assert torch.equal(second, first * 2)   # a power of two: exact


# ---- 7. the module at widths the kernel does not take ----------------------------------------------------------------

def make_prior(nf, style, cells):
    from conftest import fill_
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.score_sde.resnet import PriorSEDrop
    cfg = released_prior_cfg()
    cfg.sde.num_channels_dae = nf
    cfg.sde.num_cell_per_scale_dae = cells
    m = PriorSEDrop(cfg.sde, style, cfg)
    fill_(m)
    return m.cuda().eval()


def both_paths(m, style, B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, style, 1, 1, device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g) * 0.98 + 0.01
    with torch.no_grad():
        got = m(x=x, t=t, condition_input=None, clip_feat=None)
    with torch.enable_grad():
        ref = m(x=x, t=t, condition_input=None, clip_feat=None).detach()
    return got, ref


@pytest.mark.parametrize("B", [5, 40])
@pytest.mark.parametrize("nf,style", [(64, 128), (256, 100), (96, 128)])
def test_narrow_or_odd_width_prior_takes_the_torch_path(nf, style, B, monkeypatch):
    """an SE hidden width of 8 or 12, or a style width of 100, is no multiple of the kernel's 32-channel tile: the module
    in eval() + no_grad() must give what its grad-mode formulation gives, not raise"""
    from lion_amd import fused_ops
    calls = []
    real = fused_ops.skinny_conv
    monkeypatch.setattr(fused_ops, "skinny_conv", lambda *a, **k: calls.append(1) or real(*a, **k))
    m = make_prior(nf, style, 2)
    got, ref = both_paths(m, style, B, nf + style + B)
    assert got.shape == ref.shape == (B, style, 1, 1)
    assert not calls
    assert (got - ref).abs().max().item() / ref.abs().max().item() < 1e-4


def test_released_width_prior_still_takes_the_skinny_path(monkeypatch):
    from lion_amd import fused_ops
    calls = []
    real = fused_ops.skinny_conv
    monkeypatch.setattr(fused_ops, "skinny_conv", lambda *a, **k: calls.append(1) or real(*a, **k))
    m = make_prior(2048, 128, 1)
    got, ref = both_paths(m, 128, 5, 3)
    assert len(calls) >= 4   # input and output layer, conv1, conv2, SE fc1 (SE fc2 goes through skinny_conv_se_finish)
    assert (got - ref).abs().max().item() / ref.abs().max().item() < 1e-4
