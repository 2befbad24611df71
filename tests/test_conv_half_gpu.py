"""-m gpu: the single-product fp16 voxel convolution (csrc/conv3d_half.hip, lion_conv3d_k3_half_forward) -- the kernel behind
conv_ops.PRECISION = "half".  With the split kernel's power-of-two block scaling a hi piece is the operand rounded to an
11-bit significand (round to nearest even) at any magnitude, so the kernel computes conv(rne11(W), rne11(X)) with fp32
accumulation.  Two derived yardsticks, float64 convolutions on the CPU:
  sharp:        |y - conv64(rne11 W, rne11 X)| < 5e-6 max          (the fp32-class bound of tests/test_conv_split_gpu.py)
  elementwise:  |y - conv64(W, X)| <= 2^-10 conv64(|W|, |X|) + 5e-6 max   (two roundings of 2^-11 each)
and the distance from the exact result must EXCEED 5e-6 max: the mode is really on."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 5e-6
SHAPES = [(16, 2, 32, 64),    # two chunks: the monotone rescale can run; CB = 2
          (16, 2, 16, 32),    # CB = 1
          (32, 2, 16, 32),
          (32, 1, 64, 64)]    # the production instantiation


def rne11(t):
    """round to an 11-bit significand, ties to even, whatever the exponent (float64 result)"""
    m, e = torch.frexp(t.double())
    return torch.ldexp(torch.round(m * 2048.0) / 2048.0, e)


def conv64(x, w, bias=None):
    return F.conv3d(x.double().cpu(), w.double().cpu(), None if bias is None else bias.double().cpu(), padding=1)


def make(r, B, cin, cout, seed=0, bias=True):
    torch.manual_seed(seed + 7 * cin + cout + r)
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1, bias=bias).cuda()
    x = torch.randn(B, cin, r, r, r, device="cuda")
    return conv, x


def half_forward(x, weight, bias=None, pro=None, pbias=None, tconst=None, stats_tiles=0, occ=None):
    """the C entry point itself, on the split pack of `weight`"""
    from lion_amd import _lib, conv_ops
    b, cin, r = x.shape[0], x.shape[1], x.shape[2]
    cout = weight.shape[0]
    wp = conv_ops.split_packed_weight(weight)
    y = torch.empty((b, cout, r, r, r), device="cuda")
    st = torch.empty((b, cout, stats_tiles, 2), device="cuda") if stats_tiles else None
    pa, pb = (None, None) if pro is None else (pro[0].contiguous(), pro[1].contiguous())
    _lib.call("lion_conv3d_k3_half_forward", x.contiguous(), wp, None if bias is None else bias.detach().contiguous(),
              b, cin, cout, r, pa, pb, pbias, tconst, y, st, occ)
    return y, st


def inside_elementwise(y, exact, absprod, what):
    """|y - exact| <= 2^-10 absprod + 5e-6 max|exact|, elementwise; prints the largest ratio to the rounding term"""
    d = (y.double().cpu() - exact).abs()
    slack = BOUND * exact.abs().max()
    ratio = ((d - slack).clamp(min=0) / (2.0 ** -10 * absprod).clamp(min=1e-300)).max().item()
    print(f"{what}: max |err| / (2^-10 sum|w||x|) beyond the fp32 slack = {ratio:.3f}; "
          f"max |err| / max = {(d.max() / exact.abs().max()).item():.3e}")
    assert torch.isfinite(y).all(), what
    assert bool((d <= 2.0 ** -10 * absprod + slack).all()), (what, ratio)


@pytest.mark.parametrize("r,B,cin,cout", SHAPES)
def test_half_plain_form_against_float64(r, B, cin, cout):
    conv, x = make(r, B, cin, cout)
    with torch.no_grad():
        y, _ = half_forward(x, conv.weight, conv.bias)
        emul = conv64(rne11(x), rne11(conv.weight), conv.bias)
        exact = conv64(x, conv.weight, conv.bias)
        absprod = conv64(x.abs(), conv.weight.abs())
    mx = exact.abs().max().item()
    e_emul = (y.double().cpu() - emul).abs().max().item() / mx
    e_exact = (y.double().cpu() - exact).abs().max().item() / mx
    print(f"r={r} {cin}->{cout}: |y - conv64(rne11 W, rne11 X)| / max = {e_emul:.3e}, |y - conv64(W, X)| / max = {e_exact:.3e}")
    assert e_emul < BOUND, e_emul
    inside_elementwise(y, exact, absprod, "plain")
    assert e_exact > BOUND, e_exact      # one product, not three: the precision IS reduced


def test_half_scale_invariance_is_exact():
    """conv(x 2^k) == conv(x) 2^k and conv_{w 2^k}(x) == conv_w(x) 2^k bit for bit: no range in which the cut clamps,
    flushes or changes its rounding"""
    conv, x = make(16, 2, 32, 64, bias=False)
    with torch.no_grad():
        base, _ = half_forward(x, conv.weight)
        assert torch.isfinite(base).all()
        for k in (-80, 40):
            f = 2.0 ** k
            assert torch.equal(half_forward(x * f, conv.weight)[0], base * f), k
            assert torch.equal(half_forward(x, (conv.weight * f).contiguous())[0], base * f), k


@pytest.mark.parametrize("factor", [3.0e6, 1.0e-30])
def test_half_adversarial_ranges_stay_finite_and_inside_the_bound(factor):
    """activations far beyond fp16's 65504 and far below its smallest subnormal: the block scale carries them"""
    conv, x = make(16, 2, 32, 64, seed=5, bias=False)
    with torch.no_grad():
        x = (x * factor).contiguous()
        y, _ = half_forward(x, conv.weight)
        inside_elementwise(y, conv64(x, conv.weight), conv64(x.abs(), conv.weight.abs()), f"x * {factor:g}")


def test_half_nonfinite_inputs_reach_exactly_their_windows():
    conv, x = make(16, 2, 16, 32)
    x[0, 3, 2, 2, 2] = float("inf")
    x[1, 7, 12, 12, 12] = float("nan")
    clean = x.clone()
    clean[0, 3, 2, 2, 2] = 0.0
    clean[1, 7, 12, 12, 12] = 0.0
    with torch.no_grad():
        y, _ = half_forward(x, conv.weight, conv.bias)
        hit = torch.zeros_like(y, dtype=torch.bool)
        hit[0, :, 1:4, 1:4, 1:4] = True
        hit[1, :, 11:14, 11:14, 11:14] = True
        assert torch.equal(~torch.isfinite(y), hit)
        # the rest -- the rest of the same workgroup tiles included -- is as accurate as without the poison
        emul = conv64(rne11(clean), rne11(conv.weight), conv.bias)
    d = (y.double().cpu() - emul).abs()[~hit.cpu()]
    assert d.max().item() < BOUND * emul.abs().max().item()


@pytest.mark.parametrize("r,B,cin,cout", SHAPES)
def test_half_prologue_and_tile_sums(r, B, cin, cout):
    """swish(x A + Bs) applied while staging, per-tile channel sums in the epilogue.  The output is held to the elementwise
    bound around the float64 activation (not to the sharp one: one ulp in the kernel's activation can flip an 11-bit
    rounding); the sums to float64 sums of the kernel's own output."""
    from lion_amd import _lib
    conv, x = make(r, B, cin, cout, seed=1)
    A = torch.rand(B, cin, device="cuda") + 0.5
    Bs = torch.randn(B, cin, device="cuda") * 0.5
    tiles = _lib.load().lion_conv3d_split_stat_tiles(r, cout)
    with torch.no_grad():
        y, st = half_forward(x, conv.weight, conv.bias, pro=(A, Bs), stats_tiles=tiles)
        act = F.silu(x.double().cpu() * A.double().cpu().view(B, cin, 1, 1, 1) + Bs.double().cpu().view(B, cin, 1, 1, 1))
        exact = conv64(act, conv.weight, conv.bias)
        inside_elementwise(y, exact, conv64(act.abs(), conv.weight.abs()), "prologue")
    sums = st.double().sum(2)
    yd = y.double().flatten(2)
    scale = yd.abs().max().item()
    assert torch.allclose(sums[..., 0], yd.sum(-1), rtol=1e-4, atol=1e-5 * scale * (r ** 3) ** 0.5)
    assert torch.allclose(sums[..., 1], yd.square().sum(-1), rtol=1e-4)


def _octant_cloud(r, B, cin, seed):
    """64 points per sample confined to one octant: (counts int32 [B, r^3], the grid a voxelisation leaves -- zero where
    no point is)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    counts = torch.zeros(B, r, r, r, dtype=torch.int32, device="cuda")
    idx = torch.randint(0, r // 2, (B, 64, 3), device="cuda", generator=g)
    for b in range(B):
        counts[b, idx[b, :, 0], idx[b, :, 1], idx[b, :, 2]] = 1
    x = torch.randn(B, cin, r, r, r, device="cuda", generator=g) * (counts > 0).view(B, 1, r, r, r)
    return counts.view(B, -1).contiguous(), x.contiguous()


def _near(counts, r, margin):
    """[B, 1, r, r, r] bool: a point lies within `margin` voxels"""
    occ = (counts.view(-1, 1, r, r, r) > 0).float()
    return F.max_pool3d(occ, 2 * margin + 1, stride=1, padding=margin) > 0


@pytest.mark.parametrize("r,B,cin,cout", [(16, 2, 32, 64), (32, 1, 64, 64)])
def test_half_sparse_forms(r, B, cin, cout):
    """The work queue with occupancy masks (conv1 form) and constant + delta (conv2 form) on a cloud that leaves most tiles
    empty.  Wherever no point is within reach -- every skipped tile, and the untouched voxels of the others -- both kernels
    add an exactly zero accumulator to the same constant: bit-identical to the split kernel (and to the bias in the conv1
    form).  Elsewhere the elementwise bound holds; in the delta form the operand that is rounded is the staged delta
    act - c, so the rounding term is 2^-10 conv64(|W|, |act - c|) (zero padding: the delta is zero outside the grid in
    both).  A second launch on the same occupancy buffer gives the same output: the queue re-arms itself."""
    from lion_amd import conv_ops, fused_ops as fo
    torch.manual_seed(r)
    conv1 = torch.nn.Conv3d(cin, cout, 3, padding=1).cuda()
    conv2 = torch.nn.Conv3d(cout, cout, 3, padding=1).cuda()
    counts, x = _octant_cloud(r, B, cin, seed=r + 1)
    A = torch.rand(B, cout, device="cuda") + 0.5
    Bs = torch.randn(B, cout, device="cuda") * 0.5
    with torch.no_grad():
        occ1, occ2 = fo.conv3d_occupancy(counts, r, cout, B, consumer_aware=0)
        # ---- conv1 form
        s1, _ = fo.conv3d_fused(x, conv1, None, False, occ1, split=True)
        with conv_ops.conv_precision("half"):
            h1, _ = fo.conv3d_fused(x, conv1, None, False, occ1, split=True)
            h1b, _ = fo.conv3d_fused(x, conv1, None, False, occ1, split=True)
        assert torch.equal(h1, h1b)
        far = ~_near(counts, r, 1).expand_as(h1)
        assert far.float().mean().item() > 0.5
        assert torch.equal(h1[far], s1[far])
        assert torch.equal(h1[far], conv1.bias.view(1, -1, 1, 1, 1).expand_as(h1)[far])
        assert not torch.equal(h1, s1)
        inside_elementwise(h1, conv64(x, conv1.weight, conv1.bias), conv64(x.abs(), conv1.weight.abs()), "conv1 form")
        # ---- conv2 form: constant + delta on conv1's (fp32-accurate) output
        s2, _ = fo.conv3d_fused(s1, conv2, (A, Bs), False, occ2, prev_conv=conv1, split=True)
        with conv_ops.conv_precision("half"):
            h2, _ = fo.conv3d_fused(s1, conv2, (A, Bs), False, occ2, prev_conv=conv1, split=True)
            h2b, _ = fo.conv3d_fused(s1, conv2, (A, Bs), False, occ2, prev_conv=conv1, split=True)
        assert torch.equal(h2, h2b)
        far2 = ~_near(counts, r, 2).expand_as(h2)
        assert far2.float().mean().item() > 0.5
        assert torch.equal(h2[far2], s2[far2])
        assert not torch.equal(h2, s2)
        a64, b64 = A.double().cpu().view(B, cout, 1, 1, 1), Bs.double().cpu().view(B, cout, 1, 1, 1)
        act = F.silu(s1.double().cpu() * a64 + b64)
        const = F.silu(conv1.bias.double().cpu().view(1, cout, 1, 1, 1) * a64 + b64)
        inside_elementwise(h2, conv64(act, conv2.weight, conv2.bias), conv64((act - const).abs(), conv2.weight.abs()),
                           "conv2 delta form")


@pytest.mark.parametrize("cin,cout,r,n,kind", [(64, 64, 32, 2048, "flat"), (128, 128, 16, 1024, "clumped")])
def test_half_pvconv_unread_tiles_are_not_written_and_nothing_changes(cin, cout, r, n, kind):
    """the consumer-aware levels in half mode: the fused voxel branch's output is bit-identical whatever the unwritten tiles
    held (0, NaN, 1e30), and agrees with the evaluation that writes every voxel to fp32 rounding (only the closed-form
    GroupNorm sums of skipped tiles differ); both convolutions really ran on the half entry point"""
    from conftest import fill_
    from lion_amd import _lib, conv_ops
    from lion_amd.config import released_prior_cfg
    from lion_amd.models import pvcnn2_ada as m
    torch.manual_seed(r + cin)
    pv = m.PVConv(cin, cout, 3, r, with_se=True, attention=False, dropout=0.1, cfg=released_prior_cfg())
    fill_(pv)
    pv.cuda().eval()
    B = 3
    feat = torch.randn(B, cin, n, device="cuda")
    coords = torch.randn(B, 3, n, device="cuda")
    if kind == "flat":
        coords = coords * torch.tensor([1.0, 0.15, 0.6], device="cuda").view(1, 3, 1)
    else:
        coords[:, :, : int(0.95 * n)] *= 0.1
    sty = torch.randn(B, 128, device="cuda")

    def poison(val):
        blocks = [torch.full((B, cout, r, r, r), val, device="cuda") for _ in range(3)]
        blocks += [torch.full((B, cin, r, r, r), val, device="cuda") for _ in range(2)]
        del blocks

    names = []
    real_call = _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real_call(name, *a, **k)

    saved = m.SKIP_UNREAD
    _lib.call = spy
    try:
        with torch.no_grad(), m.voxel_plans(), conv_ops.conv_precision("half"):
            m.SKIP_UNREAD = False
            poison(float("nan"))
            ref = pv((feat, coords, None, sty))[0].clone()
            m.SKIP_UNREAD = True
            outs = []
            for val in (0.0, float("nan"), 1e30):
                poison(val)
                outs.append(pv((feat, coords, None, sty))[0].clone())
    finally:
        m.SKIP_UNREAD = saved
        _lib.call = real_call
    assert names.count("lion_conv3d_k3_half_forward") == 8 and "lion_conv3d_k3_split_forward" not in names
    assert torch.isfinite(ref).all() and all(bool(torch.isfinite(o).all()) for o in outs)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert (outs[1] - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()


@pytest.mark.parametrize("r,cin,cout", [(8, 32, 32), (16, 24, 32), (16, 32, 48)])
def test_half_unsupported_shapes_are_einval_and_write_nothing(r, cin, cout):
    from lion_amd import _lib
    x = torch.randn(1, cin, r, r, r, device="cuda")
    wp = torch.zeros(4 * 27 * 4 * 64 * 8 + 8, dtype=torch.int16, device="cuda")   # larger than any pack of these shapes
    y = torch.full((1, cout, r, r, r), 123.0, device="cuda")
    with pytest.raises(RuntimeError, match="LION_EINVAL"):
        _lib.call("lion_conv3d_k3_half_forward", x, wp, None, 1, cin, cout, r, None, None, None, None, y, None, None)
    torch.cuda.synchronize()
    assert bool((y == 123.0).all())
