"""-m gpu: the gathered-operand form of the 1x1 convolutions (lion_pwconv_grouped_forward, lion_pwconv_split_grouped_forward:
the first layer of a set-abstraction MLP reading coords / centers / feat through the ball-query indices instead of the
[B, 3 + C, M, U] tensor of lion_group_points_forward).

1. Bit identity with group_points -> the ungrouped entry point, y and every tile of the sums, through _lib.call (no policy
   in between), at the kernels' edges: the fp32 large kernel with a partial last workgroup (L = 4160), Cin 3 / 35 / 131 (one
   k group, odd, several groups), Cout 32 .. 128 with padded channel rows (48), N = 97 (no multiple of 4), both weight paths
   (L2 and, at B = 32, LDS); the fp32 small kernel at L = 160 and L = 48 (a partial 32-column tile); the split kernel at
   L = 2080 (the ungrouped call takes the 16-byte path) and L = 63 (it takes the 4-byte path), every plan.  Index patterns:
   uniform, ball-query style (first neighbour repeated), all 0, all N - 1.
2. The same cases, every index pattern and every sample, against a float64 GEMM of the operand gathered by torch indexing
   (the operand is DEFINED with one fp32 subtraction; group_points' tensor must equal it), held to the bounds of
   tests/pwconv_ref.py (fp32 kernels) and to those of tests/test_pwconv_split_gpu.py (split kernel).
3. A NaN in feat[b, c, j] or coords[b, :, j] reaches exactly the columns with idx == j of sample b.
4. PointNetSAModule on the four stage configurations (scaled down) and one PVCNN2Prior forward: SA_GATHER on == off, bit for
   bit, and with the flag on fused_ops.group_points is not called."""
import pytest
import torch

import pwconv_ref as R

pytestmark = pytest.mark.gpu

SPLIT_BOUND = 1e-5          # tests/test_pwconv_split_gpu.py
PATTERNS = ("uniform", "ballquery", "zeros", "last")


def _cloud(B, C, N, M, U, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    co = torch.randn(B, 3, N, device="cuda", generator=g)
    ctr = torch.randn(B, 3, M, device="cuda", generator=g)
    feat = torch.randn(B, C, N, device="cuda", generator=g) if C else None
    return co, ctr, feat


def _indices(pattern, B, N, M, U, seed):
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    if pattern == "uniform":
        idx = torch.randint(0, N, (B, M, U), device="cuda", generator=g)
    elif pattern == "ballquery":   # k found neighbours in ascending order, the first one repeated to fill the list
        idx = torch.randint(0, N, (B, M, U), device="cuda", generator=g).sort(-1).values
        k = torch.randint(1, U + 1, (B, M, 1), device="cuda", generator=g)
        idx = torch.where(torch.arange(U, device="cuda")[None, None, :] < k, idx, idx[..., :1])
    elif pattern == "zeros":
        idx = torch.zeros(B, M, U, device="cuda", dtype=torch.int64)
    else:
        idx = torch.full((B, M, U), N - 1, device="cuda", dtype=torch.int64)
    return idx.int().contiguous()


def _weights(cin, cout, seed):
    g = torch.Generator(device="cuda").manual_seed(200 + seed)
    w = torch.randn(cout, cin, 1, device="cuda", generator=g) * cin ** -0.5
    return w, torch.randn(cout, device="cuda", generator=g)


def _run(split, co, ctr, feat, idx, w, bias, want_stats=True, grouped=True):
    """(y [B, Cout, L], stats | None, x): the new entry point, or group_points -> the ungrouped one"""
    from lion_amd import _lib
    from lion_amd import fused_ops as fo
    lib = _lib.load()
    B, _, N = co.shape
    M, U = idx.shape[1:]
    C = 0 if feat is None else feat.shape[1]
    cin, cout, L = 3 + C, w.shape[0], M * U
    wp = (fo._pw_split_pack if split else fo._pw_pack)(w)
    tiles = (lib.lion_pwconv_split_stat_tiles if split else lib.lion_pwconv_stat_tiles)(cout, cin, L)
    assert tiles > 0
    y = torch.full((B, cout, L), float("nan"), device="cuda")
    stats = torch.full((B, cout, tiles, 2), float("nan"), device="cuda") if want_stats else None
    if grouped:
        _lib.call("lion_pwconv_split_grouped_forward" if split else "lion_pwconv_grouped_forward",
                  co, ctr, feat, idx, wp, bias, B, C, N, M, U, cout, y, stats)
        return y, stats, None
    x = fo.group_points(co, ctr, feat, idx).view(B, cin, L)
    _lib.call("lion_pwconv_split_forward" if split else "lion_pwconv_forward", x, wp, bias, B, cin, cout, L, None, None, y, stats)
    return y, stats, x


def _operand(co, ctr, feat, idx):
    """f32[B, 3 + C, M U]: the operand as the entry points define it, by torch indexing (nothing of the library):
    coords[b, k, idx] - centers[b, k, m] in ONE fp32 subtraction for k < 3, feat[b, k - 3, idx] beyond"""
    B, M, U = idx.shape
    ix = idx.long().view(B, 1, M * U)
    parts = [co.gather(2, ix.expand(B, 3, -1)) - ctr.repeat_interleave(U, dim=2)]
    if feat is not None:
        parts.append(feat.gather(2, ix.expand(B, feat.shape[1], -1)))
    return torch.cat(parts, 1)


def _same(split, co, ctr, feat, idx, w, bias, note):
    """bit identity of the new entry point with group_points -> the ungrouped one; returns y, the sums and the operand of
    _operand (which group_points' tensor equals) for the float64 side"""
    y, s, _ = _run(split, co, ctr, feat, idx, w, bias)
    y0, s0, x = _run(split, co, ctr, feat, idx, w, bias, grouped=False)
    assert torch.equal(y, y0), note
    assert torch.equal(s, s0), note
    yn, _, _ = _run(split, co, ctr, feat, idx, w, bias, want_stats=False)
    assert torch.equal(yn, y0), note
    xo = _operand(co, ctr, feat, idx)
    assert torch.equal(x, xo), note
    return y, s, xo


def _fp32_float64(y, s, x, w, bias, cols, note):
    ref, bound = R.pwconv64(x, w[:, :, 0], bias)
    assert ((y.double() - ref).abs() <= bound).all(), note
    sums, sb = R.tile_stats64(ref, bound, cols)
    assert ((s.double() - sums).abs() <= sb).all(), note


def _split_float64(y, s, x, w, bias, note):
    ref = torch.einsum("oc,bcl->bol", w.double()[:, :, 0], x.double()) + bias.double()[None, :, None]
    scale = ref.abs().max().item()
    L = ref.shape[2]
    assert (y.double() - ref).abs().max().item() / scale < SPLIT_BOUND, note
    sums = s.double().sum(2)
    assert torch.allclose(sums[..., 0], ref.sum(-1), rtol=1e-4, atol=1e-4 * scale * max(L, 1) ** 0.5), note
    assert torch.allclose(sums[..., 1], ref.square().sum(-1), rtol=1e-4, atol=1e-6), note


# ---- 1 + 2: fp32 large kernel --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout", [32, 48, 64, 128])
@pytest.mark.parametrize("C", [0, 32, 128])
def test_fp32_large_kernel(C, cout):
    B, N, M, U = 2, 97, 130, 32
    cin, L = 3 + C, M * U
    kind, cols = R.path(cin, cout, L, B)
    assert kind[0] == "large" and kind[2] is False and L % (4 * 128) != 0    # weights from L2, a partial last workgroup
    co, ctr, feat = _cloud(B, C, N, M, U, C + cout)
    w, bias = _weights(cin, cout, C + cout)
    for p in PATTERNS:
        idx = _indices(p, B, N, M, U, cout)
        y, s, x = _same(False, co, ctr, feat, idx, w, bias, (p, C, cout))
        _fp32_float64(y, s, x, w, bias, cols, (p, C, cout))


def test_fp32_large_kernel_weights_through_lds():
    B, N, M, U, C, cout = 32, 97, 1024, 32, 1, 32
    kind, cols = R.path(3 + C, cout, M * U, B)
    assert kind == ("large", 1, True)
    co, ctr, feat = _cloud(B, C, N, M, U, 5)
    w, bias = _weights(3 + C, cout, 5)
    for p in ("ballquery", "last"):
        idx = _indices(p, B, N, M, U, 5)
        y, s, x = _same(False, co, ctr, feat, idx, w, bias, p)
        _fp32_float64(y, s, x, w, bias, cols, p)


# ---- fp32 small kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,U", [(5, 32), (3, 16)])
@pytest.mark.parametrize("C", [0, 61, 320])
def test_fp32_small_kernel(C, M, U):
    B, N = 3, 97
    cin, L = 3 + C, M * U
    for cout in (48, 128):
        assert R.path(cin, cout, L, B)[0] == ("small",)
        co, ctr, feat = _cloud(B, C, N, M, U, C + M)
        w, bias = _weights(cin, cout, C + M + cout)
        for p in PATTERNS:
            idx = _indices(p, B, N, M, U, M)
            y, s, x = _same(False, co, ctr, feat, idx, w, bias, (p, C, cout))
            _fp32_float64(y, s, x, w, bias, 32, (p, C, cout))


# ---- split kernel --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout", [32, 64, 128])
@pytest.mark.parametrize("C", [13, 128, 192])
@pytest.mark.parametrize("M,U", [(65, 32), (7, 9)])
def test_split_kernel(M, U, C, cout):
    B, N = 2, 97
    cin, L = 3 + C, M * U
    assert (L % 4 == 0) == (U == 32)     # the ungrouped reference runs the 16-byte path at L = 2080, the 4-byte path at L = 63
    co, ctr, feat = _cloud(B, C, N, M, U, C + cout + M)
    w, bias = _weights(cin, cout, C + cout + M)
    for p in PATTERNS:
        idx = _indices(p, B, N, M, U, cout + M)
        y, s, x = _same(True, co, ctr, feat, idx, w, bias, (p, C, cout))
        _split_float64(y, s, x, w, bias, (p, C, cout))


# ---- 3: a NaN stays in the columns that gather it ------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["large", "small", "split"])
def test_nan_reaches_only_the_columns_that_gather_it(family):
    B, N, C, cout = 2, 97, 32, 64
    M, U = {"large": (130, 32), "small": (5, 32), "split": (65, 32)}[family]
    split = family == "split"
    L, cin = M * U, 3 + C
    if not split:
        assert R.path(cin, cout, L, B)[0][0] == family
    cols = 256 if split else R.path(cin, cout, L, B)[1]     # columns per tile of the sums (split, Cout = 64: 128 x VB = 2)
    co, ctr, feat = _cloud(B, C, N, M, U, 11)
    w, bias = _weights(cin, cout, 11)
    g = torch.Generator(device="cuda").manual_seed(12)
    idx = torch.randint(0, N - 1, (B, M, U), device="cuda", generator=g).int()     # nobody gathers point N - 1 ...
    hit = torch.zeros(B, L, dtype=torch.bool, device="cuda")
    hit[1, [0, 3, 31, 32, min(L - 1, cols + 5)]] = True                              # ... but these columns of sample 1
    idx.view(B, L)[hit] = N - 1
    y0, s0, _ = _run(split, co, ctr, feat, idx, w, bias)
    assert torch.isfinite(y0).all() and torch.isfinite(s0).all()
    tile_hit = torch.nn.functional.pad(hit, (0, s0.shape[2] * cols - L)).view(B, -1, cols).any(-1)   # [B, T]
    for what in ("feat", "coords"):
        co2, feat2 = co.clone(), feat.clone()
        if what == "feat":
            feat2[1, 7, N - 1] = float("nan")
        else:
            co2[1, :, N - 1] = float("nan")
        feat2[0, 7, N - 1] = float("nan")      # sample 0 does not gather the point at all
        y, s, _ = _run(split, co2, ctr, feat2, idx, w, bias)
        assert torch.isnan(y.transpose(1, 2)[hit]).all(), (family, what)
        keep = ~hit[:, None, :].expand_as(y)
        assert torch.equal(y[keep], y0[keep]), (family, what)
        tkeep = ~tile_hit[:, None, :, None].expand_as(s)
        assert torch.isnan(s[~tkeep]).all() and torch.equal(s[tkeep], s0[tkeep]), (family, what)


# ---- 4: module level -----------------------------------------------------------------------------------------------------

@pytest.fixture()
def count_group_points(monkeypatch):
    from lion_amd import fused_ops as fo
    calls = []
    real = fo.group_points

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(fo, "group_points", counted)
    return calls


# (feature channels, centres at N = 256, radius, neighbours, MLP): the four set-abstraction stages of the released denoiser
# as PVCNN2Prior builds them from its own table, models/latent_points_ada_localprior.py::sa_blocks (first layers 35 -> 32,
# 67 -> 64, 131 -> 128, 195 -> 128: the 64 time-embedding channels ride in the features from stage 1 on; the VAE's
# latent_points_ada.py::_VAE_SA_BLOCKS is wider at SA-2 and would give 323 at SA-3), M / N as there
STAGES = [(32, 128, 0.1, 32, (32, 64)), (64, 64, 0.2, 32, (64, 128)), (128, 64, 0.4, 32, (128, 128)),
          (192, 64, 0.8, 32, (128, 128, 128))]


@pytest.mark.parametrize("stage", range(4))
def test_sa_module_gather_equals_materialised(stage, monkeypatch, count_group_points):
    from conftest import fill_
    from lion_amd.config import released_prior_cfg
    from lion_amd.models import pvcnn2_ada as m
    C, M, radius, U, mlp = STAGES[stage]
    cfg = released_prior_cfg()
    sa = m.PointNetSAModule(M, radius, U, C, list(mlp), cfg=cfg)
    fill_(sa)
    sa.cuda().eval()
    B, N = 2, 256
    g = torch.Generator(device="cuda").manual_seed(stage)
    coords = torch.randn(B, 3, N, device="cuda", generator=g) * 0.5
    feats = torch.randn(B, C, N, device="cuda", generator=g)
    style = torch.randn(B, cfg.latent_pts.style_dim, device="cuda", generator=g)
    outs = {}
    with torch.no_grad():
        for on in (False, True):
            monkeypatch.setattr(m, "SA_GATHER", on)
            del count_group_points[:]
            outs[on] = sa((feats, coords, None, style))[0].clone()
            assert len(count_group_points) == (0 if on else 1), (stage, on)
    assert tuple(outs[True].shape) == (B, mlp[-1], M) and torch.isfinite(outs[True]).all()
    assert torch.equal(outs[True], outs[False])
    # a consumer outside the own-kernel inference path still gets the tensor
    monkeypatch.setattr(m, "SA_GATHER", True)
    del count_group_points[:]
    with torch.no_grad():
        sa.train()
        out = sa((feats, coords, None, style))[0]
    assert len(count_group_points) == 1 and tuple(out.shape) == (B, mlp[-1], M)


def test_prior_forward_gather_equals_materialised(monkeypatch, count_group_points):
    from conftest import fill_
    from lion_amd import chain
    from lion_amd.config import released_prior_cfg
    from lion_amd.models import pvcnn2_ada as m
    from lion_amd.models.latent_points_ada_localprior import PVCNN2Prior
    cfg = released_prior_cfg()
    loc = PVCNN2Prior(cfg.sde, 1, cfg)
    fill_(loc)
    loc.cuda().eval()
    B = 2
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, loc.num_points * loc.num_classes, 1, 1, device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g)
    cond = torch.randn(B, 128, 1, 1, device="cuda", generator=g)
    outs, keys = {}, {}
    with torch.no_grad():
        for on in (False, True):
            monkeypatch.setattr(m, "SA_GATHER", on)
            keys[on] = chain.policy_key()
            del count_group_points[:]
            outs[on] = loc(x, t, condition_input=cond).clone()
            assert len(count_group_points) == (0 if on else 4), on
    assert keys[True] != keys[False]          # a captured chain is re-captured when the flag flips
    assert torch.isfinite(outs[True]).all() and torch.equal(outs[True], outs[False])
