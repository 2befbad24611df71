"""-m gpu: the 16-byte transport of the split-operand 1x1 convolution (csrc/pwconv_split.hip, WIDE: activation rows by
16-byte LDS-DMA, results by 16-byte stores) against the 4-byte path it falls back to -- bit for bit -- at the smallest
shapes where it can go wrong: one chunk / a ragged last chunk / a ring wrap-around (Cin 16 / 35 / 131), every plan, padded
channel rows and two channel tiles (Cout 32 .. 256), less than a column block / one tile / a tile + 4 columns / ragged
(L 4 / 128 / 132 / 260).  The launcher takes the wide path iff L % 4 == 0 and x, y are 16-byte aligned."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 1e-5          # tests/test_pwconv_split_gpu.py
B = 2
CINS, COUTS, LS = (16, 35, 131), (32, 64, 96, 128, 256), (4, 128, 132, 260)
SHAPES = [(ci, co) for ci in CINS for co in COUTS]


def _tile_width(cout):
    """columns per statistics tile = per workgroup (pws_plan: 128 x VB)"""
    return 128 if ((cout + 31) // 32) % 4 == 0 else 256


def _params(cin, cout, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(cout, cin, 1, device="cuda", generator=g) * cin ** -0.5
    bias = torch.randn(cout, device="cuda", generator=g)
    A = torch.randn(B, cin, device="cuda", generator=g) * 0.5 + 1.0
    Bs = torch.randn(B, cin, device="cuda", generator=g) * 0.3
    return w, bias, A, Bs


def _x(cin, L, seed):
    g = torch.Generator(device="cuda").manual_seed(1000 + seed)
    return torch.randn(B, cin, L, device="cuda", generator=g)


def _run(x, w, bias, pro, want_stats, y=None, stats=None):
    """lion_pwconv_split_forward on the views given (no .contiguous(), no reallocation: alignment is the caller's)"""
    from lion_amd import _lib
    from lion_amd import fused_ops as fo
    cout, cin = w.shape[:2]
    L = x.shape[2]
    assert x.is_contiguous() and x.shape[1] == cin
    wp = fo._pw_split_pack(w)
    if y is None:
        y = torch.empty(x.shape[0], cout, L, device="cuda")
    tiles = _lib.load().lion_pwconv_split_stat_tiles(cout, cin, L)
    if want_stats and stats is None:
        stats = torch.empty(x.shape[0], cout, tiles, 2, device="cuda")
    pa, pb = pro if pro is not None else (None, None)
    _lib.call("lion_pwconv_split_forward", x, wp, bias, x.shape[0], cin, cout, L, pa, pb, y, stats if want_stats else None)
    return y, (stats if want_stats else None)


def _embedded(x):
    """the same columns inside a tensor one column longer: L + 1 is odd, the launcher must take the 4-byte path"""
    x2 = torch.full((x.shape[0], x.shape[1], x.shape[2] + 1), 3.25, device="cuda")
    x2[..., :-1] = x
    return x2


def _ref64(x, w, bias, pro):
    xin = x.double()
    if pro is not None:
        t = xin * pro[0].double()[:, :, None] + pro[1].double()[:, :, None]
        xin = t * torch.sigmoid(t)
    return torch.einsum("oc,bcl->bol", w.double()[:, :, 0], xin) + bias.double()[None, :, None]


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_wide_path_equals_the_4_byte_path(cin, cout):
    w, bias, A, Bs = _params(cin, cout, cin * 1000 + cout)
    tw = _tile_width(cout)
    for L in LS:
        x = _x(cin, L, L)
        x2 = _embedded(x)
        for pro in (None, (A, Bs)):
            for st in (True, False):
                y, s = _run(x, w, bias, pro, st)
                y2, s2 = _run(x2, w, bias, pro, st)
                assert torch.equal(y, y2[..., :L]), (L, pro is not None, st)
                if st:
                    full = L // tw      # tiles full in both runs
                    assert s.shape[2] == (L + tw - 1) // tw
                    assert torch.equal(s[:, :, :full], s2[:, :, :full]), (L, pro is not None)


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_column_permutation_commutes_bit_for_bit(cin, cout):
    w, bias, A, Bs = _params(cin, cout, cin * 1000 + cout + 1)
    g = torch.Generator(device="cuda").manual_seed(7)
    for L in LS:
        x = _x(cin, L, L + 1)
        perm = torch.randperm(L, device="cuda", generator=g)
        xp = x[..., perm].contiguous()
        for pro in (None, (A, Bs)):
            for st in (True, False):
                y, _ = _run(x, w, bias, pro, st)
                yp, _ = _run(xp, w, bias, pro, st)
                assert torch.equal(yp, y[..., perm]), (L, pro is not None, st)


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_wide_path_within_the_bounds_of_the_split_kernel(cin, cout):
    """max error < 1e-5 of the output's maximum against float64; the sums within the tolerances of test_pwconv_split_gpu.py"""
    w, bias, A, Bs = _params(cin, cout, cin * 1000 + cout + 2)
    for L in LS:
        x = _x(cin, L, L + 2)
        for pro in (None, (A, Bs)):
            ref = _ref64(x, w, bias, pro)
            y, s = _run(x, w, bias, pro, True)
            y0, _ = _run(x, w, bias, pro, False)
            assert torch.equal(y, y0)
            scale = ref.abs().max().item()
            e = (y.double() - ref).abs().max().item() / scale
            assert e < BOUND, (L, pro is not None, e)
            sums = s.double().sum(2)
            assert torch.allclose(sums[..., 0], ref.sum(-1), rtol=1e-4, atol=1e-4 * scale * max(L, 1) ** 0.5)
            assert torch.allclose(sums[..., 1], ref.square().sum(-1), rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("cin,cout", [(35, 96), (131, 128), (16, 64)])
def test_fallback_is_taken_and_correct(cin, cout):
    """L = 131 (no 16-byte pieces) and an x that starts one float into its buffer run the 4-byte path; both equal the
    aligned computation of the same data."""
    w, bias, A, Bs = _params(cin, cout, cin + cout)
    tw = _tile_width(cout)
    for pro in (None, (A, Bs)):
        # L = 131: against float64, and against the wide run of the same columns followed by one more
        x = _x(cin, 131, 5)
        y, s = _run(x, w, bias, pro, True)
        ref = _ref64(x, w, bias, pro)
        assert (y.double() - ref).abs().max().item() / ref.abs().max().item() < BOUND
        x132 = _embedded(x)
        assert x132.shape[2] % 4 == 0 and x132.data_ptr() % 16 == 0
        yw, sw = _run(x132, w, bias, pro, True)
        assert torch.equal(y, yw[..., :131])
        assert torch.equal(s[:, :, :131 // tw], sw[:, :, :131 // tw])
        # L = 132, storage one float into the buffer
        xa = _x(cin, 132, 6)
        buf = torch.empty(xa.numel() + 1, device="cuda")
        xm = buf[1:].view_as(xa)
        xm.copy_(xa)
        assert xa.data_ptr() % 16 == 0 and xm.data_ptr() % 16 == 4
        ya, sa = _run(xa, w, bias, pro, True)
        ym, sm = _run(xm, w, bias, pro, True)
        assert torch.equal(ya, ym) and torch.equal(sa, sm)
        # ... and a y one float into its buffer
        ybuf = torch.empty(ya.numel() + 1, device="cuda")
        yv = ybuf[1:].view_as(ya)
        _run(xa, w, bias, pro, False, y=yv)
        assert torch.equal(ya, yv)


@pytest.mark.parametrize("cin,cout", [(35, 96), (131, 256), (16, 32), (35, 128)])
@pytest.mark.parametrize("L", [132, 4])
def test_guard_bands_stay_intact(cin, cout, L):
    """y and stats in the middle of larger buffers: nothing outside the views is written; memory behind x's last row (same
    allocation) is not part of the result."""
    from lion_amd import _lib
    w, bias, A, Bs = _params(cin, cout, cin + cout + L)
    tiles = _lib.load().lion_pwconv_split_stat_tiles(cout, cin, L)
    pad, sentinel = 1024, -12345.5
    n, ny, ns = B * cin * L, B * cout * L, B * cout * tiles * 2
    for pro in (None, (A, Bs)):
        for tail in (0.0, float("nan")):
            xbig = torch.full((n + 4096,), tail, device="cuda")
            x = xbig[:n].view(B, cin, L)
            x.copy_(_x(cin, L, 9))
            ybig = torch.full((ny + 2 * pad,), sentinel, device="cuda")
            sbig = torch.full((ns + 2 * pad,), sentinel, device="cuda")
            y = ybig[pad:pad + ny].view(B, cout, L)
            s = sbig[pad:pad + ns].view(B, cout, tiles, 2)
            assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
            _run(x, w, bias, pro, True, y=y, stats=s)
            torch.cuda.synchronize()
            for big, m in ((ybig, ny), (sbig, ns)):
                assert (big[:pad] == sentinel).all() and (big[pad + m:] == sentinel).all()
            assert torch.isfinite(y).all() and torch.isfinite(s).all()
            if tail == 0.0:
                y0, s0 = y.clone(), s.clone()
            else:
                assert torch.equal(y, y0) and torch.equal(s, s0)


def test_graph_replay_equals_eager(monkeypatch):
    """one SharedMLP forward over a 2-D activation [2, 35, 9, 32] (L = 288: wide, two tiles and a ragged third) with every
    layer on the split kernel: captured, replayed twice, bit-identical to eager."""
    from lion_amd import fused_ops as fo
    from lion_amd.config import released_prior_cfg
    from lion_amd.models import pvcnn2_ada as m
    from conftest import fill_
    monkeypatch.setattr(fo, "pw_use_split", lambda split, b, cin, cout, L: True)
    cfg = released_prior_cfg()
    torch.manual_seed(6)
    mlp = m.SharedMLP(35, [64, 128], dim=2, cfg=cfg)
    fill_(mlp)
    mlp.cuda().eval()
    x = torch.randn(2, 35, 9, 32, device="cuda")
    sty = torch.randn(2, cfg.latent_pts.style_dim, device="cuda")
    with torch.no_grad():
        eager = mlp(x, sty).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                mlp(x, sty)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = mlp(x, sty)
        for _ in range(2):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
    assert torch.isfinite(eager).all() and tuple(eager.shape) == (2, 128, 9, 32)
