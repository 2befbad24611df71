"""-m gpu: the small serial launches of a PVConv after their dependent round trips were taken out, each against the plain
kernel it replaces, bit for bit on int32 views (a NaN and the sign of a zero count):
  * lion_groupnorm_fold_se == lion_internal_groupnorm_fold_se_plain;
  * lion_pwconv_forward / lion_pwconv_grouped_forward at L <= 4096 == lion_internal_pwconv_small_plain.
Only where and when a value is requested differs between the twins: any difference at all is a bug."""
import itertools
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return torch.equal(bits(a), bits(b))


def gen_for(*key):
    return torch.Generator(device="cuda").manual_seed(zlib.crc32(repr(key).encode()))


def tile_sums(B, C, T, scale, gen):
    """[B,C,T,2] sums of 64-voxel tiles of a field with mean = std = scale (0: all zero -> the var > 0 clamp and var = 0)"""
    x = torch.randn(B, C, T, 64, device="cuda", generator=gen) * scale + scale
    return torch.stack([x.sum(-1), (x * x).sum(-1)], dim=-1).contiguous()


# ---------------------------------------------------------------- fold + SE gate

def se_inputs(B, C, H, T, G, gen):
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    fg = rn(B, 2 * C)
    return dict(stats=tile_sums(B, C, T, 3.0, gen), gam=rn(C), bet=rn(C), fac=fg[:, :C], gb=fg[:, C:], w1=rn(H, C), w2=rn(C, H))


def se_both(i, B, C, H, T, G):
    from lion_amd import _lib
    outs = []
    for name in ("lion_groupnorm_fold_se", "lion_internal_groupnorm_fold_se_plain"):
        A, Bs = torch.full((B, C), NAN, device="cuda"), torch.full((B, C), NAN, device="cuda")
        _lib.call(name, i["stats"], B, C, T, G, T * 64, i["gam"], i["bet"], i["fac"], i["gb"], 2 * C, 1e-5, i["w1"], i["w2"], H,
                  A, Bs)
        outs.append((A, Bs))
    return outs


@pytest.mark.parametrize("C", [4, 60, 64, 256])
def test_fold_se_equals_its_plain_twin(C):
    """H = 4, 8, 16, 32 (the SE layers of the model) run the one-round-trip kernel, every other H the plain kernel on both
    sides; T = 128 is more than one batch of eight tile-sum requests per lane at every C"""
    for H, T, B in itertools.product((1, 4, 7, 8, 16, 32, 128), (1, 5, 128), (1, 3)):
        i = se_inputs(B, C, H, T, 4, gen_for("fold_se", C, H, T, B))
        (A1, B1), (A0, B0) = se_both(i, B, C, H, T, 4)
        assert same(A0, A1) and same(B0, B1), (C, H, T, B)
        assert bool(torch.isfinite(A1).all() and torch.isfinite(B1).all()), (C, H, T, B)


def test_fold_se_with_an_unaligned_w2_takes_the_plain_kernel():
    """w2 rows that cannot be read 16 bytes at a time: same bits through the entry point's fall-back"""
    B, C, H, T, G = 2, 64, 8, 5, 8
    i = se_inputs(B, C, H, T, G, gen_for("fold_se_unaligned"))
    aligned = se_both(i, B, C, H, T, G)[0]
    buf = torch.zeros(C * H + 1, device="cuda")
    buf[1:] = i["w2"].reshape(-1)
    i["w2"] = buf[1:].view(C, H)
    assert i["w2"].data_ptr() % 16 == 4
    (A1, B1), (A0, B0) = se_both(i, B, C, H, T, G)
    assert same(A0, A1) and same(B0, B1) and same(A1, aligned[0]) and same(B1, aligned[1])


def test_fold_se_nan_stays_in_its_sample():
    B, C, H, T, G = 3, 64, 8, 5, 8
    i = se_inputs(B, C, H, T, G, gen_for("fold_se_nan"))
    clean = se_both(i, B, C, H, T, G)[0]
    i["stats"][1, 17, 3, 0] = NAN
    (A1, B1), (A0, B0) = se_both(i, B, C, H, T, G)
    assert same(A0, A1) and same(B0, B1)
    # the NaN reaches the sample's own scalars (Bs through the group mean; the var > 0 clamp and the ReLU swallow it elsewhere)
    assert bool(torch.isnan(A1[1]).any() or torch.isnan(B1[1]).any())
    for b in (0, 2):
        assert same(A1[b], clean[0][b]) and same(B1[b], clean[1][b])


# ---------------------------------------------------------------- short-activation 1x1 convolution

GUARD = 4096   # floats of NaN behind y and behind the sums: nothing beyond column L or row Cout is ever written


def pw_pair(B, Cin, Cout, L, pro, stats, gen, gather=None):
    """(y buffer, sums buffer) of the public entry and of the plain twin; the buffers carry a NaN guard"""
    from lion_amd import _lib
    lib = _lib.load()
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    wp = torch.zeros(lib.lion_pwconv_packed_floats(Cout, Cin), device="cuda")
    _lib.call("lion_pwconv_pack_weights", rn(Cout, Cin), Cout, Cin, wp)
    bias = rn(Cout)
    pa, pb = (rn(B, Cin) * 0.5 + 1.0, rn(B, Cin) * 0.3) if pro else (None, None)
    tiles = lib.lion_pwconv_stat_tiles(Cout, Cin, L)
    assert tiles == (L + 31) // 32
    if gather is None:
        x = rn(B, Cin, L)
    else:
        C, N, U, M = gather
        coords, centers, feat = rn(B, 3, N), rn(B, 3, M), rn(B, C, N)
        idx = torch.randint(-2, N + 2, (B, M, U), device="cuda", generator=gen, dtype=torch.int32)   # clamped by the kernel
    out = []
    for plain in (False, True):
        y = torch.full((B * Cout * L + GUARD,), NAN, device="cuda")
        st = torch.full((B * Cout * tiles * 2 + GUARD,), NAN, device="cuda")
        s = st if stats else None
        if plain and gather is None:
            _lib.call("lion_internal_pwconv_small_plain", x, wp, bias, B, Cin, Cout, L, pa, pb, None, None, None, None, 0, 0, y, s)
        elif plain:
            _lib.call("lion_internal_pwconv_small_plain", None, wp, bias, B, Cin, Cout, L, None, None, coords, centers, feat, idx,
                      N, U, y, s)
        elif gather is None:
            _lib.call("lion_pwconv_forward", x, wp, bias, B, Cin, Cout, L, pa, pb, y, s)
        else:
            _lib.call("lion_pwconv_grouped_forward", coords, centers, feat, idx, wp, bias, B, C, N, M, U, Cout, y, s)
        out.append((y, st))
    return out


def check_pw(pair, B, Cout, L, stats, where):
    (y1, s1), (y0, s0) = pair
    tiles = (L + 31) // 32
    assert same(y0, y1), (where, "y")
    assert same(s0, s1), (where, "sums")
    assert bool(torch.isfinite(y1[:B * Cout * L]).all()) and bool(torch.isnan(y1[B * Cout * L:]).all()), where
    n = B * Cout * tiles * 2
    assert bool(torch.isfinite(s1[:n]).all()) if stats else bool(torch.isnan(s1[:n]).all()), where
    assert bool(torch.isnan(s1[n:]).all()), where


@pytest.mark.parametrize("Cin", [3, 64, 255, 256, 258, 515, 1024])
def test_pwconv_small_equals_its_plain_twin(Cin):
    """one round (Cin <= 256: 3, 64), a clamped tail (255), the multi-round kernel at two rounds per wave (258, 515) and
    at four with a short last one (1024: 128 k-steps per wave in rounds of 16 against the plain kernel's 32)"""
    for Cout, L, B in itertools.product((32, 64, 100, 128), (1, 31, 32, 33, 64), (1, 2)):
        for pro, stats in itertools.product((False, True), (False, True)):
            pair = pw_pair(B, Cin, Cout, L, pro, stats, gen_for("pw", Cin, Cout, L, B, pro, stats))
            check_pw(pair, B, Cout, L, stats, (Cin, Cout, L, B, pro, stats))


def test_pwconv_small_gathered_equals_its_plain_twin():
    C, N, U, M = 3, 40, 8, 4
    for Cout, B, stats in itertools.product((32, 64, 100, 128), (1, 2), (False, True)):
        pair = pw_pair(B, 3 + C, Cout, M * U, False, stats, gen_for("pwg", Cout, B, stats), gather=(C, N, U, M))
        check_pw(pair, B, Cout, M * U, stats, ("gathered", Cout, B, stats))
