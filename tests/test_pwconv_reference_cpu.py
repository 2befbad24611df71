"""CPU: the float64 references and bounds of tests/pwconv_ref.py.  The shape table against what the library reports (pure
host calls), the references against plain torch, and the bounds against an fp32 numpy emulation of the kernels' own
arithmetic (csrc/pwconv.hip) on every data kind -- so they are known to be satisfiable before any GPU run -- and against
the mistakes they are there to catch."""
import math

import numpy as np
import pytest
import torch

import pointwise_ref as pr
import pwconv_ref as pw


def ratio(got, ref, bound):
    err = (torch.as_tensor(np.asarray(got)).double() - ref).abs()
    assert bool((bound > 0).all())
    return float((err / bound).max())


def test_shape_table_reaches_every_path_of_the_kernels():
    from lion_amd import _lib
    pw.check_table(_lib.load())
    keys = list(pw.TABLE)
    small = {k[2] for k in keys if k[2] <= pw.SMALL_L}
    assert {1, 31, 32, 33, 4095, 4096} <= small and 4097 in {k[2] for k in keys}
    assert {1, 2, 3, 5} <= {k[0] for k in keys} and any(k[0] > 128 and k[2] > 4096 for k in keys)
    assert {1, 31, 33, 96, 160, 320, 32, 64, 128, 256} <= {k[1] for k in keys}
    # plans decided by what fits LDS, at a length the large kernel runs
    assert pw.TABLE[(259, 128, 4100, 2)][1] == 4 and pw.TABLE[(300, 128, 4500, 2)][1] == 2 and pw.TABLE[(320, 256, 4200, 2)][1] == 2
    # a large L whose last workgroup has whole waves beyond L, with one live column
    for (cin, cout, L, B), want in pw.TABLE.items():
        if want[0] == "large" and L == 4097:
            cols = pw.path(cin, cout, L, B)[1]
            assert L % cols == 1 and cols // 4 > 1


def test_plan_mirror_at_the_lds_edges():
    from lion_amd import _lib
    lib = _lib.load()
    for cout in (32, 64, 128, 256, 96, 320):
        for cin in range(1, 1300, 7):
            cb, vb = pw.pw_plan(cout, cin)
            assert lib.lion_pwconv_stat_tiles(cout, cin, 100000) == (math.ceil(100000 / (128 * vb)) if cb else 0), (cout, cin)
    assert pw.pw_plan(256, 136) == (8, 1) and pw.pw_plan(256, 137) == (4, 2)
    assert pw.pw_plan(128, 284) == (4, 2) and pw.pw_plan(128, 285) == (2, 4)
    assert pw.pw_plan(32, 1200) == (0, 0)


def test_swish64_and_bound_are_those_of_pointwise_ref():
    t = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 0.3, -1.278, 20.0, -20.0, 100.0, -100.0, 1e4, -1e4], dtype=torch.float64)
    s = pw.swish64(t)
    assert np.array_equal(s.numpy(), pr.swish64(t.numpy()))
    assert np.allclose(pw.swish_bound(t, s, torch.zeros_like(t)).numpy(), pr.swish_bound(t.numpy()), rtol=1e-15, atol=0)
    x = torch.linspace(-8, 8, 100001, dtype=torch.float64)
    slope = (pw.swish64(x[1:]) - pw.swish64(x[:-1])) / (x[1:] - x[:-1])
    assert slope.abs().max().item() < 1.1      # the Lipschitz constant of operand64 / max64


@pytest.mark.parametrize("pro", [False, True])
def test_pwconv64_is_the_module_arithmetic(pro):
    x, w, bias, p = pw.make_data("unit", 7, 5, 40, 2, 3)
    ref, bound = pw.pwconv64(x, w, bias, p if pro else None)
    xin = x.double()
    if pro:
        t = xin * p[0].double()[:, :, None] + p[1].double()[:, :, None]
        xin = t * torch.sigmoid(t)
    want = torch.nn.functional.conv1d(xin, w.double()[:, :, None], bias.double())
    assert (ref - want).abs().max().item() <= 1e-14 * want.abs().max().item()
    assert bool((bound > 0).all()) and bound.max().item() < 1e-5
    s, b = pw.tile_stats64(ref, bound, 32)
    assert tuple(s.shape) == (2, 5, 2, 2)
    assert torch.allclose(s[:, :, 1, 0], ref[:, :, 32:].sum(-1), rtol=1e-14, atol=1e-14)
    assert torch.allclose(s[:, :, 0, 1], ref[:, :, :32].square().sum(-1), rtol=1e-14)


def test_integer_data_is_exact_and_the_emulation_reproduces_it():
    for cin, cout, L, cols in ((5, 3, 33, 32), (131, 4, 40, 32), (7, 3, 300, 128), (3, 2, 700, 512)):
        x, w, bias, _ = pw.make_data("int", cin, cout, L, 2, cin)
        assert pw.exact_ok(x, w, bias)
        ref, _ = pw.pwconv64(x, w, bias)
        s, _ = pw.tile_stats64(ref, torch.zeros_like(ref), cols)
        assert s.abs().max().item() < pw.EXACT_MAX
        y, st = pw.emulate_pwconv32(x.numpy(), w.numpy(), bias.numpy(), None, cols)
        assert np.array_equal(y.astype(np.float64), ref.numpy()) and np.array_equal(st.astype(np.float64), s.numpy())


# (Cin, Cout, L, B, columns per tile): both kernels, ragged tails, idle waves, every depth of the reduction
EMU = [(1, 3, 33, 2, 32), (5, 4, 40, 2, 32), (131, 6, 70, 1, 32), (35, 5, 200, 2, 128), (9, 3, 300, 2, 256),
       (67, 4, 600, 1, 512), (259, 3, 40, 1, 32)]


@pytest.mark.parametrize("kind", pw.KINDS)
@pytest.mark.parametrize("cin,cout,L,B,cols", EMU)
def test_bounds_hold_for_the_kernels_own_arithmetic(kind, cin, cout, L, B, cols):
    x, w, bias, pro = pw.make_data(kind, cin, cout, L, B, cin + L)
    for p, fused in ((None, False), (pro, False), (pro, True)):
        ref, bound = pw.pwconv64(x, w, bias, p)
        sref, sbound = pw.tile_stats64(ref, bound, cols)
        pn = None if p is None else (p[0].numpy(), p[1].numpy())
        y, st = pw.emulate_pwconv32(x.numpy(), w.numpy(), bias.numpy(), pn, cols, fused_arg=fused)
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(st))
        assert ratio(y, ref, bound) <= 1.0
        assert ratio(st, sref, sbound) <= 1.0


def test_cancelling_data_cancels_and_bias_dominates():
    x, w, bias, _ = pw.make_data("cancel", 64, 8, 64, 1, 0)
    parts = [torch.einsum("oc,bcl->bol", w[:, lo:lo + 16].double(), x[:, lo:lo + 16].double()) for lo in range(0, 64, 16)]
    assert (parts[0] + parts[1]).abs().mean().item() < 0.1 * parts[0].abs().mean().item()
    assert (parts[2] + parts[3]).abs().mean().item() < 0.1 * parts[2].abs().mean().item()
    x, w, bias, _ = pw.make_data("bias", 64, 8, 64, 1, 0)
    ref, _ = pw.pwconv64(x, w, bias)
    assert ref.mean(-1).abs().min().item() > 30 * ref.std(-1).max().item()


def test_bounds_tell_the_mistakes_apart():
    """what the GPU tests are there to catch moves a result by far more than its bound: a tile sum in the neighbouring
    slot, a clamped column counted in a ragged tile, one weight taken from the neighbouring channel"""
    x, w, bias, _ = pw.make_data("unit", 35, 8, 100, 2, 1)
    ref, bound = pw.pwconv64(x, w, bias)
    s, b = pw.tile_stats64(ref, bound, 32)
    assert float(((s[:, :, 1:] - s[:, :, :-1]).abs() / b[:, :, 1:]).min()) > 100
    counted = s[:, :, 3, 1] + 28 * ref[:, :, 99] ** 2       # the 28 columns beyond L loaded from column L - 1
    assert float(((counted - s[:, :, 3, 1]) / b[:, :, 3, 1]).min()) > 100
    w2 = w.clone()
    w2[:, 0] = w[:, 0].roll(1)
    wrong, _ = pw.pwconv64(x, w2, bias)
    assert float(((wrong - ref).abs() / bound).median()) > 100


def test_max64_is_the_max_of_the_activated_group():
    x, w, bias, pro = pw.make_data("unit", 6, 4, 64, 2, 5)
    ref, bound = pw.pwconv64(x, w, bias)
    a, b = pro[0][:, :4], pro[1][:, :4]
    m, e = pw.max64(ref, bound, a, b)
    t = ref * a.double()[:, :, None] + b.double()[:, :, None]
    want = (t * torch.sigmoid(t)).view(2, 4, 2, 32).amax(-1)
    assert (m - want).abs().max().item() <= 1e-14 and tuple(e.shape) == (2, 4, 2) and bool((e > 0).all())
    # the kernel's epilogue in fp32 on the emulated y stays inside
    y, _ = pw.emulate_pwconv32(x.numpy(), w.numpy(), bias.numpy(), None, 512)
    t32 = ((y * a.numpy()[:, :, None]).astype(np.float32) + b.numpy()[:, :, None]).astype(np.float32)
    got = pw._swish_fast32(t32).reshape(2, 4, 2, 32).max(-1)
    assert ratio(got, m, e) <= 1.0


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("B,K,O", [(1, 1, 1), (33, 3, 31), (5, 129, 65), (70, 2, 33)])
def test_linear_bound_holds_for_the_kernels_own_arithmetic(B, K, O, act):
    g = torch.Generator().manual_seed(B + K + O)
    x = torch.randn(B, K, generator=g)
    w = torch.randn(O, K, generator=g) / math.sqrt(K)
    bias = torch.randn(O, generator=g) * 0.1
    ref, bound = pw.linear64(x, w, bias, act, 0.1)
    want = x.double() @ w.double().t() + bias.double()
    want = {0: want, 1: torch.relu(want), 2: torch.nn.functional.leaky_relu(want, 0.1)}[act]
    assert (ref - want).abs().max().item() <= 1e-14
    got = pw.emulate_linear32(x.numpy(), w.numpy(), bias.numpy(), act, 0.1)
    assert ratio(got, ref, bound) <= 1.0


def test_packed_layout():
    w = torch.arange(1, 3 * 5 + 1, dtype=torch.float32).view(3, 5)
    p = pw.packed_layout(w)
    assert tuple(p.shape) == (6, 64) and p[4, 2] == w[2, 4] and p[0, 1] == w[1, 0]
    assert p[5].abs().sum() == 0 and p[:, 3:].abs().sum() == 0 and p.sum() == w.sum()
