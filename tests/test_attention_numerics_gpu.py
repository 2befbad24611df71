"""-m gpu: the LinearAttention core, csrc/attention.hip, forward and backward against the float64 expression and its
autograd at the point counts where the kernels change path -- 8 (lanes per softmax row), 32 (column block), 64 (staged
tile), 128 (four waves x 32) -- with logits that need the max-subtraction, and with the error taken per (batch, head)
block, and per gradient part, so that a wrong head cannot hide next to a large one."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
BH = ((1, 1), (2, 3))
DATA = ("unit", "shifted", "dominant", "flat", "head-disparity")
# The project's bounds; every case below meets them, so none has a bound of its own.  Measured on the MI355X, worst block
# over all cases, under the measures below (kernel / the same expressions in fp32 torch):
#     forward 1.7e-7 / 1.7e-7      gq 4.4e-7 / 6.4e-7      gk 4.7e-7 / 5.4e-7      gv 7.4e-7 / 7.6e-7
FWD_TOL = 1e-5    # fp32 kernels against float64
GRAD_TOL = 5e-5   # per gradient part (tests/test_train_ops_gpu.py)


def make_case(B, H, N, data):
    """qkv f32 [B, 3 * H * 32, N] and gout f32 [B, H * 32, N]"""
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((B, H, N, data)).encode()) & 0x7fffffff)
    qkv = torch.randn(B, 3, H, 32, N, device="cuda", generator=gen) * 1.5
    gout = torch.randn(B, H, 32, N, device="cuda", generator=gen)
    k = qkv[:, 1]
    if data == "shifted":   # a constant per row of k: the softmax is that of the shifted float32 values, which the reference reads too
        shifts = torch.tensor([-1e4, -80.0, 30.0, 80.0, 1e4], device="cuda")
        k += shifts[torch.arange(B * H * 32, device="cuda") % 5].view(B, H, 32, 1)
    elif data == "dominant":   # one point per row leads the others by 60
        lead = torch.randint(0, N, (B, H, 32, 1), device="cuda", generator=gen)
        k.scatter_(3, lead, k.amax(3, keepdim=True) + 60.0)
    elif data == "flat":   # a row of equal logits: p = 1 / N, exactly for a power of two
        k.copy_(k[..., :1].expand_as(k).clone())
    elif data == "head-disparity":   # q, v and gout of head h at 10^(-3h) of head 0
        scale = (10.0 ** (-3.0 * torch.arange(H, device="cuda"))).view(1, H, 1, 1)
        qkv[:, 0] *= scale
        qkv[:, 2] *= scale
        gout *= scale
    return qkv.reshape(B, 3 * H * 32, N).contiguous(), gout.reshape(B, H * 32, N).contiguous()


def core(qkv, B, H, N):
    """the reference's expressions (models/pvcnn2_ada.py:62-68) in the dtype of qkv -> out [B, H, 32, N] and its parts"""
    q, k, v = qkv.view(B, 3, H, 32, N).unbind(1)
    p = k.softmax(dim=-1)
    ctx = torch.einsum("bhdn,bhen->bhde", p, v)
    return torch.einsum("bhde,bhdn->bhen", ctx, q), (q, p, v)


def block_max(t):
    """[B, H, rows, N] -> [B, H]"""
    return t.flatten(2).amax(2)


def forward_measure(out, ref, q, p, v):
    """per (batch, head): max |out - ref| / max over (e, n) of sum_d |ctx|[d, e] |q[d, n]|, |ctx| = sum_n p |v|"""
    actx = torch.einsum("bhdn,bhen->bhde", p, v.abs())
    norm = block_max(torch.einsum("bhde,bhdn->bhen", actx, q.abs()))
    return block_max((out.double() - ref).abs()) / norm


def gradient_measures(g, gref, gout64, q, p, v):
    """per (batch, head, part): max |g - gref| over the block / the block's scale.  gq and gv: the block's max |gref|,
    as tests/test_train_ops_gpu.py takes it over the tensor.  gk = p (gp - dot) is a difference that is exactly zero for
    N = 1 and for a flat row: its scale is the block's max of p (|gp| + |dot|), the two terms the kernel subtracts."""
    B, H, _, N = q.shape
    g, gref = g.view(B, 3, H, 32, N).double(), gref.view(B, 3, H, 32, N)
    err = [block_max((g[:, i] - gref[:, i]).abs()) for i in range(3)]
    gctx = torch.einsum("bhdn,bhen->bhde", q, gout64)
    gp = torch.einsum("bhde,bhen->bhdn", gctx, v)
    dot = (p * gp).sum(-1, keepdim=True)
    norm = [block_max(gref[:, 0].abs()), block_max(p * (gp.abs() + dot.abs())), block_max(gref[:, 2].abs())]
    return torch.stack([e / n for e, n in zip(err, norm)], -1)   # [B, H, 3]


def reference(qkv, gout, B, H, N):
    q64 = qkv.double().requires_grad_(True)
    ref, (q, p, v) = core(q64, B, H, N)
    (gref,) = torch.autograd.grad(ref, q64, gout.double().view(B, H, 32, N))
    return ref.detach(), gref, q.detach(), p.detach(), v.detach()


def torch_fp32(qkv, gout, B, H, N):
    """the same expressions in fp32 torch: what the kernel's error is put next to when it is printed"""
    x = qkv.clone().requires_grad_(True)
    out, _ = core(x, B, H, N)
    (g,) = torch.autograd.grad(out, x, gout.view(B, H, 32, N))
    return out.detach(), g


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("N", NS)
def test_linear_attention_forward_per_head(N, B, H, data):
    from lion_amd import fused_ops
    qkv, gout = make_case(B, H, N, data)
    ref, _, q, p, v = reference(qkv, gout, B, H, N)
    with torch.no_grad():
        out = fused_ops.linear_attention_core(qkv, H, 32)
    assert out.shape == (B, H * 32, N) and torch.isfinite(out).all()
    m = forward_measure(out.view(B, H, 32, N), ref, q, p, v)
    mt = forward_measure(torch_fp32(qkv, gout, B, H, N)[0], ref, q, p, v)
    print(f"attention forward N={N} B={B} H={H} {data}: kernel {m.max().item():.3e} fp32-torch {mt.max().item():.3e}")
    assert (m < FWD_TOL).all(), m


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("N", NS)
def test_linear_attention_backward_per_head_and_part(N, B, H, data):
    from lion_amd import train_ops
    qkv, gout = make_case(B, H, N, data)
    ref, gref, q, p, v = reference(qkv, gout, B, H, N)
    x = qkv.clone().requires_grad_(True)
    out = train_ops.linear_attention_core(x, H)
    (g,) = torch.autograd.grad(out, x, gout)
    assert torch.isfinite(g).all()
    gout64 = gout.double().view(B, H, 32, N)
    assert (forward_measure(out.detach().view(B, H, 32, N), ref, q, p, v) < FWD_TOL).all()
    m = gradient_measures(g, gref, gout64, q, p, v)
    mt = gradient_measures(torch_fp32(qkv, gout, B, H, N)[1], gref, gout64, q, p, v)
    worst, worst_t = m.amax((0, 1)).tolist(), mt.amax((0, 1)).tolist()
    print(f"attention backward N={N} B={B} H={H} {data}: kernel q {worst[0]:.3e} k {worst[1]:.3e} v {worst[2]:.3e}"
          f" fp32-torch q {worst_t[0]:.3e} k {worst_t[1]:.3e} v {worst_t[2]:.3e}")
    assert (m < GRAD_TOL).all(), m
