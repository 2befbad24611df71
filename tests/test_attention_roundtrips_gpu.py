"""-m gpu: lion_linear_attention_core on its resident path (k read once into LDS) and its streaming path (loads a tile
ahead) against the plain kernel they replaced (lion_internal_linear_attention_core_plain), bit for bit on int32 views.
Only the memory schedule -- and where the one expf per element is kept -- differs: any difference at all is a bug."""
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (4, 16, 60, 64, 68, 124, 128, 132, 1020, 1024, 1028, 2048)
DATA = ("gauss", "wide-rows", "constant-row")


def lib():
    from lion_amd import _lib
    return _lib.load()


def bits(t):
    return t.contiguous().view(torch.int32)


def make_qkv(B, H, N, data, offset=0):
    """qkv f32 [B, 3 * H * 32, N], starting `offset` floats into its (256-byte aligned) allocation"""
    gen = torch.Generator(device="cuda").manual_seed(zlib.crc32(repr((B, H, N, data)).encode()) & 0x7fffffff)
    vals = torch.randn(B, 3, H, 32, N, device="cuda", generator=gen)
    k = vals[:, 1]
    if data == "wide-rows":   # every row of k spans -80 .. 80: expf underflows to 0 for most of a row
        k.copy_(torch.rand(B, H, 32, N, device="cuda", generator=gen) * 160.0 - 80.0)
        k[..., 0] = -80.0
        k[..., N - 1] = 80.0
    elif data == "constant-row":   # row 7 of every head is one value: p = 1 / N
        k[:, :, 7, :] = 3.25
    buf = torch.empty(vals.numel() + offset, device="cuda")
    qkv = buf[offset:].view(B, 3 * H * 32, N)
    qkv.copy_(vals.view(B, 3 * H * 32, N))
    return qkv


def run(name, qkv, B, H, N, offset=0):
    from lion_amd import _lib
    buf = torch.full((B * H * 32 * N + offset,), float("nan"), device="cuda")
    out = buf[offset:].view(B, H * 32, N)
    _lib.call(name, qkv, B, H, 32, N, out)
    return out


def test_paths():
    path = lib().lion_internal_linear_attention_path
    assert {n: path(n, 1) for n in NS} == {n: (1 if n <= 1024 else 2) for n in NS}
    assert [path(n, 1) for n in (1, 63, 65)] == [0, 0, 0]
    assert [path(n, 0) for n in (64, 1024, 2048)] == [0, 0, 0]


@pytest.mark.parametrize("N", NS)
def test_core_equals_the_plain_kernel_bit_for_bit(N):
    assert lib().lion_internal_linear_attention_path(N, 1) in (1, 2)
    for B in (1, 3):
        for H in (1, 4, 8):
            for data in DATA:
                qkv = make_qkv(B, H, N, data)
                assert qkv.data_ptr() % 16 == 0
                got = run("lion_linear_attention_core", qkv, B, H, N)
                ref = run("lion_internal_linear_attention_core_plain", qkv, B, H, N)
                assert torch.isfinite(ref).all(), (B, H, N, data)
                assert torch.equal(bits(got), bits(ref)), ((B, H, N, data), int((bits(got) != bits(ref)).sum()))


@pytest.mark.parametrize("N", [1, 63, 65])
def test_point_counts_off_four_take_the_plain_kernel(N):
    assert lib().lion_internal_linear_attention_path(N, 1) == 0
    qkv = make_qkv(3, 4, N, "gauss")
    got = run("lion_linear_attention_core", qkv, 3, 4, N)
    ref = run("lion_internal_linear_attention_core_plain", qkv, 3, 4, N)
    assert torch.isfinite(ref).all() and torch.equal(bits(got), bits(ref))


@pytest.mark.parametrize("N", [64, 1024])
def test_a_view_one_float_into_its_buffer_takes_the_plain_kernel(N):
    """qkv (or out) 4 bytes off a 16-byte boundary cannot be read in 16-byte pieces: the launcher sees it in the pointer
    and runs the plain kernel, with the result of the aligned call"""
    B, H = 3, 4
    aligned, shifted = make_qkv(B, H, N, "gauss"), make_qkv(B, H, N, "gauss", offset=1)
    assert shifted.data_ptr() % 16 == 4 and torch.equal(aligned, shifted)
    assert lib().lion_internal_linear_attention_path(N, int(shifted.data_ptr() % 16 == 0)) == 0
    ref = run("lion_linear_attention_core", aligned, B, H, N)
    for q, off in ((shifted, 0), (aligned, 1), (shifted, 1)):
        got = run("lion_linear_attention_core", q, B, H, N, offset=off)
        assert torch.equal(bits(got), bits(ref)), (N, off)
