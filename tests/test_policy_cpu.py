"""host logic that picks the arithmetic of a layer (no GPU): split-operand kernels where they can run and are the faster
ones, the fp32 MFMA kernels elsewhere; explicit True / False override the module policy but never the kernel's limits."""
from lion_amd import conv_ops, fused_ops


def test_conv_split_policy():
    assert conv_ops.split_supported(64, 64, 32) and conv_ops.split_supported(128, 128, 8)
    assert not conv_ops.split_supported(4, 32, 32)        # Cin % 16 != 0: the first layer stays on the fp32 kernel
    assert not conv_ops.split_supported(64, 48, 32)       # Cout % 32 != 0
    assert not conv_ops.split_supported(64, 64, 12)
    assert conv_ops.use_split(True, 64, 64, 16) and not conv_ops.use_split(False, 64, 64, 16)
    assert not conv_ops.use_split(True, 35, 64, 16)       # forcing cannot make an unsupported shape run
    assert conv_ops.use_split(None, 128, 128, 8) == (conv_ops.SPLIT and conv_ops.SPLIT_MIN_R <= 8)


def test_conv_route_follows_the_policy():
    """conv_route names the split / half entry points exactly where use_split / use_half say so, and only entry points the
    library has; an input that requires grad never goes to the half kernel"""
    import torch
    from lion_amd import _lib
    shapes = [(64, 64, 32), (128, 128, 8), (4, 32, 32), (64, 48, 32), (64, 64, 12), (64, 64, 16), (35, 64, 16),
              (128, 128, 16), (16, 32, 16)]                # those of test_conv_split_policy and of the half policy's table
    grad_x = torch.zeros(1, 64, 2, 2, 2, requires_grad=True)
    for precision in conv_ops.PRECISIONS:
        with conv_ops.conv_precision(precision):
            for shape in shapes:
                for split in (None, True, False):
                    route = conv_ops.conv_route(*shape, split=split)
                    want = "f32" if not conv_ops.use_split(split, *shape) else "half" if conv_ops.use_half(*shape) else "split"
                    assert route.kind == want, (precision, shape, split)
                    names = [v for v in route if isinstance(v, str) and v != route.kind]
                    assert len(names) == 2 and all(n in _lib.SIGNATURES for n in names), (precision, shape, split, names)
                    assert ("_half_" in route.forward) == (route.kind == "half"), (precision, shape, split)
                    assert route.kind != "half" or conv_ops.half_supported(*shape), (precision, shape, split)
                    assert conv_ops.conv_route(*shape, split=split, half=False).kind in ("f32", "split")
                    with torch.enable_grad():
                        assert conv_ops.conv_route(*shape, split=split, x=grad_x).kind != "half", (precision, shape, split)
    with conv_ops.conv_precision("half"):
        assert conv_ops.conv_route(64, 64, 32, split=True).kind == "half"   # (so the loop above did see the half route)


def test_pointwise_split_policy():
    pol = fused_ops.pw_use_split
    if fused_ops.PW_SPLIT:
        assert pol(None, 32, 192, 128, 2048)              # feature propagation at N = 2048: 65536 columns
        assert pol(None, 32, 320, 256, 512)
        assert not pol(None, 32, 256, 128, 128)           # 4096 columns: a handful of workgroups, latency bound
        assert not pol(None, 32, 35, 32, 32768)           # long and thin: the fp32 kernel already streams it
        assert pol(None, 32, 64, 128, 8192)
        assert not pol(None, 1, 128, 128, 2048)           # B = 1 demo config
    assert pol(True, 1, 128, 128, 16) and not pol(False, 32, 192, 128, 2048)
    assert not pol(True, 2, 4096, 64, 1 << 18)            # Cin * L beyond the 32-bit byte offsets of the kernel


def test_pointwise_route_follows_the_policy():
    """pw_route names the split entry points exactly where pw_use_split says so, and only entry points the library has"""
    from lion_amd import _lib
    shapes = [(32, 192, 128, 2048), (32, 320, 256, 512), (32, 256, 128, 128), (32, 35, 32, 32768), (32, 64, 128, 8192),
              (1, 128, 128, 2048), (1, 128, 128, 16), (2, 4096, 64, 1 << 18)]     # those of test_pointwise_split_policy
    for shape in shapes:
        for split in (None, True, False):
            route = fused_ops.pw_route(*shape, split=split)
            use = fused_ops.pw_use_split(split, *shape)
            names = [v for v in route if isinstance(v, str)]
            assert route.split == use and len(names) == 3, (shape, split)
            for name in names:
                assert name in _lib.SIGNATURES and ("_split_" in name) == use, (shape, split, name)
