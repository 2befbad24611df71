"""The voxel Conv3d entry points (csrc/conv3d.hip, conv3d_split.hip, conv3d_half.hip, conv3d_wgrad.hip) and the two readers of
their tile geometry (lion_conv3d_tile_occupancy_aware, lion_voxel_scatter_read) refuse these calls BEFORE any launch: the
return code of each is pinned here, through ctypes on the loaded library with dummy non-null pointers (never dereferenced)
and a NULL stream.  -1 is LION_EINVAL, -2 LION_EUNSUPPORTED, -3 LION_EWORKSPACE.  The module skips itself where a GPU is
present: a dummy pointer must never be able to reach a kernel there.

Only calls that are refused before the launcher are here.  A call that gets as far as the launcher asks for the current
device first, and without a device that answers -1 as well: a -1 could then not tell a refusal from a launch, so every
LION_EINVAL case below is one of the argument checks in front of the plan, and shapes that have a kernel (r = 8 on the fp32
and split entries, Cin = 24 on the fp32 entry, Cin = 12 on the fp32 weight gradient, ...) are left out.

One code is kept on purpose: the half entry has no kernel of its own below r = 16 or off the split kernel's channel
counts and answers LION_EINVAL there, not LION_EUNSUPPORTED (conv_ops.use_half never sends such a shape)."""
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no launch can succeed")

P = 4096           # a non-null, 16-byte aligned pointer; every case returns before anything reads it
ODD = 4100         # ... and one that is not 16-byte aligned
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
FUSED, SPLIT, HALF = "lion_conv3d_k3_fused_forward", "lion_conv3d_k3_split_forward", "lion_conv3d_k3_half_forward"
PRO = dict(pro_a=P, pro_b=P)


def _call(name, order, defaults, over):
    from lion_amd import _lib
    unknown = set(over) - set(defaults)
    assert not unknown, unknown
    args = dict(defaults, **over)
    return getattr(_lib.load(), name)(*[args[k] for k in order.split()], None)


def forward(name, **over):
    return _call(name, "x wp bias B Cin Cout r pro_a pro_b pro_bias tconst y stats occ",
                 dict(x=P, wp=P, bias=P, B=1, Cin=64, Cout=64, r=16, pro_a=None, pro_b=None, pro_bias=None, tconst=None, y=P,
                      stats=P, occ=None), over)


def wgrad(name, **over):
    return _call(name, "x gy B Cin Cout r gw ws ws_floats",
                 dict(x=P, gy=P, B=1, Cin=16, Cout=32, r=16, gw=P, ws=P, ws_floats=2 ** 40), over)


def wgrad_sparse(**over):
    return _call("lion_conv3d_k3_wgrad_split_sparse", "x gy cnt B Cin Cout r gw ws ws_floats",
                 dict(x=P, gy=P, cnt=P, B=1, Cin=16, Cout=32, r=16, gw=P, ws=P, ws_floats=2 ** 40), over)


def occupancy(**over):
    return _call("lion_conv3d_tile_occupancy_aware", "cnt B r Cout m1 m2 aware",
                 dict(cnt=P, B=1, r=16, Cout=64, m1=P, m2=P, aware=0), over)


def scatter_read(**over):
    return _call("lion_voxel_scatter_read", "feat plan plan_bytes B C N r occ out",
                 dict(feat=P, plan=P, plan_bytes=2 ** 40, B=1, C=16, N=256, r=16, occ=P, out=P), over)


@pytest.mark.parametrize("name", [FUSED, SPLIT, HALF])
def test_forward_argument_checks(name):
    assert forward(name, x=None) == EINVAL
    assert forward(name, pro_a=P) == EINVAL                                   # half a prologue
    assert forward(name, tconst=P) == EINVAL                                  # a constant response without a prologue
    assert forward(name, occ=P, **PRO) == EINVAL                              # an activated input is sparse only as delta
    assert forward(name, B=0) == EINVAL
    assert forward(name, Cin=272, **PRO) == EUNSUPPORTED                      # prologue scalars of more than 256 channels


@pytest.mark.parametrize("name, code", [(FUSED, EUNSUPPORTED), (SPLIT, EUNSUPPORTED), (HALF, EINVAL)])
def test_forward_shapes_without_a_kernel(name, code):
    assert forward(name, r=12) == code
    assert forward(name, Cout=48) == code
    assert forward(name, Cin=6) == code
    assert forward(name, r=8, Cout=48) == code
    if name != FUSED:                                                         # (the fp32 kernel takes Cin % 4 == 0)
        assert forward(name, Cin=24) == code
        assert forward(name, r=8, occ=P) == code                              # the r = 8 split kernel has no work queue
        assert forward(name, r=8, tconst=P, **PRO) == code                    # ... and no constant + delta form
    if name == HALF:
        assert forward(name, r=8) == EINVAL                                   # r = 8 stays on the three-product kernel


@pytest.mark.parametrize("name", ["lion_conv3d_k3_wgrad", "lion_conv3d_k3_wgrad_split"])
def test_wgrad(name):
    assert wgrad(name, x=None) == EINVAL
    assert wgrad(name, Cin=6) == EUNSUPPORTED
    assert wgrad(name, Cout=48) == EUNSUPPORTED
    assert wgrad(name, r=12) == EUNSUPPORTED
    assert wgrad(name, ws=None) == EWORKSPACE
    assert wgrad(name, ws_floats=0) == EWORKSPACE
    if name.endswith("_split"):
        assert wgrad(name, Cin=12) == EUNSUPPORTED                            # Cin % 8
        assert wgrad(name, x=ODD) == EUNSUPPORTED                             # 16-byte loads


def test_wgrad_sparse_and_the_workspace_queries():
    from lion_amd import _lib
    lib = _lib.load()
    assert wgrad_sparse(cnt=None) == EINVAL
    assert wgrad_sparse(cnt=ODD) == EUNSUPPORTED
    assert wgrad_sparse(Cin=12) == EUNSUPPORTED
    assert lib.lion_conv3d_wgrad_workspace_floats(1, 16, 32, 16) == 110656    # 4 splits of 32 * 16 * 27 partials + 64
    assert lib.lion_conv3d_wgrad_sparse_workspace_floats(1, 16, 32, 16) == 110720
    assert lib.lion_conv3d_wgrad_sparse_workspace_floats(1, 6, 32, 16) == 0


def test_tile_occupancy():
    assert occupancy(r=8) == EUNSUPPORTED                                     # sparse plans exist at r = 16 / 32
    assert occupancy(cnt=ODD) == EUNSUPPORTED
    assert occupancy(m1=None, m2=None) == EINVAL
    assert occupancy(Cout=48) == EUNSUPPORTED


def test_voxel_scatter_read():
    assert scatter_read(occ=None) == EINVAL
    assert scatter_read(r=8) == EUNSUPPORTED
    assert scatter_read(out=ODD) == EUNSUPPORTED
    assert scatter_read(plan_bytes=0) == EWORKSPACE
