"""The 1x1-convolution entry points (csrc/pwconv.hip, csrc/pwconv_split.hip) refuse these calls BEFORE any launch: the return
code of each is pinned here, through ctypes on the loaded library with dummy non-null pointers (never dereferenced) and a
NULL stream.  -1 is LION_EINVAL, -2 LION_EUNSUPPORTED; a dispatch bug that let one of these calls reach a launch shows up on
a machine without a GPU as a positive HIP error code.  The module skips itself where a GPU is present: a dummy pointer must
never be able to reach a kernel there."""
import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="dummy pointers: only where no launch can succeed")

P = 4096           # a non-null pointer; every case returns before anything reads it
EINVAL, EUNSUPPORTED = -1, -2


def _call(name, order, defaults, over):
    from lion_amd import _lib
    unknown = set(over) - set(defaults)
    assert not unknown, unknown
    args = dict(defaults, **over)
    return getattr(_lib.load(), name)(*[args[k] for k in order.split()], None)


def forward(**over):
    return _call("lion_pwconv_forward", "x wp bias B Cin Cout L pro_a pro_b y stats",
                 dict(x=P, wp=P, bias=P, B=1, Cin=64, Cout=64, L=8192, pro_a=None, pro_b=None, y=P, stats=P), over)


def forward_max(**over):
    return _call("lion_pwconv_forward_max", "x wp bias B Cin Cout L pro_a pro_b out_a out_b stats ymax",
                 dict(x=P, wp=P, bias=P, B=1, Cin=64, Cout=64, L=8192, pro_a=None, pro_b=None, out_a=None, out_b=None,
                      stats=P, ymax=None), over)


def grouped(name="lion_pwconv_grouped_forward", **over):
    return _call(name, "coords centers feat idx wp bias B C N M U Cout y stats",
                 dict(coords=P, centers=P, feat=P, idx=P, wp=P, bias=P, B=1, C=0, N=8, M=2, U=4, Cout=32, y=P, stats=P), over)


def split_grouped(**over):
    return grouped("lion_pwconv_split_grouped_forward", **over)


def walk(**over):
    return _call("lion_internal_pwconv_walk",
                 "x wp bias B Cin Cout L pro_a pro_b out_a out_b coords centers feat idx N U y stats max_wg lds_weights",
                 dict(x=P, wp=P, bias=P, B=1, Cin=64, Cout=64, L=64, pro_a=None, pro_b=None, out_a=None, out_b=None,
                      coords=None, centers=None, feat=None, idx=None, N=0, U=0, y=P, stats=P, max_wg=0, lds_weights=-1), over)


def walk_gathered(**over):
    return walk(**dict(dict(x=None, coords=P, centers=P, idx=P, N=8, U=4, L=8, Cin=3), **over))


def split_forward(**over):
    return _call("lion_pwconv_split_forward", "x wp bias B Cin Cout L pro_a pro_b y stats",
                 dict(x=P, wp=P, bias=P, B=1, Cin=64, Cout=64, L=8192, pro_a=None, pro_b=None, y=P, stats=P), over)


def test_forward():
    assert forward(x=None) == EINVAL
    assert forward(pro_a=P) == EINVAL
    assert forward(L=0) == EINVAL
    assert forward(L=1 << 27) == EUNSUPPORTED
    assert forward(Cin=2048, Cout=32) == EUNSUPPORTED                         # no channel tile fits LDS
    assert forward(Cin=9000, Cout=32, L=64, pro_a=P, pro_b=P) == EUNSUPPORTED  # prologue scalars beyond 64 KiB


def test_forward_max():
    assert forward_max(out_a=P) == EINVAL
    assert forward_max(stats=None) == EINVAL
    assert forward_max(out_a=P, out_b=P) == EINVAL                            # second pass without ymax
    assert forward_max(x=None, L=33) == EINVAL                                # EINVAL wins over the unsupported L
    for L in (8200, 4096, 1 << 27):
        assert forward_max(L=L) == EUNSUPPORTED, L
    assert forward_max() == EUNSUPPORTED                                      # first pass, 16 tiles: grid below 2048
    assert forward_max(Cin=2048, Cout=32) == EUNSUPPORTED


def test_grouped_forward():
    assert grouped(idx=None) == EINVAL
    assert grouped(C=32, feat=None) == EINVAL
    assert grouped(M=1 << 16, U=1 << 15) == EUNSUPPORTED
    assert grouped(N=1 << 27, M=1024, U=32, Cout=64) == EUNSUPPORTED
    assert grouped(C=1 << 20, N=1 << 11) == EUNSUPPORTED


def test_walk():
    assert walk(wp=None) == EINVAL
    assert walk(y=None, stats=None) == EINVAL
    assert walk(out_a=P, out_b=P, y=None) == EINVAL
    assert walk(x=None) == EINVAL
    assert walk_gathered(pro_a=P, pro_b=P) == EINVAL
    assert walk_gathered(L=10) == EINVAL
    assert walk_gathered(Cin=2) == EINVAL
    assert walk_gathered(Cin=5) == EINVAL                                     # features without feat
    assert walk_gathered(y=None) == EINVAL
    assert walk(y=None, L=33) == EUNSUPPORTED                                 # sums only
    assert walk(L=1 << 27) == EUNSUPPORTED
    assert walk(Cin=2048, Cout=32) == EUNSUPPORTED


def test_split_forward():
    assert split_forward(y=None) == EINVAL
    assert split_forward(pro_b=P) == EINVAL
    assert split_forward(Cin=4097, L=16) == EUNSUPPORTED
    assert split_forward(Cin=4096, L=1 << 17) == EUNSUPPORTED


def test_split_grouped_forward():
    assert split_grouped(C=8, feat=None) == EINVAL
    assert split_grouped(C=5000, M=1, U=1) == EUNSUPPORTED
    assert split_grouped(N=1 << 28, M=1, U=1) == EUNSUPPORTED
    assert split_grouped(M=1 << 15, U=1 << 13) == EUNSUPPORTED
