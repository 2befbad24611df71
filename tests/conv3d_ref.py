"""Float64 references, error bounds, the tile plan and the case table for conv3d_k3_kernel, the exact-fp32 MFMA 3x3x3
convolution of csrc/conv3d.hip, and a numpy emulation of the kernel's own arithmetic that
tests/test_conv3d_reference_cpu.py holds to the same bounds.  torch on any device (the GPU tests evaluate the float64 side
on the device, in batch chunks); imports nothing from lion_amd.

u = 2^-24 is the unit roundoff of fp32 (pointwise_ref.U32) and K = 27 ceil4(Cin) the number of products behind one output:
the kernel walks the input channels in chunks of four (the wrapper pads Cin with zero channels), each MFMA step is an fma
per k, i.e. ONE rounding per product.

Bounds, all elementwise and derived -- none is a measured figure (first order in u; the neglected factor 1 / (1 - K u) is
below 1.0005 at the largest K here, 27 x 256):
  plain     |y - ref| <= (K + 2) u (conv64(|x|, |w|) + |bias|).  K fused accumulations and the bias add round once each,
            whatever their order (the dot-product bound, Higham, Accuracy and Stability, 3.1); one more u is slack.
  prologue  the staged input is z~ = swish_fast(fl(x a + b)) for z = swish64(x a + b): with |z~ - z| <= E_in the exact
            result moves by at most conv64(E_in, |w|), and the plain bound holds with |z| in place of |x|.
            E_in = pointwise_ref.swish_bound(t) + 1.1 u |x a|, t = x a + b in float64: swish_bound is swish_fast's error on
            its fp32 argument, and the rounding of the product x a -- which an fma saves and two separate operations
            make -- goes through swish, 1.1-Lipschitz.  The rounding of the sum moves swish by u |t swish'(t)| <=
            1.28 u |swish(t)| for t >= -0.7, inside the 2 u of slack swish_bound keeps; for a negative argument whose
            shift dominates the product (|x a| < 0.5 and t < -0.7) that term can pass the slack by up to 0.5 u, which only
            the other terms of the K-term sum cover: the CPU tests hold the emulated kernel to the bound at such scalars too.
            Zero padding stays zero exactly.
  tile sums against the kernel's OWN stored output y, n = 128 VB voxels per tile:
            |s1 - sum_tile y| <= n u sum_tile |y|,  |s2 - sum_tile y^2| <= (n + 1) u sum_tile y^2
            (any order of summation has fewer than n roundings per term; squaring adds one).
  delta     the constant-plus-sparse-delta form of the second convolution of a PVConv is a different decomposition of
            the same sum (a per-border-configuration constant formed in double, the MFMA loop on the difference): no derived
            bound is given for it.  It keeps the project's DELTA_RTOL = 1e-5 of max |ref|, the figure of
            test_hip_parity_gpu.py::test_conv3d_constant_plus_delta_matches_dense."""
import numpy as np
import torch

import pointwise_ref as pr
from pwconv_ref import _fma32, _swish_fast32, swish64

U32 = pr.U32
DELTA_RTOL = 1e-5


def ceil4(c):
    return (c + 3) // 4 * 4


def k_products(cin):
    return 27 * ceil4(cin)


# ---- the plan of the library, restated (conv_plan / launch_conv of csrc/conv3d.hip, csrc/conv3d_tiles.h) --------------

def conv_plan(r, cout, B, sparse):
    """(vb, cot, tiles): voxel blocks per wave, output channels per workgroup, spatial tiles; (0, 0, 0): unsupported"""
    r3 = r * r * r
    if not sparse and cout % 64 == 0 and r >= 16 and (r3 // 512) * (cout // 64) * B >= 512:
        return 4, 64, r3 // 512
    if cout % 64 == 0 and (r3 // 256) * (cout // 64) * B >= 512:
        return 2, 64, r3 // 256
    if cout % 32 == 0 and r >= 16 and not sparse:
        return 4, 32, r3 // 512
    if cout % 32 == 0 and r >= 16:
        return 2, 32, r3 // 256
    if cout % 32 == 0:
        return 1, 32, r3 // 128
    return 0, 0, 0


def tile_dims(r, vb):
    """(TD, TH, TW) of the spatial tile: 4 waves x vb blocks x 32 voxels, as wide as the grid"""
    if r == 32:
        return (2 if vb == 2 else 4), 4, 32
    if r == 16:
        return (4 if vb == 2 else 8), 4, 16
    return (4 if vb == 2 else 2), 8, r


# the ten launch_conv<COT>(TD, TH, TW) that the fp32 entry instantiates, as (r, vb, cot)
LAUNCH_TILES = {(32, 2, 64), (32, 4, 64), (16, 4, 64), (32, 4, 32), (32, 2, 32), (16, 2, 32), (16, 2, 64), (16, 4, 32),
                (8, 2, 64), (8, 1, 32)}

# name -> ((r, B, Cout, sparse), (vb, cot)): the smallest batch that reaches each tile, and the batches just under a threshold
PLAN_CASES = {
    "r32-vb4-cot64": ((32, 8, 64, False), (4, 64)),
    "r32-vb2-cot64": ((32, 4, 64, False), (2, 64)),
    "r32-vb2-cot64-sparse": ((32, 6, 64, True), (2, 64)),              # 768 items
    "r32-vb4-cot32": ((32, 2, 32, False), (4, 32)),
    "r32-vb4-cot32-under": ((32, 3, 64, False), (4, 32)),              # just under both thresholds, two channel tiles
    "r32-vb2-cot32-sparse": ((32, 2, 32, True), (2, 32)),
    "r16-vb4-cot64": ((16, 16, 256, False), (4, 64)),
    "r16-vb2-cot64": ((16, 16, 128, False), (2, 64)),
    "r16-vb2-cot64-sparse": ((16, 10, 256, True), (2, 64)),            # 640 items
    "r16-vb4-cot32": ((16, 2, 32, False), (4, 32)),
    "r16-vb2-cot32-sparse": ((16, 2, 32, True), (2, 32)),
    "r8-vb2-cot64": ((8, 32, 512, False), (2, 64)),
    "r8-vb1-cot32": ((8, 2, 32, False), (1, 32)),
    "r8-vb1-cot32-under": ((8, 31, 512, False), (1, 32)),              # just under the threshold, 16 channel tiles
}
DENSE_CASES = [k for k, v in PLAN_CASES.items() if not v[0][3]]
SPARSE_CASES = [k for k, v in PLAN_CASES.items() if v[0][3]]


# ---- float64 references and bounds ---------------------------------------------------------------------------------------

def _conv64(xin, w, bias):
    """F.conv3d (3x3x3, zero padding 1) of float64 operands, in batch chunks of at most 2^23 output elements"""
    B, cout = xin.shape[0], w.shape[0]
    n = max(1, (1 << 23) // (cout * xin[0, 0].numel()))
    return torch.cat([torch.nn.functional.conv3d(xin[lo:lo + n], w, bias, padding=1) for lo in range(0, B, n)])


def _col(v):
    return v.double()[:, :, None, None, None]


def operand64(x, pro):
    """(z, E_in): the convolution's input in float64 and the bound of the kernel's error on it (module docstring)"""
    x = x.double()
    if pro is None:
        return x, None
    xa = x * _col(pro[0])
    t = xa + _col(pro[1])
    z = swish64(t)
    return z, (t.abs() + 8.0) * U32 * z.abs() + 1e-35 + 1.1 * U32 * xa.abs()    # pointwise_ref.swish_bound(t) + 1.1 u |x a|


def conv64(x, w, bias=None, pro=None):
    """(ref, bound) f64[B, Cout, r, r, r] of y = conv(act(x), w) + bias for fp32 x [B, Cin, r, r, r], w [Cout, Cin, 3, 3, 3],
    pro = (A, Bs) f32[B, Cin] or None.  The two bound terms share |w|, so they are one convolution:
    conv64((K + 2) u |z| + E_in, |w|) + (K + 2) u |bias|."""
    z, e_in = operand64(x, pro)
    w = w.double()
    k = (k_products(w.shape[1]) + 2) * U32
    ref = _conv64(z, w, None if bias is None else bias.double())
    mag_in = k * z.abs()
    if e_in is not None:
        mag_in = mag_in + e_in
    bound = _conv64(mag_in, w.abs(), None if bias is None else k * bias.double().abs())
    return ref, bound


def tile_view(y, r, vb):
    """[B, C, r, r, r] -> [B, C, T, n]: the n = 128 vb voxels of each tile; tile index = d_tile * (r / TH) + h_tile"""
    td, th, tw = tile_dims(r, vb)
    assert tw == r
    B, C = y.shape[:2]
    v = y.reshape(B, C, r // td, td, r // th, th, r).permute(0, 1, 2, 4, 3, 5, 6)
    return v.reshape(B, C, (r // td) * (r // th), td * th * r)


def tile_stats64(y, r, vb):
    """(sums, bounds) f64[B, C, T, 2]: (sum y, sum y^2) per tile of the given output in float64, and what fp32 sums of those
    very numbers may differ by: n u sum |y| and (n + 1) u sum y^2"""
    v = tile_view(y.double(), r, vb)
    n = 128 * vb
    assert v.shape[-1] == n
    s2 = (v * v).sum(-1)
    return torch.stack([v.sum(-1), s2], -1), torch.stack([n * U32 * v.abs().sum(-1), (n + 1) * U32 * s2], -1)


def border_regions(r):
    """(name, index) of the 6 faces, 12 edges and 8 corners of [..., r, r, r]"""
    lo_hi = ((0, "lo"), (r - 1, "hi"))
    out = []
    for ax, an in enumerate("dhw"):
        for v, n in lo_hi:
            idx = [slice(None)] * 3
            idx[ax] = v
            out.append((f"face {an}={n}", (Ellipsis,) + tuple(idx)))
    for free, fn in enumerate("dhw"):
        a, b = [i for i in range(3) if i != free]
        for va, na in lo_hi:
            for vb_, nb in lo_hi:
                idx = [slice(None)] * 3
                idx[a], idx[b] = va, vb_
                out.append((f"edge along {fn} at {'dhw'[a]}={na} {'dhw'[b]}={nb}", (Ellipsis,) + tuple(idx)))
    for vd, nd in lo_hi:
        for vh, nh in lo_hi:
            for vw, nw in lo_hi:
                out.append((f"corner d={nd} h={nh} w={nw}", (Ellipsis, vd, vh, vw)))
    assert len(out) == 26
    return out


# ---- the kernel's arithmetic in fp32 numpy ---------------------------------------------------------------------------

F = np.float32


def emulate_conv32(x, w, bias, pro=None, reverse=False, fused_arg=False):
    """y f32[B, Cout, r, r, r] as conv3d_k3_kernel forms it: the input (behind the prologue: swish_fast of the fp32 argument,
    x*a+b as two roundings or, fused_arg, as one fma) zero padded; one fp32 accumulator per output, the products added in
    ascending order of (4-channel chunk, channel pair, tap, k) with one rounding each (v_mfma_f32_32x32x2_f32 is an fma per
    k); then + bias.  reverse: the same terms in the opposite order."""
    x, w = np.asarray(x, dtype=F), np.asarray(w, dtype=F)
    B, cin, r = x.shape[:3]
    cout = w.shape[0]
    if pro is not None:
        a, b = (np.asarray(p, dtype=F)[:, :, None, None, None] for p in pro)
        t = _fma32(x, np.broadcast_to(a, x.shape), np.broadcast_to(b, x.shape)) if fused_arg else ((x * a).astype(F) + b).astype(F)
        x = _swish_fast32(t)
    cp4 = ceil4(cin)
    xp = np.zeros((B, cp4, r + 2, r + 2, r + 2), F)
    xp[:, :cin, 1:-1, 1:-1, 1:-1] = x
    wp = np.zeros((cout, cp4, 3, 3, 3), F)
    wp[:, :cin] = w
    order = [(q * 4 + cp * 2 + k, tap) for q in range(cp4 // 4) for cp in range(2) for tap in range(27) for k in range(2)]
    if reverse:
        order.reverse()
    acc = np.zeros((B, cout, r, r, r), F)
    for c, tap in order:
        kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
        xs = xp[:, None, c, kd:kd + r, kh:kh + r, kw:kw + r]
        acc = _fma32(np.broadcast_to(wp[None, :, c, kd, kh, kw, None, None, None], acc.shape), np.broadcast_to(xs, acc.shape), acc)
    if bias is not None:
        acc = (acc + np.asarray(bias, dtype=F)[None, :, None, None, None]).astype(F)
    return acc


def emulate_tile_stats32(y, r, vb, reverse=False):
    """f32[B, C, T, 2]: the tile sums of an fp32 y by a serial fp32 chain over the tile's voxels (ascending or descending):
    the deepest nesting any order can have, n - 1 additions"""
    v = tile_view(torch.as_tensor(np.asarray(y, dtype=F)), r, vb).numpy()
    if reverse:
        v = v[..., ::-1]
    s1 = np.zeros(v.shape[:-1], F)
    s2 = np.zeros(v.shape[:-1], F)
    for i in range(v.shape[-1]):
        s1 = (s1 + v[..., i]).astype(F)
        s2 = (s2 + (v[..., i] * v[..., i]).astype(F)).astype(F)
    return np.stack([s1, s2], -1)
