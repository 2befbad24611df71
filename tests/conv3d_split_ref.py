"""The plan, float64 reference, error bounds, numpy emulation and case table for the split-operand 3x3x3 convolution:
conv3d_split_pipe_kernel (r = 8, csrc/conv3d_split.hip) and conv3d_split_kernel<P = 2> (r = 16 / 32,
csrc/conv3d_split_kernel.h).  tests/test_conv3d_split_reference_cpu.py holds the emulation to the bounds and shows that
seeded defects leave them; tests/test_conv3d_split_numerics_gpu.py holds the kernels to them.  torch on any device;
imports nothing from lion_amd.

The arithmetic (csrc/split_ops.h).  Weights are scaled by one power of two per tensor, w^ = w 2^ew with max |w^| in
[2^13, 2^14); activations (behind the prologue) by one power of two per (workgroup tile, 16-channel chunk), x^ = z 2^E, E
running and monotone: max |x^| over the tile's halo in [2^13, 2^14) when E is chosen, and a chunk with a larger maximum
first multiplies the accumulators by the exact ratio.  Each scaled operand a is cut into a_h = fp16(a) and
a_l = fp16((a - a_h) 2048); three products per operand pair accumulate in fp32 inside v_mfma_f32_32x32x16_f16:
    acc += W_h X_h,  cor += W_h X_l + W_l X_h,  y = ((acc + cor / 2048) 2^-E) 2^-ew + bias.

Bounds, elementwise and derived -- none is a measured figure.  K = 27 Cin products per output, S = conv64(|z|, |w|).

  accumulation   ASSUMPTION: every product an MFMA adds to its fp32 accumulator costs one rounding of at most 2^-23
            relative to the running sum -- 2^-23 and not fp32's 2^-24 because the internal adder of v_mfma_f32_32x32x16_f16 is
            not documented as round-to-nearest (a truncating adder has a whole ulp).  The products themselves are exact
            (11 x 11 bits).  With the dot-product bound (Higham 3.1) acc carries gamma(K) S, gamma(n) = n 2^-23 / (1 - n 2^-23).
            cor sums 2 K products, each at most |w^||x^| (1 + 2^-11) (|a_l| <= |a| (1 + 2^-11) by the representation
            paragraph), and is divided by 2048: 2 K 2^-23 * 2 S / 2048 = K 2^-32 S, taken as K 2^-31 S to cover its second order.
            The sum acc + cor / 2048 and the bias add round once each (2^-24 each: plain fp32 additions), the two scalings
            are exact powers of two:
                |y - exact| <= gamma(K + 2 + K 2^-8) (S + |bias|).
  representation   for a scaled operand a with |a| < 2^14: a_h rounds to 11 bits, |a - a_h| <= 2^-11 |a| while a_h is a
            normal fp16 (|a| >= 2^-14), at most 2^-25 (half a subnormal step) below that.  The residual is an fp32 number
            (exact subtraction), times 2048 at most 2^14: a_l rounds IT to 11 bits, so
                d(a) = |a - a_h - a_l / 2048| <= 2^-22 |a|   while (a - a_h) 2048 is a normal fp16, at most 2^-36 below that,
            i.e. d(a) <= 2^-22 |a| + 2^-36 and |a_l| / 2048 <= (2^-11 |a| + 2^-25) (1 + 2^-11).  Then
                w^ x^ - (W_h X_h + (W_h X_l + W_l X_h) / 2048) = W_l X_l / 2^22 + d(w^) x^ + d(x^) (w^ - d(w^)):
            THREE terms of 2^-22 |w^||x^| each -- the integer is 3 -- times at most (1 + 2^-9) of second order:
                3 2^-22 (1 + 2^-9) S,
            plus what the absolute parts leave: per product at most 2 (2^-36 |x^| + 2^-36 |w^|) (once from d, once from the
            dropped product) and 2^-50, which is the floor term.
  floor     undoing the scales, 2^-36 of a scaled operand is f_w = 2^-36 2^-ew <= 2^-49 max |w| for a weight and
            f_x = 2^-36 2^-E <= 2^-49 m for an activation, m the fp32 maximum over the tile's halo that set the final E (E only
            falls along the K walk, so the final one is the coarsest).  In float64 terms m <= 2 M, M = max |z| over the tile
            and its one-voxel halo, all Cin channels, finite values only (the prologue's own error is far inside that factor
            of two): f_x <= 2^-48 M.  scale_exp clamps both exponents at 100, so neither step is ever below 2^-136.  Summed
            over the K products behind an output, with |x| <= M and |w| <= max |w|:
                2 K (f_w M + f_x max |w|),  f_w = max(2^-49 max |w|, 2^-136),  f_x = max(2^-48 M, 2^-136) (0 where M = 0):
            an absolute term of at most 6 K 2^-49 max |w| M per tile away from the clamp; the 2^-50 per product is below 2^-27 of
            it.  An operand 2^27 below its block's maximum leaves the normal range of the hi piece; the lo piece carries it
            down to 2^-36 / 2^13 = 2^-49 of the maximum, which is what this term charges.
  prologue  E_in of conv3d_ref.operand64, unchanged (the kernels share pro_act): + conv64(E_in, |w|), |z| in place of |x|.
  tile sums against the kernel's OWN stored output: conv3d_ref.tile_stats64 at vb = 2 -- n = 256 voxels, the split kernels' tile
            dimensions are conv3d_ref.tile_dims(r, 2) at every r, asserted below.
  delta     no derived bound, as in conv3d_ref: DELTA_RTOL of max |ref|, taken PER SAMPLE.

What the output bound cannot see.  It is a worst-case dot-product bound, linear in K, and the kernels sit at a few
thousandths of it.  A lost lo piece costs ~2^-12 per product with a random sign: outside the bound at Cin = 16 (K = 432), inside
it from Cin = 64 on (K 2^-23 = 2^-12.2).  The dynamic-range tests therefore also keep the project's older yardstick, max error <
5e-6 of max |ref| (test_conv_split_gpu.py), per sample: the emulation meets it at ~3e-7 and misses it 40-fold without the lo
piece (test_conv3d_split_reference_cpu.py).

Non-finite inputs stay out of the block maximum and reach the outputs of their 3x3x3 neighbourhood only; the bounds are
evaluated on the input with those voxels zeroed and hold outside the neighbourhoods."""
import numpy as np
import torch

import conv3d_ref as cr
from pwconv_ref import _swish_fast32

DELTA_RTOL = cr.DELTA_RTOL
KS = 16                        # input channels per chunk
UA = 2.0 ** -23                # per accumulated product (the assumption above)
REP = 3 * 2.0 ** -22 * (1 + 2.0 ** -9)


def gamma(n):
    return n * UA / (1.0 - n * UA)


def k_products(cin):
    return 27 * cin


# ---- the plan, restated (lion_conv3d_k3_split_forward, split_tile_forward, launch_split_t, launch_split_pipe) ------------

def split_plan(r, cin, cout, pro=False, stats=False, occ=False, tconst=False):
    """None where the entry point answers LION_EUNSUPPORTED, else a dict: kernel "pipe" | "tile", tile (TD, TH, TW), cb
    (32-channel blocks per workgroup), grid (dense launch, per sample), stat_tiles, chunks, and inst = (PRO, STATS), the
    instantiation that runs: launch_split_t sends statistics without a prologue to the PRO one when CB = 2 and Cin <= 256."""
    if r not in (8, 16, 32) or cin <= 0 or cin % KS or cout <= 0 or cout % 32 or (pro and cin > 256):
        return None
    if r == 8:
        if occ or tconst:
            return None
        return dict(kernel="pipe", tile=(4, 8, 8), cb=1, grid=(2, cout // 32), stat_tiles=2, chunks=cin // KS,
                    inst=(bool(pro), bool(stats)))
    cb = 2 if cout % 64 == 0 else 1
    tile = (4, 4, 16) if r == 16 else (2, 4, 32)
    pro_inst = bool(pro) or (bool(stats) and cb == 2 and cin <= 256)
    return dict(kernel="tile", tile=tile, cb=cb, grid=(r ** 3 // 256, cout // (32 * cb)), stat_tiles=r ** 3 // 256,
                chunks=cin // KS, inst=(pro_inst, bool(stats)))


for _r in (8, 16, 32):      # the tile sums reuse conv3d_ref.tile_view / tile_stats64 at vb = 2: the same tiles
    assert split_plan(_r, 16, 32)["tile"] == cr.tile_dims(_r, 2)
    assert split_plan(_r, 16, 32)["stat_tiles"] == _r ** 3 // 256 or _r == 8

VB = 2


def tile_stats64(y, r):
    return cr.tile_stats64(y, r, VB)


# ---- float64 reference and bound -----------------------------------------------------------------------------------------

def halo_max(z, r):
    """M f64[B, 1, r, r, r]: at every voxel, the largest finite |z| over all channels of its tile and the tile's one-voxel
    halo (tiles span w, so over every w)"""
    td, th, _ = cr.tile_dims(r, VB)
    a = torch.nan_to_num(z.abs(), nan=0.0, posinf=0.0, neginf=0.0).amax(dim=(1, 4))                     # [B, r(d), r(h)]
    a = torch.nn.functional.max_pool2d(a[:, None], 3, 1, 1)[:, 0]
    B = a.shape[0]
    t = a.reshape(B, r // td, td, r // th, th).amax(dim=(2, 4), keepdim=True)
    return t.expand(B, r // td, td, r // th, th).reshape(B, 1, r, r, 1).expand(B, 1, r, r, r)


def conv64(x, w, bias=None, pro=None):
    """(ref, bound) f64[B, Cout, r, r, r] for y = conv(act(x), w) + bias on the split kernels (module docstring):
    conv64((gamma + REP) |z| + E_in, |w|) + gamma |bias| + floor."""
    r = x.shape[-1]
    z, e_in = cr.operand64(x, pro)
    w = w.double()
    K = k_products(w.shape[1])
    g = gamma(K + 2 + K * 2.0 ** -8)
    ref = cr._conv64(z, w, None if bias is None else bias.double())
    mag_in = (g + REP) * z.abs()
    if e_in is not None:
        mag_in = mag_in + e_in
    bound = cr._conv64(mag_in, w.abs(), None if bias is None else g * bias.double().abs())
    wmax = float(w.abs().max())
    M = halo_max(z, r)
    f_w = max(2.0 ** -49 * wmax, 2.0 ** -136)
    f_x = torch.where(M > 0, torch.clamp(2.0 ** -48 * M, min=2.0 ** -136), torch.zeros_like(M))
    return ref, bound + 2 * K * (f_w * M + f_x * wmax)


def per_sample_max(ref):
    return ref.abs().flatten(1).amax(1).view(-1, 1, 1, 1, 1)


def per_sample_err(got, ref):
    """max over the samples of max |got - ref| / max |ref|, each over one sample: the measure of test_conv_split_gpu.py (held to
    5e-6 there), taken per sample"""
    return float(((got.double() - ref).abs().flatten(1).amax(1) / ref.abs().flatten(1).amax(1)).max())


# ---- the kernel's arithmetic in numpy ------------------------------------------------------------------------------------

F = np.float32
DEFECTS = ("no-rescale", "scale-not-monotone", "drop-lo-x", "drop-hi-chunk")


def scale_exp(m):
    """split_ops.h::scale_exp: e with 2^13 <= m 2^e < 2^14, clamped at 100"""
    return min(13 - (int(np.frexp(F(m))[1]) - 1), 100)


def cut(v):
    """split_ops.h::cut / cut2: hi = fp16(v), lo = fp16((v - hi) * 2048), round to nearest even"""
    v = v.astype(F)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(F)) * F(2048.0)).astype(np.float16)
    return hi.astype(F), lo.astype(F)


def pow2(e):
    return F(2.0 ** e)


def emulate_split(x, w, bias, pro=None, tile=(4, 8), defect=None):
    """y f32[B, Cout, r, r, r] as the split kernels form it, for any grid r and tile (TD, TH) x r that divides it -- the
    extension of test_split_numerics_cpu.py::split_gemm to the 3x3x3 case: one weight scale per tensor; one activation scale
    per (tile, 16-channel chunk) from the finite maximum over the tile's halo, monotone, the accumulators rescaled by the
    exact ratio when it falls; hi / lo cut; the three products of every tap accumulated in fp32 (the order inside an MFMA is
    not part of the claim: numpy's fp32 matrix product); epilogue ((acc + cor / 2048) 2^-E) 2^-ew + bias.
    defect: None, or one of DEFECTS --
      no-rescale           the accumulators stay as they are when the scale changes
      scale-not-monotone   every chunk takes its own maximum's scale, up as well as down (rescaling only downwards)
      drop-lo-x            the lo piece of the activations is dropped (cor += W_l X_h alone)
      drop-hi-chunk        the hi x hi product of chunk 1 (chunk 0 of a one-chunk walk) is dropped"""
    assert defect is None or defect in DEFECTS
    x, w = np.asarray(x, dtype=F), np.asarray(w, dtype=F)
    B, cin, r = x.shape[:3]
    cout = w.shape[0]
    td, th = tile
    assert cin % KS == 0 and r % td == 0 and r % th == 0
    if pro is not None:
        a, b = (np.asarray(p, dtype=F)[:, :, None, None, None] for p in pro)
        x = _swish_fast32(((x * a).astype(F) + b).astype(F))
    zp = np.zeros((B, cin, r + 2, r + 2, r + 2), F)
    zp[:, :, 1:-1, 1:-1, 1:-1] = x
    wmax = np.abs(w).max()
    ew = scale_exp(wmax) if wmax > 0 else 0
    wh, wl = cut(w.reshape(cout, cin, 27) * pow2(ew))
    nch = cin // KS
    bad_chunk = min(1, nch - 1)
    y = np.zeros((B, cout, r, r, r), F)
    n = td * th * r
    for b in range(B):
        for d0 in range(0, r, td):
            for h0 in range(0, r, th):
                halo = zp[b, :, d0:d0 + td + 2, h0:h0 + th + 2, :]
                acc, cor, E = np.zeros((cout, n), F), np.zeros((cout, n), F), 127
                for q in range(nch):
                    hc = halo[q * KS:(q + 1) * KS]
                    fin = np.abs(hc[np.isfinite(hc)])
                    m = fin.max() if fin.size else F(0)
                    if m > 0:
                        e = scale_exp(m)
                        if e < E or (defect == "scale-not-monotone" and e != E):
                            if E != 127 and e < E and defect != "no-rescale":
                                f = pow2(max(e - E, -126))
                                acc, cor = acc * f, cor * f
                            E = e
                    with np.errstate(invalid="ignore", over="ignore"):
                        xh, xl = cut(hc * (F(1) if E == 127 else pow2(E)))
                        if defect == "drop-lo-x":
                            xl = np.zeros_like(xl)
                        for tap in range(27):
                            kd, kh, kw = tap // 9, (tap // 3) % 3, tap % 3
                            sh = xh[:, kd:kd + td, kh:kh + th, kw:kw + r].reshape(KS, n)
                            sl = xl[:, kd:kd + td, kh:kh + th, kw:kw + r].reshape(KS, n)
                            whq, wlq = wh[:, q * KS:(q + 1) * KS, tap], wl[:, q * KS:(q + 1) * KS, tap]
                            if not (defect == "drop-hi-chunk" and q == bad_chunk):
                                acc = (acc + whq @ sh).astype(F)
                            cor = (cor + (whq @ sl).astype(F)).astype(F)
                            cor = (cor + (wlq @ sh).astype(F)).astype(F)
                with np.errstate(invalid="ignore", over="ignore"):
                    o = ((acc + cor * F(1.0 / 2048.0)).astype(F) * (F(1) if E == 127 else pow2(-E))).astype(F) * pow2(-ew)
                    if bias is not None:
                        o = (o.astype(F) + np.asarray(bias, dtype=F)[:, None]).astype(F)
                y[b, :, d0:d0 + td, h0:h0 + th, :] = o.reshape(cout, td, th, r)
    return y


# ---- dynamic-range cases -------------------------------------------------------------------------------------------------

RANGE_CASES = ("nine-decades", "beyond-fp16-max", "tiny", "per-sample-scales", "huge-one-chunk", "tiny-weights",
               "huge-weights", "residual-bits", "rising", "falling")
SAMPLE_SCALES = (1e-6, 3e7, 1.0, 1e4)


def range_case(case, x, w, bias, gen):
    """(x, w, bias) of a dynamic-range case from normal x [B, Cin, r, r, r] and a Conv3d's default w, bias: the eight cases of
    test_conv_split_gpu.py::test_split_adversarial_dynamic_range (huge-one-chunk: the chunk at Cin / 2 times 1e4, chunk 0 times
    1e-3; per-sample-scales: the first B of SAMPLE_SCALES; tiny: the bias times 1e-30 as well) and
      rising    chunk q times 2^(7 q): the maximum grows at every chunk, so the rescale runs at every chunk;
      falling   chunk q times 2^(-7 q): no rescale, the later chunks sit ever deeper under the maximum.
    gen: a torch.Generator on x's device."""
    assert case in RANGE_CASES
    B, cin = x.shape[:2]
    dev = x.device
    x, w, bias = x.clone(), w.clone(), bias.clone()
    sign = lambda: torch.where(torch.rand(x.shape, device=dev, generator=gen) < 0.5, -1.0, 1.0)
    if case == "nine-decades":
        lo, hi = float(np.log(1e-6)), float(np.log(1e4))
        x = torch.exp(torch.empty(x.shape, device=dev).uniform_(lo, hi, generator=gen)) * sign()
    elif case == "beyond-fp16-max":
        x = x * 3.0e6
    elif case == "tiny":          # the bias goes down with it: next to a bias of normal size the whole sum is below its rounding
        x, bias = x * 1e-30, bias * 1e-30
    elif case == "per-sample-scales":
        x = x * torch.tensor(SAMPLE_SCALES[:B], device=dev).view(B, 1, 1, 1, 1)
    elif case == "huge-one-chunk":
        c = cin // 2
        x[:, c:c + KS] *= 1e4
        x[:, :KS] *= 1e-3
    elif case == "tiny-weights":
        w, bias = w * 1e-9, bias * 1e-9
    elif case == "huge-weights":
        w = w * 1e6
    elif case == "residual-bits":
        k = torch.randint(-2048, 2048, x.shape, device=dev, generator=gen).float()
        x = (1.0 + k * 2.0 ** -22) * sign()
    else:
        q = torch.arange(cin, device=dev) // KS
        f = torch.pow(2.0, 7.0 * q) if case == "rising" else torch.pow(2.0, -7.0 * q)
        x = x * f.view(1, cin, 1, 1, 1)
    return x.contiguous(), w.contiguous(), bias.contiguous()


def chunk_exponents(x, r):
    """[B, T, chunks] int: scale_exp of each (tile, chunk) halo maximum of a finite fp32 x -- what the running scale walks
    through (100 where the chunk's halo is all zero)"""
    B, cin = x.shape[:2]
    out = []
    for q in range(cin // KS):
        m = halo_max(x[:, q * KS:(q + 1) * KS].double(), r)
        t = cr.tile_view(m, r, VB)[:, 0, :, 0]
        e = 13 - torch.floor(torch.log2(t.clamp(min=1e-300)))
        out.append(torch.where(t > 0, e.clamp(max=100), torch.full_like(e, 100)))
    return torch.stack(out, -1).long()


def rescales(x, r):
    """number of accumulator rescales the K walk makes, summed over tiles: a chunk whose exponent is below the running one"""
    e = chunk_exponents(x, r)
    run = torch.cummin(e, -1).values
    return int((e[..., 1:] < run[..., :-1]).sum())


# ---- the case tables -----------------------------------------------------------------------------------------------------

# A. dense, four forms at Cin = 48 (three chunks): name -> ((r, B, Cin, Cout), (kernel, cb, channel tiles))
DENSE_CASES = {
    "r8-pipe": ((8, 2, 48, 32), ("pipe", 1, 1)),
    "r16-cb1": ((16, 2, 48, 32), ("tile", 1, 1)),
    "r16-cb2": ((16, 2, 48, 64), ("tile", 2, 1)),
    "r32-cb1": ((32, 2, 48, 32), ("tile", 1, 1)),
    "r32-cb2": ((32, 2, 48, 64), ("tile", 2, 1)),
    "r16-cb1-three-channel-tiles": ((16, 2, 48, 96), ("tile", 1, 3)),
}
# B. the edges of Cin, four forms: one chunk (`more` never true, the weight ring filled once) and two chunks
CIN_FOUR_FORMS = {
    "r8-one-chunk": ((8, 2, 16, 32), ("pipe", 1, 1)),
    "r8-two-chunks": ((8, 2, 32, 32), ("pipe", 1, 1)),
    "r16-cb2-one-chunk": ((16, 2, 16, 64), ("tile", 2, 1)),
    "r16-cb2-two-chunks": ((16, 2, 32, 64), ("tile", 2, 1)),
}
# single forms: name -> ((r, B, Cin, Cout), pro, stats, inst): the instantiation (PRO, STATS) the name is about
CIN_SINGLE_FORMS = {
    "r8-prologue-table-maximum": ((8, 2, 256, 32), True, True, (True, True)),
    "r16-cb1-prologue-table-maximum": ((16, 2, 256, 32), True, True, (True, True)),
    "r16-cb2-sums-without-prologue-272": ((16, 1, 272, 64), False, True, (False, True)),   # the real <false, true>
    "r8-plain-272": ((8, 2, 272, 32), False, False, (False, False)),
}
REFUSED = {"r8-prologue-272": (8, 2, 272, 32), "r16-prologue-272": (16, 2, 272, 32)}
# C. dynamic range: name -> (r, B, Cin, Cout); rising / falling run at Cin = 64 on both
RANGE_SHAPES = {"r8": (8, 2, 64, 32), "r32-cb1": (32, 1, 32, 32)}
RANGE_SHAPES_64 = {"r8": (8, 2, 64, 32), "r32-cb1": (32, 1, 64, 32)}


def range_shape(shape, case):
    return (RANGE_SHAPES_64 if case in ("rising", "falling") else RANGE_SHAPES)[shape]


# D. hand-built clouds: the voxels of sample 0; sample 1 holds the point reflection v -> r - 1 - v
CLOUDS = ("origin", "far-corner", "interior", "last-d-row", "single-bit", "full")
SPARSE_SHAPES = ((16, 32), (16, 64), (32, 32), (32, 64))     # (r, channels): c -> c, B = 2
LEVELS = (0, 1, 2)


def cloud_voxels(kind, r):
    """[(d, h, w)] of sample 0, or None for the full grid.
    r = 16: tiles of (4, 4, 16), 4 x 4 of them; r = 32: tiles of (2, 4, 32), 16 x 8 of them.
      interior     the middle of tile (1, 1) at r = 16, of tile (7, 3) at r = 32: empty tiles without a reader on the low face,
                   in the interior and on the high face, in d and in h
      last-d-row   on the last d-row of its tile: the halo reaches into the next tile in d
      single-bit   r = 16: first d-row of tile (2, 1) -> tile (1, 1) runs wave 3 alone; r = 32: last d-row, last h-row of
                   tile (5, 2) -> tile (6, 2) runs wave 1 alone"""
    assert kind in CLOUDS and r in (16, 32)
    if kind == "full":
        return None
    return {"origin": [(0, 0, 0)], "far-corner": [(r - 1, r - 1, r - 1)],
            "interior": [(5, 5, 7)] if r == 16 else [(14, 13, 17)],
            "last-d-row": [(7, 9, 3)] if r == 16 else [(9, 18, 30)],
            "single-bit": [(8, 5, 11)] if r == 16 else [(11, 11, 4)]}[kind]


def cloud_counts(kind, r, B=2):
    """int32 [B, r^3] point counts: sample 0 the named voxels (count 1 + index), odd samples the reflected ones"""
    cnt = torch.zeros(B, r, r, r, dtype=torch.int32)
    vox = cloud_voxels(kind, r)
    if vox is None:
        cnt[:] = 1
    else:
        for b in range(B):
            for i, (d, h, w) in enumerate(vox):
                p = (d, h, w) if b % 2 == 0 else (r - 1 - d, r - 1 - h, r - 1 - w)
                cnt[(b,) + p] = 1 + i
    return cnt.reshape(B, r ** 3)


def tile_flags(cnt, r, level):
    """what lion_conv3d_tile_occupancy_aware leaves in the flag words (conv_tile_occ_kernel of csrc/conv3d.hip), from a
    max-pool dilation of the count grid: dict of [B, T] tensors --
      mask1, mask2   4-bit wave masks at margin 1 / 2: bit w = wave w's 64-voxel block (64 / r rows of one d-plane) has a point
                     within the margin in d and h (tiles span w)
      word1, word2   the whole flag words: mask | reader << 8 | (margin-2 words: occupied at margin 1) << 9
      stored1, stored2   the tile's output is written by the conv on the voxelised grid / by the delta conv at this level"""
    B = cnt.shape[0]
    td, th, _ = cr.tile_dims(r, VB)
    rw = 64 // r
    g = (cnt.reshape(B, r, r, r) > 0).any(-1).float()[:, None]
    out = {}
    for m in (1, 2):
        d = torch.nn.functional.max_pool2d(g, 2 * m + 1, 1, m)[:, 0]
        bits = d.reshape(B, r // td, td, r // th, th // rw, rw).amax(-1).permute(0, 1, 3, 2, 4).reshape(B, -1, 4).long()
        out[f"mask{m}"] = (bits << torch.arange(4)).sum(-1)
    occ1, occ2 = out["mask1"] != 0, out["mask2"] != 0
    grid2 = occ2.reshape(B, 1, r // td, r // th).float()
    near = torch.nn.functional.max_pool2d(grid2, 3, 1, 1).reshape(B, -1) > 0
    need1 = torch.zeros_like(near) if level == 2 else near
    out["word1"] = out["mask1"] | (need1.long() << 8)
    out["word2"] = out["mask2"] | (occ2.long() << 8) | (occ1.long() << 9)
    out["stored1"] = torch.ones_like(occ1) if level == 0 else out["word1"] != 0
    out["stored2"] = torch.ones_like(occ2) if level == 0 else out["word2"] != 0
    return out


def tile_kinds(r):
    """[T] strings: the position of each tile on the d and h axes, 'lo' | 'in' | 'hi' each (the closed-form sums of an unstored
    tile count the voxels of the 27 border configurations from these)"""
    td, th, _ = cr.tile_dims(r, VB)
    pos = lambda i, n: "lo" if i == 0 else "hi" if i == n - 1 else "in"
    return [pos(dt, r // td) + "-" + pos(ht, r // th) for dt in range(r // td) for ht in range(r // th)]


def tiles_to_voxels(mask, r):
    """[B, T] bool -> [B, 1, r, r, r] bool"""
    td, th, _ = cr.tile_dims(r, VB)
    B = mask.shape[0]
    m = mask.reshape(B, r // td, 1, r // th, 1, 1).expand(B, r // td, td, r // th, th, r)
    return m.reshape(B, 1, r, r, r)
