"""A/B of the voxel-convolution precisions (conv_ops.PRECISION: "fp32" = three-product split kernel, "half" = single-product
kernel, csrc/conv3d_half.hip), HIP events, B = 32:
  * the kernel at 64->64 @ 32^3 and 128->128 @ 16^3 -- dense plain call, and the two in-step forms on a surface-like cloud
    (conv1: work queue + occupancy masks + tile sums; conv2: AdaGN+Swish prologue, constant + delta, tile sums);
  * ms per step of the product sampler (generate_samples_vada_2prior, graphed chains) on its own chain and on forced clouds
    (bench.py's ForcedClouds).
On a tree without the mode (the parent commit) only the fp32 columns are measured: run it in both trees on one box.
usage: python tools/conv_half_bench.py [--steps 100] [--reps 3] [--no-step]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lion_amd import conv_ops, fused_ops  # noqa: E402

HAVE_HALF = hasattr(conv_ops, "conv_precision")
PRECISIONS = ["fp32", "half"] if HAVE_HALF else ["fp32"]


def precision(p):
    import contextlib
    return conv_ops.conv_precision(p) if HAVE_HALF else contextlib.nullcontext()


def us(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def sphere_counts(B, r, dev):
    """point counts [B, r^3] of 2048 points on a sphere per sample (the clouds a trained chain visits late)"""
    g = torch.Generator(device=dev).manual_seed(0)
    v = torch.randn(B, 2048, 3, device=dev, generator=g)
    v = v / v.norm(dim=2, keepdim=True)
    idx = ((v * 0.45 + 0.5) * r).long().clamp(0, r - 1)
    flat = (idx[..., 0] * r + idx[..., 1]) * r + idx[..., 2]
    counts = torch.zeros(B, r ** 3, dtype=torch.int32, device=dev)
    counts.scatter_add_(1, flat, torch.ones_like(flat, dtype=torch.int32))
    return counts


def kernel_table(B):
    dev = "cuda"
    print(f"kernel, B = {B}, us per launch (median of 3 x 20 launches)")
    print(f"{'shape':18s} {'form':14s} " + " ".join(f"{p:>9s}" for p in PRECISIONS))
    for cin, r in ((64, 32), (128, 16)):
        cout = cin
        torch.manual_seed(cin)
        conv1 = torch.nn.Conv3d(cin, cout, 3, padding=1).to(dev)
        conv2 = torch.nn.Conv3d(cout, cout, 3, padding=1).to(dev)
        x = torch.randn(B, cin, r, r, r, device=dev)
        counts = sphere_counts(B, r, dev)
        grid = (x * (counts > 0).view(B, 1, r, r, r)).contiguous()
        A = torch.rand(B, cout, device=dev) + 0.5
        Bs = torch.randn(B, cout, device=dev) * 0.5
        rows = {"dense": [], "in-step conv1": [], "in-step conv2": []}
        with torch.no_grad():
            occ1, occ2 = fused_ops.conv3d_occupancy(counts, r, cout, B, consumer_aware=2)
            y1, _ = fused_ops.conv3d_fused(grid, conv1, None, True, fused_ops.conv3d_occupancy(counts, r, cout, B)[0], split=True)
            for p in PRECISIONS:
                with precision(p):
                    med = lambda fn: sorted(us(fn) for _ in range(3))[1]
                    rows["dense"].append(med(lambda: conv_ops.conv3d_k3(x, conv1.weight, conv1.bias, split=True)))
                    rows["in-step conv1"].append(med(lambda: fused_ops.conv3d_fused(grid, conv1, None, True, occ1, split=True)))
                    rows["in-step conv2"].append(med(lambda: fused_ops.conv3d_fused(y1, conv2, (A, Bs), True, occ2,
                                                                                   prev_conv=conv1, split=True)))
        for form, vals in rows.items():
            print(f"{cin:3d}->{cout:3d} @ {r:2d}^3   {form:14s} " + " ".join(f"{v:9.1f}" for v in vals))


def step_table(B, K, reps):
    import bench
    from lion_amd.config import released_prior_cfg
    from lion_amd.sampling import generate_samples_vada_2prior
    dev = torch.device("cuda")
    lion = bench.build_models(released_prior_cfg("airplane"), dev)
    d, shapes = lion.diffusion, lion.vae.latent_shape()

    def sample(p, hook=None):
        torch.manual_seed(1234)
        kw = {"conv_precision": p} if HAVE_HALF else {}
        return generate_samples_vada_2prior(shapes, lion.priors, d, lion.vae, B, ddim_step=K, state_hook=hook, **kw)

    def timed(p, hook=None):
        sample(p, hook)                       # captures (or re-captures after a precision change) and warms up
        runs = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sample(p, hook)
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
        return sorted(runs)

    with torch.no_grad():
        eps = [torch.randn([B] + shapes[0], device=dev), torch.randn([B] + shapes[1], device=dev)]
        lion.vae.sample(num_samples=B, decomposed_eps=eps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lion.vae.sample(num_samples=B, decomposed_eps=eps)
        torch.cuda.synchronize()
        decode = time.perf_counter() - t0
        print(f"sampler, B = {B}, {K} DDIM steps per prior, ms per step = (call - decode) / steps, decode {decode * 1e3:.1f} ms;"
              f" median [min .. max] of {reps} calls")
        for p in PRECISIONS:
            own = timed(p)
            forced = timed(p, bench.ForcedClouds(d, B, dev, K, force=True))
            f = lambda runs: " ".join(f"{(t - decode) / K * 1e3:.3f}" for t in (runs[len(runs) // 2], runs[0], runs[-1]))
            print(f"{p:5s} own chain     ms per step: {f(own)}")
            print(f"{p:5s} forced clouds ms per step: {f(forced)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    print(f"tree: {ROOT}  half mode available: {HAVE_HALF}")
    kernel_table(a.batch)
    if not a.no_step:
        step_table(a.batch, a.steps, a.reps)
