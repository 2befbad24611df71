"""What the match-free EMD loss costs or saves: forward + backward of

  (a)  lion_amd.emd.emd_loss(pred, target).sum()                     -- lion_emd_loss_forward (23 launches, nothing of size
                                                                        N*M in memory), lion_emd_loss_backward (one launch)
  (b)  (EarthMoverDistanceFunction.apply(pred, target) / N).sum()    -- the composition it replaces: lion_emd_approxmatch (the
                                                                        [B,M,N] match matrix rewritten at each of 10 levels),
                                                                        lion_emd_matchcost, lion_emd_matchcost_backward

alternating in one process, device events around windows of --iters iterations, --windows windows each, after a warm-up,
driven from the host (at milliseconds per iteration the launch overhead does not show).  (a) is timed twice: with the
prediction's gradient only (what the VAE asks for) and with both gradients, which (b) always computes.  Peak device memory
above the inputs (torch.cuda.max_memory_allocated) is taken over one iteration of each afterwards.

  python tools/bench_emd_loss.py [--batch 32] [--points 2048] [--iters 50] [--windows 5] [--out profiles/emd_loss_bench.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emd_loss_bench.txt"))
    args = ap.parse_args()

    import torch
    from lion_amd.emd import EarthMoverDistanceFunction, emd_loss
    assert torch.cuda.is_available(), "this is a GPU measurement: no device, no number"
    B, N = args.batch, args.points
    gen = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.rand(B, N, 3, device="cuda", generator=gen).requires_grad_()
    target = torch.rand(B, N, 3, device="cuda", generator=gen)
    target_g = target.clone().requires_grad_()

    def loss_op(t):
        def step():
            pred.grad = t.grad = None
            emd_loss(pred, t).sum().backward()
        return step

    def composition():
        pred.grad = target_g.grad = None
        (EarthMoverDistanceFunction.apply(pred, target_g) / float(N)).sum().backward()

    paths = [("(a) emd_loss, prediction's gradient", loss_op(target)),
             ("(a) emd_loss, both gradients", loss_op(target_g)),
             ("(b) EarthMoverDistanceFunction / N", composition)]
    for _, fn in paths:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in paths}
    for _ in range(args.windows):
        for name, fn in paths:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.iters)

    peaks = {}
    for name, fn in paths:
        pred.grad = target_g.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base

    # agreement of the two at this size: the same auction; the sums differ by their order, the target's gradient by one
    # rounding per weight.  Uniform clouds at this size are not certified as well conditioned: reported, not asserted.
    pred.grad = target_g.grad = None
    la = emd_loss(pred, target_g)
    la.sum().backward()
    ga, gta = pred.grad.clone(), target_g.grad.clone()
    pred.grad = target_g.grad = None
    lb = EarthMoverDistanceFunction.apply(pred, target_g) / float(N)
    lb.sum().backward()
    rel_loss = ((la - lb).abs() / lb.abs()).max().item()
    rel_g1 = ((ga - pred.grad).abs().max() / pred.grad.abs().max()).item()
    rel_g2 = ((gta - target_g.grad).abs().max() / target_g.grad.abs().max()).item()

    lines = [f"tools/bench_emd_loss.py on {torch.cuda.get_device_name(0)}: B = {B}, N = M = {N}, uniform clouds, forward + backward, "
             f"device events, {args.windows} alternating windows of {args.iters} iterations (host-driven)"]
    for name, _ in paths:
        t = times[name]
        lines.append(f"{name}: median {statistics.median(t):.1f} us per iteration, {min(t):.1f} - {max(t):.1f} "
                     f"(windows: {', '.join('%.1f' % v for v in t)}); peak memory above the inputs {peaks[name] / 2 ** 20:.1f} MiB")
    med = {name: statistics.median(times[name]) for name, _ in paths}
    comp = med[paths[2][0]]
    lines.append(f"median window, composition / op: {comp / med[paths[0][0]]:.2f} x (prediction's gradient), "
                 f"{comp / med[paths[1][0]]:.2f} x (both gradients)")
    lines.append(f"agreement at this size: loss max relative difference {rel_loss:.2e}, gradients {rel_g1:.2e} (prediction) / "
                 f"{rel_g2:.2e} (target) of their largest entry")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
