"""What the atomic-free Chamfer loss costs or saves: forward + backward of

  (a)  lion_amd.chamfer3d.chamfer_loss(pred, target, "mean").sum()           -- lion_chamfer_forward, lion_chamfer_loss_reduce,
                                                                                lion_chamfer_loss_backward (gather form)
  (b)  d1, d2 = chamfer_3DDist()(pred, target); (d1.mean(1) + d2.mean(1)).sum()  -- the composition it replaces: the same
                                                                                forward launch, two ATen means and an add,
                                                                                autograd through them, lion_chamfer_backward
                                                                                (four launches, float atomics)

alternating in one process, device events around windows of --iters iterations, --windows windows each, after a warm-up;
first driven from the host (launch and autograd overhead included), then each captured once and replayed as a hipGraph.
(a) is timed twice: with the prediction's gradient only (what the VAE asks for: the target's direction is not launched) and
with both gradients, which (b) always computes.  Kernel launches per iteration are counted afterwards with torch.profiler.

  python tools/bench_chamfer_loss.py [--batch 32] [--points 2048] [--iters 200] [--windows 3] [--out profiles/chamfer_loss_bench.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer_loss_bench.txt"))
    args = ap.parse_args()

    import torch
    from lion_amd.chamfer3d import chamfer_3DDist, chamfer_loss
    assert torch.cuda.is_available(), "this is a GPU measurement: no device, no number"
    B, N = args.batch, args.points
    gen = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.rand(B, N, 3, device="cuda", generator=gen).requires_grad_()
    target = torch.rand(B, N, 3, device="cuda", generator=gen)
    target_g = target.clone().requires_grad_()
    dist = chamfer_3DDist()

    def loss_op(t):
        def step():
            pred.grad = t.grad = None
            chamfer_loss(pred, t, "mean").sum().backward()
        return step

    def composition():
        pred.grad = None
        d1, d2, _, _ = dist(pred, target)
        (d1.mean(1) + d2.mean(1)).sum().backward()

    paths = [("(a) chamfer_loss, prediction's gradient", loss_op(target)),
             ("(a) chamfer_loss, both gradients", loss_op(target_g)),
             ("(b) chamfer_3DDist + means + autograd", composition)]
    for _, fn in paths:
        for _ in range(20):
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

    # the same three as hipGraph replays: device time without the host's launch and autograd overhead
    graphed = {}
    for name, fn in paths:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphed[name] = g
        for _ in range(20):
            g.replay()
    torch.cuda.synchronize()
    gtimes = {name: [] for name, _ in paths}
    for _ in range(args.windows):
        for name, _ in paths:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                graphed[name].replay()
            b.record()
            b.synchronize()
            gtimes[name].append(a.elapsed_time(b) * 1e3 / args.iters)
    del graphed

    # agreement of the two at this size (same arg-mins; the sums differ by their order only)
    pred.grad = None
    la = chamfer_loss(pred, target, "mean")
    la.sum().backward()
    ga = pred.grad.clone()
    pred.grad = None
    d1, d2, _, _ = dist(pred, target)
    lb = d1.mean(1) + d2.mean(1)
    lb.sum().backward()
    rel_loss = ((la - lb).abs() / lb.abs()).max().item()
    rel_grad = ((ga - pred.grad).abs().max() / pred.grad.abs().max()).item()

    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        for name, fn in paths:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                  and not e.name.lower().startswith(("memcpy", "memset"))]
            ours = sum("chamfer" in e.name for e in ev)
            launches[name] = f"{len(ev)} kernel launches per iteration ({ours} of this library, {len(ev) - ours} ATen)"
    except Exception as e:      # the count is a by-product; the times above stand without it
        launches = {name: f"launches not counted ({type(e).__name__}: {e})" for name, _ in paths}

    lines = [f"tools/bench_chamfer_loss.py on {torch.cuda.get_device_name(0)}: B = {B}, N = M = {N}, uniform clouds, forward + backward, "
             f"device events, {args.windows} alternating windows of {args.iters} iterations (host-driven: launch overhead included)"]
    for name, _ in paths:
        t = times[name]
        lines.append(f"{name}: {min(t):.1f} - {max(t):.1f} us per iteration (windows: {', '.join('%.1f' % v for v in t)}); {launches[name]}")
        t = gtimes[name]
        lines.append(f"    as a hipGraph replay: {min(t):.1f} - {max(t):.1f} us (windows: {', '.join('%.1f' % v for v in t)})")
    lines.append(f"agreement at this size: loss max relative difference {rel_loss:.2e}, prediction's gradient {rel_grad:.2e} of its largest entry")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
