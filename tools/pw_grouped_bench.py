"""First layer of the set-abstraction MLPs at B = 32: the materialised pair (group_points + 1x1 convolution) against the
gathered-operand call (fused_ops.pwconv_grouped_fused), per stage of the local prior (models/latent_points_ada_localprior.py::PVCNN2Prior.sa_blocks), each form
captured in one hipGraph and replayed as tools/pw_bench.py does.  Also the two halves of the pair on their own and a
bit-identity check of the two forms.  Prints one row per stage: a stage that did not gain would stay on the pair."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lion_amd import fused_ops as fo
from lion_amd.functional.ball_query import _ball_query_compute
from lion_amd.functional.sampling import _fps_compute


def t_us(f, n=20):
    """n calls captured in one hipGraph, replayed: kernel time without the python between launches"""
    for _ in range(3): f()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n): f()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5): g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (5 * n)


B = int(os.environ.get("PWG_BATCH", "32"))
# (name, points N, feature channels C, centres M, radius, neighbours U, Cout): real FPS centres and ball-query lists of a
# Gaussian cloud (the latent points of a sampling step), each stage on the previous stage's centres
# (PVCNN2Prior.sa_blocks + the 64 time-embedding channels from SA-1 on: first layers 35->32, 67->64, 131->128, 195->128)
STAGES = [("SA-0", 2048, 32, 1024, 0.1, 32, 32), ("SA-1", 1024, 64, 256, 0.2, 32, 64), ("SA-2", 256, 128, 64, 0.4, 32, 128),
          ("SA-3", 64, 192, 16, 0.8, 32, 128)]
print(f"B = {B}; us per call, hipGraph replay (20 calls x 5 replays)")
print(f"{'stage':5s} {'3+C->Cout':>10s} {'L':>6s} {'kernel':>6s} {'grouped MB':>10s} {'group':>7s} {'layer':>7s} {'pair':>7s} {'fused':>7s} {'saved':>7s} {'equal':>5s}")
torch.manual_seed(0)
coords = torch.randn(B, 3, STAGES[0][1], device="cuda") * float(os.environ.get("PWG_SIGMA", "0.5"))
with torch.no_grad():
    for name, N, C, M, radius, U, cout in STAGES:
        assert coords.shape[2] == N
        centers = _fps_compute(coords, M)
        idx = _ball_query_compute(centers, coords, radius, U)
        feat = torch.randn(B, C, N, device="cuda")
        conv = torch.nn.Conv2d(3 + C, cout, 1).cuda()
        gp = fo.GroupedPoints(coords, centers, feat, idx)
        L = M * U
        split = fo.pw_use_split(None, B, 3 + C, cout, L)
        x = gp.materialize()
        y0, s0 = fo.pwconv_fused(x, conv)
        y1, s1 = fo.pwconv_grouped_fused(gp, conv)
        same = torch.equal(y0, y1) and torch.equal(s0, s1)
        tg = t_us(lambda: gp.materialize())
        tl = t_us(lambda: fo.pwconv_fused(x, conv))
        tp = t_us(lambda: fo.pwconv_fused(gp.materialize(), conv))
        tf = t_us(lambda: fo.pwconv_grouped_fused(gp, conv))
        print(f"{name:5s} {3 + C:>5d}->{cout:<4d} {L:>6d} {'split' if split else 'fp32':>6s} {x.numel() * 4 / 1e6:>10.1f} {tg:>7.1f} {tl:>7.1f} "
              f"{tp:>7.1f} {tf:>7.1f} {tp - tf:>7.1f} {str(same):>5s}")
        coords = centers
