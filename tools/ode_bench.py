"""Measurements of the probability-flow ODE sampler (lion_amd/ode.py, csrc/ode.hip) for the global
and the local prior of the released airplane config (random weights from torch.manual_seed(0): no trained checkpoint is
shipped, so nfe is that of an untrained flow).

  python tools/ode_bench.py [--batch 32] [--tol 1e-5] [--evals 30] [--no-host-loop] [--out FILE]
      per prior: ms per function evaluation, graphed (lion_ode_stage + replay of [forward -> drift]) and eager; ms per
      replayed DDIM chain step of the same prior (the issue's yardstick); nfe, attempted steps and wall time of one graphed
      sample_model_ode from 1 to 1e-5; the same solve through scipy's solve_ivp driving the eager model on the host, as the
      reference does (device -> host -> device per evaluation).
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ode -- python tools/ode_bench.py --trace-run PRIOR
      one capture solve, then one graphed solve of PRIOR (global | local) -- for the kernel trace
  python tools/ode_bench.py --share DIR [--attempts 8]
      from that trace: over the last ATTEMPTS attempted steps, the solver kernels' share of the summed kernel time and the
      ATen kernels launched (must be none)
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SOLVER = re.compile(r"::(stage|drift|partials|control)_kernel\(")


def setup(B):
    import torch
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion_continuous import make_diffusion
    from lion_amd.models.lion import LION
    torch.manual_seed(0)
    cfg = released_prior_cfg()
    lion = LION(cfg)
    lion.priors.eval()
    lion.vae.eval()
    diff = make_diffusion(cfg.sde, device="cuda")
    shapes = lion.vae.latent_shape()
    g = torch.Generator(device="cuda").manual_seed(1)
    zs = [torch.randn([B] + s, device="cuda", generator=g) for s in shapes]
    with torch.no_grad():
        cond = lion.vae.global2style(torch.randn([B] + shapes[0], device="cuda", generator=g))
    return {"global": (lion.priors[0], shapes[0], zs[0], None), "local": (lion.priors[1], shapes[1], zs[1], cond)}, diff


def ms_per(fn, n):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def host_loop(model, shape, z, cond, diff, tol):
    """the reference's path: solve_ivp(RK45) on the host, every evaluation a device round trip of the eager model"""
    import numpy as np
    import torch
    from scipy.integrate import solve_ivp
    B = z.shape[0]
    t0, tb, sign = diff.ode_span(1.0, 1e-5)

    def fun(t, y):
        tt = torch.tensor(t).to("cuda", torch.float32) * sign
        x = torch.tensor(y).to("cuda", torch.float32).reshape([B] + list(shape))
        with torch.no_grad():
            eps = model(x=x, t=tt.view(1).expand(B), condition_input=cond, clip_feat=None)
            dx = diff.f(tt) * x + 0.5 * diff.g2(tt) * eps / torch.sqrt(diff.var(tt))
        return (sign * dx).cpu().numpy().reshape(-1)
    tic = time.perf_counter()
    sol = solve_ivp(fun, (t0, tb), z.double().cpu().numpy().reshape(-1), method="RK45", rtol=tol, atol=tol,
                    t_eval=[t0, tb])
    return sol.nfev, time.perf_counter() - tic, sol.status


def bench(args):
    import torch
    from lion_amd import chain as _chain
    from lion_amd import ode
    priors, diff = setup(args.batch)
    sched = diff.ode_scalars()
    t0, tb, sign = diff.ode_span(1.0, 1e-5)
    lines = []
    for name, (model, shape, z, cond) in priors.items():
        B = z.shape[0]
        with torch.no_grad():
            g = ode.graph_for(model, B, shape, cond, None, z.device, sched)
            if g.cond is not None:
                g.cond.copy_(cond)
            g.state.reset(z, t0, tb, args.tol, args.tol, sign)      # stage f0 repeated: drift does not advance it
            graphed = ms_per(g.evaluate, args.evals)
            st = ode.OdeState(z.numel(), B, z.device)
            st.reset(z, t0, tb, args.tol, args.tol, sign)
            eager = ms_per(ode.eager_evaluator(st, model, shape, sched, cond), args.evals)
            ch = _chain.GraphedChain(model, B, shape, cond, None, z.device, _chain.DDIM, 64)
            ch.x.copy_(z)
            ddim = ms_per(ch.replay, args.evals)
            del ch
            diff.sample_model_ode(model, B, shape, 1e-5, 1e-2, False, 1.0, noise=z, condition_input=cond)  # captured
            x, nfe, secs = diff.sample_model_ode(model, B, shape, 1e-5, args.tol, False, 1.0, noise=z,
                                                 condition_input=cond)
        c = diff.last_ode
        rec = {"prior": name, "batch": B, "tol": args.tol, "ms_per_eval_graphed": round(graphed, 4),
               "ms_per_eval_eager": round(eager, 4), "ms_per_ddim_chain_step": round(ddim, 4),
               "graphed_eval_over_ddim_step": round(graphed / ddim, 4), "nfe": nfe,
               "attempted_steps": c["n_accepted"] + c["n_rejected"], "rejected": c["n_rejected"],
               "host_syncs": c["n_accepted"] + c["n_rejected"] + 1, "solve_s": round(secs, 4),
               "finite": bool(torch.isfinite(x).all())}
        if not args.no_host_loop:
            hn, hs, status = host_loop(model, shape, z, cond, diff, args.tol)
            rec.update({"host_loop_nfe": hn, "host_loop_s": round(hs, 4), "host_loop_status": status,
                        "speedup_vs_host_loop": round(hs / secs, 3)})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


def trace_run(args):
    import torch
    priors, diff = setup(args.batch)
    model, shape, z, cond = priors[args.trace_run]
    B = z.shape[0]
    diff.sample_model_ode(model, B, shape, 1e-5, 1e-2, False, 1.0, noise=z, condition_input=cond)   # capture
    torch.cuda.synchronize()
    x, nfe, secs = diff.sample_model_ode(model, B, shape, 1e-5, args.tol, False, 1.0, noise=z, condition_input=cond)
    c = diff.last_ode
    print(json.dumps({"prior": args.trace_run, "batch": B, "tol": args.tol, "nfe": nfe,
                      "attempted_steps": c["n_accepted"] + c["n_rejected"], "solve_s": round(secs, 4)}))


def share(args):
    f = glob.glob(os.path.join(args.share, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    ctl = [i for i, r in enumerate(rows) if "::control_kernel(" in r["Kernel_Name"]]
    k = min(args.attempts, len(ctl) - 3)       # the last solve's attempted steps, without its two initial-step norms
    if k < 1:
        print(json.dumps({"error": "fewer than 4 control launches in the trace"}))
        return
    win = rows[ctl[-k - 1] + 1: ctl[-1] + 1]
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    total = sum(dur(r) for r in win)
    solver = sum(dur(r) for r in win if SOLVER.search(r["Kernel_Name"]))
    aten = [r["Kernel_Name"][:120] for r in win if "at::native" in r["Kernel_Name"] or "rocclr" in r["Kernel_Name"]]
    by = {}
    for r in win:
        m = SOLVER.search(r["Kernel_Name"])
        if m:
            by[m.group(1)] = by.get(m.group(1), 0.0) + dur(r) / k
    print(json.dumps({"attempted_steps": k, "launches_per_attempt": round(len(win) / k, 1),
                      "kernel_us_per_attempt": round(total / k, 1), "solver_us_per_attempt": round(solver / k, 2),
                      "solver_share": round(solver / total, 5) if total else None,
                      "solver_us_by_kernel": {a: round(b, 2) for a, b in by.items()},
                      "aten_launches": len(aten), "aten_names": sorted(set(aten))[:10]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--evals", type=int, default=30)
    ap.add_argument("--no-host-loop", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", choices=["global", "local"], default=None)
    ap.add_argument("--share", default=None)
    ap.add_argument("--attempts", type=int, default=8)
    args = ap.parse_args()
    if args.share:
        share(args)
    elif args.trace_run:
        trace_run(args)
    else:
        bench(args)


if __name__ == "__main__":
    main()
