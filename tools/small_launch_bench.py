"""In-graph time of the small serial launches of a PVConv, as tools/pw_bench.py times a 1x1
convolution: 20 calls captured in one hipGraph, replayed 5 times, microseconds per call; REPEATS repeats per case.
  fold_tconst  lion_groupnorm_fold, lion_conv3d_const_response and the two one after the other (conv1's fold and conv2's
               constant response of a PVConv)
  fold_se      lion_groupnorm_fold_se and lion_internal_groupnorm_fold_se_plain
  pw           lion_pwconv_forward (short-activation kernel) and lion_internal_pwconv_small_plain
A plain twin the loaded library does not have (an older tree) is left out.
usage: small_launch_bench.py [--cases CASES.json from tools/step_shapes.py] [--batches 32,4] [--repeats 3] [--kinds fold_tconst,fold_se,pw]"""
import argparse, json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lion_amd import _lib

# the local prior's step at 2048 points, B = 32 (tools/step_shapes.py; `launches` = over the 7 forward passes of that run)
DEFAULT = [
    dict(kind='fold_se', launches=14, C=32, T=128, G=8, H=4),
    dict(kind='fold_se', launches=7, C=64, T=16, G=8, H=8),
    dict(kind='fold_se', launches=14, C=64, T=128, G=8, H=8),
    dict(kind='fold_se', launches=49, C=128, T=2, G=8, H=16),
    dict(kind='fold_se', launches=14, C=128, T=16, G=8, H=16),
    dict(kind='fold_tconst', launches=14, C=32, T=128, G=8, Cout=32),
    dict(kind='fold_tconst', launches=7, C=64, T=16, G=8, Cout=64),
    dict(kind='fold_tconst', launches=14, C=64, T=128, G=8, Cout=64),
    dict(kind='fold_tconst', launches=14, C=128, T=16, G=8, Cout=128),
    dict(kind='pw', launches=21, Cin=128, Cout=128, L=64, pro=False, stats=True),
    dict(kind='pw', launches=7, Cin=128, Cout=128, L=64, pro=True, stats=True),
    dict(kind='pw', launches=7, Cin=128, Cout=768, L=16, pro=False, stats=False),
    dict(kind='pw', launches=7, Cin=256, Cout=128, L=16, pro=False, stats=False),
    dict(kind='pw', launches=3, Cin=320, Cout=128, L=64, pro=False, stats=True),
    dict(kind='pw', launches=4, Cin=384, Cout=128, L=64, pro=False, stats=True),
]


def t_us(f, n=20):
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


def have(name):
    return name in _lib.SIGNATURES


def fold_args(B, C, T, G):
    r = lambda *s: torch.randn(*s, device="cuda")
    stats = r(B, C, T, 2)
    stats[..., 1] = stats[..., 1].abs() * 40 + 30
    fg = r(B, 2 * C)
    return stats, r(C), r(C), fg[:, :C], fg[:, C:], torch.empty(B, C, device="cuda"), torch.empty(B, C, device="cuda")


def runners(c, B):
    """label -> callable, in print order"""
    r = lambda *s: torch.randn(*s, device="cuda")
    k = c["kind"]
    if k == "fold_tconst":
        C, T, G, Co = c["C"], c["T"], c["G"], c["Cout"]
        stats, gam, bet, fac, gb, A, Bs = fold_args(B, C, T, G)
        cm, ws, b2, b1, tc = torch.empty(B, C, device="cuda"), r(27, C, Co), r(Co), r(C), torch.empty(B, 27, Co, device="cuda")
        fold = lambda: _lib.call("lion_groupnorm_fold", stats, B, C, T, G, 4096, gam, bet, fac, gb, 2 * C, 1e-5, A, Bs, cm)
        resp = lambda: _lib.call("lion_conv3d_const_response", ws, b2, b1, A, Bs, B, C, Co, tc)
        out = {"fold": fold, "response": resp, "fold+response": lambda: (fold(), resp())}
        return out
    if k == "fold_se":
        C, T, G, H = c["C"], c["T"], c["G"], c["H"]
        stats, gam, bet, fac, gb, A, Bs = fold_args(B, C, T, G)
        w1, w2 = r(H, C), r(C, H)
        f = lambda name: (lambda: _lib.call(name, stats, B, C, T, G, 4096, gam, bet, fac, gb, 2 * C, 1e-5, w1, w2, H, A, Bs))
        out = {"fold_se": f("lion_groupnorm_fold_se")}
        if have("lion_internal_groupnorm_fold_se_plain"):
            out["plain"] = f("lion_internal_groupnorm_fold_se_plain")
        return out
    if k == "pw":
        Ci, Co, L = c["Cin"], c["Cout"], c["L"]
        lib = _lib.load()
        wp = torch.zeros(lib.lion_pwconv_packed_floats(Co, Ci), device="cuda")
        _lib.call("lion_pwconv_pack_weights", r(Co, Ci), Co, Ci, wp)
        x, bias, y = r(B, Ci, L), r(Co), torch.empty(B, Co, L, device="cuda")
        pa, pb = (r(B, Ci), r(B, Ci)) if c["pro"] else (None, None)
        st = torch.empty(B, Co, lib.lion_pwconv_stat_tiles(Co, Ci, L), 2, device="cuda") if c["stats"] else None
        out = {"pwconv": lambda: _lib.call("lion_pwconv_forward", x, wp, bias, B, Ci, Co, L, pa, pb, y, st)}
        if have("lion_internal_pwconv_small_plain"):
            out["plain"] = lambda: _lib.call("lion_internal_pwconv_small_plain", x, wp, bias, B, Ci, Co, L, pa, pb, None, None, None,
                                             None, 0, 0, y, st)
        return out
    return {}


ap = argparse.ArgumentParser()
ap.add_argument("--cases", default=None)
ap.add_argument("--batches", default="32,4")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--kinds", default="fold_tconst,fold_se,pw")
a = ap.parse_args()
cases = [c for c in (json.load(open(a.cases)) if a.cases else DEFAULT) if c["kind"] in a.kinds.split(",")]
torch.manual_seed(0)
for B in [int(b) for b in a.batches.split(",")]:
    print(f"B = {B}: us per call in a 20-call graph, {a.repeats} repeats (min .. max)")
    for c in cases:
        rs = runners(c, B)
        if not rs:
            continue
        shape = " ".join(f"{k}={v}" for k, v in c.items() if k not in ("kind", "launches"))
        cells = []
        for label, f in rs.items():
            ts = [t_us(f) for _ in range(a.repeats)]
            cells.append(f"{label} {sorted(ts)[len(ts) // 2]:5.1f} ({min(ts):.1f} .. {max(ts):.1f})")
        print(f"  {c['kind']:11s} {shape:44s} " + "   ".join(cells), flush=True)
