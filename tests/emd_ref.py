"""Float64 reference of the approximate earth mover's distance (csrc/emd.hip), the inputs its GPU tests run on, and the
condition those inputs must meet.  numpy on the CPU; imports nothing from lion_amd.  Written from the algorithm emd.hip
documents (its header, the comments of its three passes and its entry points):

    remainL[k] = multiL, remainR[l] = multiR         (N >= M: multiL = 1, multiR = N // M;  else multiL = M // N, multiR = 1)
    for level in -4^7, -4^6, ..., -4^-1, 0:           E[l, k] = exp(level |x1[k] - x2[l]|^2)
      pass 1:  ratioL[k] = remainL[k] / (1e-9 + sum_l E[l, k] remainR[l])
      pass 2:  sumr[l]   = remainR[l] sum_k E[l, k] ratioL[k]
               ratioR[l] = fmin(remainR[l] / (sumr[l] + 1e-9), 1) remainR[l];   remainR[l] = fmax(0, remainR[l] - sumr[l])
      pass 3:  w[l, k]   = E[l, k] ratioL[k] ratioR[l];   match[l, k] += w;   remainL[k] = fmax(0, remainL[k] - sum_l w[l, k])
    cost = sum match[l, k] |x1[k] - x2[l]|^2,   d cost / d x1[k] = 2 sum_l match[l, k] (x1[k] - x2[l])   (match held constant)

The auction is well conditioned on some clouds and badly on others, and the shape does not tell which: where supply is
tight (N close to M) the clamps and the 1e-9 + sum denominators turn a rounding of one exp() into a visible change of the
plan.  `certificate` measures that on the CPU, from this reference alone: it reruns the auction with every exp() perturbed
by the error class of a CORRECT fp32 implementation and reports the largest deviation.  CASES lists, per shape, the first
(kind, seed) of a search over kinds x seeds 0..31 whose certificate stays within a quarter of the tolerance the GPU test
applies (tests/test_emd_reference_cpu.py asserts it), so a failure of the GPU test on such an input is a finding about the
kernel and not about the tolerance."""
import collections
import functools
import math

import numpy as np

U32 = 2.0 ** -24
LEVELS = tuple(-(4.0 ** j) for j in range(7, -2, -1)) + (0.0,)      # -4^7 ... -4^-1, 0

# the project's tolerances for this operator: what the GPU tests apply ...
TOL_COST, TOL_COST_FAST, TOL_MATCH, TOL_GRAD = 1e-4, 2e-4, 2e-3, 2e-3
# ... and the quarter of them a certified input keeps its own sensitivity within
CERT_LITERAL = {"cost": TOL_COST / 4, "match": TOL_MATCH / 4, "grad": TOL_GRAD / 4}
CERT_FAST = {"cost": TOL_COST_FAST / 4}


def f64(a):
    return np.asarray(a, dtype=np.float64)


def multipliers(N, M):
    """(multiL, multiR): integer division, as the entry points do it"""
    return (1, N // M) if N >= M else (M // N, 1)


# ---- perturbation models ------------------------------------------------------------------------------------------------

class Perturb:
    """The error class of a correct fp32 auction, drawn fresh wherever it is asked (that is per pass and level):
    `literal`  every exponent level * d carries a relative 2^-23 (the roundings of the distance and of the product), every
               value exp() a relative 2^-22 (v_exp_f32 and the rounded product that follows it);
    `fast`     `literal`, and every coordinate a relative 2^-23 of its own: the evaluation path rounds x * s, s up to 153,
               before it subtracts.
    Each factor is 1 + r * U with U uniform on [-1, 1]."""

    def __init__(self, model, seed):
        assert model in ("literal", "fast")
        self.model = model
        self.rng = np.random.default_rng(seed)

    def _factor(self, shape, r):
        return 1.0 + r * self.rng.uniform(-1.0, 1.0, shape)

    def coords(self, x):
        return x * self._factor(x.shape, 2.0 ** -23) if self.model == "fast" else x

    def arg(self, a):
        return a * self._factor(a.shape, 2.0 ** -23)

    def val(self, e):
        return e * self._factor(e.shape, 2.0 ** -22)


def sqdist(x1, x2):
    """D[l, k] = |x1[k] - x2[l]|^2, [M, N]"""
    d = x2[:, None, :] - x1[None, :, :]
    return (d * d).sum(-1)


def _weights(level, x1, x2, perturb):
    """E[l, k] of one pass"""
    if perturb is None:
        return np.exp(level * sqdist(x1, x2))
    return perturb.val(np.exp(perturb.arg(level * sqdist(perturb.coords(x1), perturb.coords(x2)))))


def auction64(x1, x2, perturb=None, levels=LEVELS, state=None):
    """match[M, N] of one pair of clouds x1 [N, 3], x2 [M, 3].  `state`, a dict, receives remainL / remainR / ratioL / ratioR
    as they stand after the last level run (with `levels` cut short: what the kernels' workspace holds at that point)."""
    x1, x2 = f64(x1), f64(x2)
    N, M = x1.shape[0], x2.shape[0]
    multiL, multiR = multipliers(N, M)
    remainL, remainR = np.full(N, float(multiL)), np.full(M, float(multiR))
    match = np.zeros((M, N))
    ratioL = ratioR = None
    for level in levels:
        E = _weights(level, x1, x2, perturb)
        ratioL = remainL / (1e-9 + (E * remainR[:, None]).sum(0))
        E = _weights(level, x1, x2, perturb)
        sumr = (E * ratioL[None, :]).sum(1) * remainR
        ratioR = np.fmin(remainR / (sumr + 1e-9), 1.0) * remainR
        remainR = np.fmax(0.0, remainR - sumr)
        E = _weights(level, x1, x2, perturb)
        w = E * ratioL[None, :] * ratioR[:, None]
        match += w
        remainL = np.fmax(0.0, remainL - w.sum(0))
    if state is not None:
        state.update(remainL=remainL, remainR=remainR, ratioL=ratioL, ratioR=ratioR)
    return match


# ---- the linear kernels ---------------------------------------------------------------------------------------------------

def matchcost64(x1, x2, match):
    """(cost, absprod): sum of match[l, k] |x1[k] - x2[l]|^2 and the sum of the absolute products"""
    p = f64(match) * sqdist(f64(x1), f64(x2))
    return float(p.sum()), float(np.abs(p).sum())


def grads64(gc, x1, x2, match):
    """(g1 [N, 3], g2 [M, 3], absprod1, absprod2) of gc * cost with match held constant (the reference's semantics)"""
    x1, x2, match, gc = f64(x1), f64(x2), f64(match), float(gc)
    diff = x1[None, :, :] - x2[:, None, :]                          # [M, N, 3]: x1[k] - x2[l]
    t = 2.0 * gc * match[:, :, None] * diff
    return t.sum(0), -t.sum(1), np.abs(t).sum(0), np.abs(t).sum(1)


def cost_floor(x1, x2):
    """2^-22 mass r^2: the part of the cost bound that does not scale with the cost (it matters where cost64 ~ 0).  mass is
    what the plan can ship, r^2 the largest squared coordinate norm."""
    N, M = len(x1), len(x2)
    multiL, multiR = multipliers(N, M)
    r2 = max(float((f64(x1) ** 2).sum(-1).max()), float((f64(x2) ** 2).sum(-1).max()))
    return 2.0 ** -22 * min(N * multiL, M * multiR) * r2


def chain_lengths(N, M):
    """the longest fp32 chain of each linear kernel: cost (M per row, then the per-workgroup partials), grad1, grad2"""
    return {"cost": M + math.ceil(N / 256), "grad1": M, "grad2": math.ceil(N / 64)}


def linear_bound(T, absprod):
    return (T + 8) * U32 * f64(absprod) + 1e-35


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def _sphere(rng, n, radius):
    v = rng.standard_normal((n, 3))
    return radius * v / np.linalg.norm(v, axis=1, keepdims=True)


def clouds(kind, N, M, seed, offset=(0.0, 0.0, 0.0)):
    """(x1 [N, 3], x2 [M, 3]) float32; everything downstream, the reference included, sees these float32 values
    uniform   both in the unit cube
    surface   a unit sphere against a sphere of radius 0.9
    permuted  cloud 2 is a permutation of cloud 1 (uniform; N == M)"""
    rng = np.random.default_rng([seed, N, M])
    if kind == "uniform":
        a, b = rng.random((N, 3)), rng.random((M, 3))
    elif kind == "surface":
        a, b = _sphere(rng, N, 1.0), _sphere(rng, M, 0.9)
    elif kind == "permuted":
        assert N == M
        a = rng.random((N, 3))
        b = a[rng.permutation(N)]
    else:
        raise ValueError(kind)
    off = np.asarray(offset, dtype=np.float64)
    return (a + off).astype(np.float32), (b + off).astype(np.float32)


Case = collections.namedtuple("Case", "N M kind seed offset")
Case.id = property(lambda c: f"{c.N}x{c.M}-{c.kind}{c.seed}" + ("-offset" if any(c.offset) else ""))
_O = (0.0, 0.0, 0.0)

# (kind, seed) per shape: the first of kinds x seeds 0..31 whose certificate passes (module docstring)
CASES = (
    Case(1, 1, "uniform", 0, _O),
    Case(1, 5, "uniform", 0, _O),
    Case(5, 1, "uniform", 0, _O),
    Case(7, 3, "uniform", 0, _O),
    Case(63, 65, "uniform", 0, _O),
    Case(65, 63, "uniform", 0, _O),
    Case(64, 256, "uniform", 0, _O),
    Case(127, 129, "uniform", 0, _O),
    Case(129, 127, "uniform", 0, _O),
    Case(255, 257, "surface", 3, _O),
    Case(257, 255, "surface", 2, _O),
    Case(130, 64, "uniform", 0, _O),
    Case(64, 200, "uniform", 0, _O),
    Case(300, 200, "surface", 2, _O),
    Case(1023, 1025, "surface", 0, _O),
    Case(1025, 1023, "surface", 0, _O),
    Case(64, 200, "uniform", 0, (3.0, -2.0, 1.0)),
    Case(129, 129, "permuted", 0, _O),
)


def case_clouds(case):
    return clouds(case.kind, case.N, case.M, case.seed, case.offset)


def filler_clouds(case, j=1):
    """an arbitrary pair of the case's shape, for the other slots of a batch"""
    return clouds("uniform", case.N, case.M, 1000 * j + case.seed, case.offset)


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict of the float64 results of a case (gc = 1), computed once: x1, x2, match, cost, absprod, g1, g2"""
    x1, x2 = case_clouds(case)
    match = auction64(x1, x2)
    cost, absprod = matchcost64(x1, x2, match)
    g1, g2, _, _ = grads64(1.0, x1, x2, match)
    return dict(x1=x1, x2=x2, match=match, cost=cost, absprod=absprod, g1=g1, g2=g2)


def deviation(base, x1, x2, match):
    """how far `match` lies from the reference results `base` of the same clouds: cost relative and absolute, match max
    abs, gradients max abs relative to max |g64|"""
    cost, _ = matchcost64(x1, x2, match)
    g1, g2, _, _ = grads64(1.0, x1, x2, match)
    gmax = max(np.abs(base["g1"]).max(), np.abs(base["g2"]).max(), 1e-300)
    return {"cost": abs(cost - base["cost"]) / max(abs(base["cost"]), 1e-300),
            "cost_abs": abs(cost - base["cost"]),
            "match": float(np.abs(match - base["match"]).max()),
            "grad": float(max(np.abs(g1 - base["g1"]).max(), np.abs(g2 - base["g2"]).max()) / gmax)}


def certificate(case, model, draws=3):
    """the largest deviation, over `draws` seeded draws of the perturbation `model`, of the perturbed auction from
    auction64 on the clouds of `case`: {"cost": relative, "cost_abs", "match": max abs, "grad": max abs / max |g64|}"""
    base = reference(case)
    worst = {"cost": 0.0, "cost_abs": 0.0, "match": 0.0, "grad": 0.0}
    for d in range(draws):
        m = auction64(base["x1"], base["x2"], Perturb(model, [d, case.N, case.M, case.seed]))
        for k, v in deviation(base, base["x1"], base["x2"], m).items():
            worst[k] = max(worst[k], v)
    return worst


def certificate_failures(case, model, c):
    """the entries of the certificate `c` beyond a quarter of the tolerance the GPU test applies to `case`, as a list of
    (name, value, limit).  The cost passes on its relative limit or, where the cost itself nearly vanishes (`permuted`), on a
    quarter of the floor of the GPU bound -- either alone, which is never more than a quarter of their sum."""
    lim = CERT_LITERAL if model == "literal" else CERT_FAST
    base = reference(case)
    bad = []
    if c["cost"] > lim["cost"] and c["cost_abs"] > cost_floor(base["x1"], base["x2"]) / 4:
        bad.append(("cost", c["cost"], lim["cost"]))
    for k in ("match", "grad"):
        if k in lim and c[k] > lim[k]:
            bad.append((k, c[k], lim[k]))
    return bad


def certified(case, model, draws=3):
    c = certificate(case, model, draws)
    return not certificate_failures(case, model, c), c
