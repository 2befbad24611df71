"""CPU: what makes tests/emd_ref.py and its inputs trustworthy before tests/test_emd_numerics_gpu.py leans on them.  The
vectorised float64 auction against a scalar loop transcription and float64 autograd, the invariants of a transport plan on
every case, the CONDITION on the inputs (every row of CASES keeps its own sensitivity to the rounding of a correct fp32
implementation within a quarter of the tolerance the GPU test applies: a condition, not a measurement), the project's fp32
oracle against the float64 reference on those inputs, and plain fp32 numpy evaluations of the linear kernels within HALF of
their derived bounds."""
import math

import numpy as np
import pytest
import torch

import emd_ref as er

f32 = np.float32
IDS = [c.id for c in er.CASES]


def draws_of(case):
    return 2 if max(case.N, case.M) > 1000 else 3


# ---- the reference itself ----------------------------------------------------------------------------------------------

def auction_loops(x1, x2):
    """the three passes as plain scalar loops, one accumulation per statement, in Python floats (float64)"""
    N, M = len(x1), len(x2)
    x1, x2 = [[float(v) for v in p] for p in x1], [[float(v) for v in p] for p in x2]
    multiL, multiR = (1.0, float(N // M)) if N >= M else (float(M // N), 1.0)
    remainL, remainR = [multiL] * N, [multiR] * M
    ratioL, ratioR = [0.0] * N, [0.0] * M
    match = [[0.0] * N for _ in range(M)]

    def d2(k, l):
        return (x2[l][0] - x1[k][0]) ** 2 + (x2[l][1] - x1[k][1]) ** 2 + (x2[l][2] - x1[k][2]) ** 2

    for j in range(7, -3, -1):
        level = 0.0 if j == -2 else -(4.0 ** j)
        for k in range(N):
            suml = 1e-9
            for l in range(M):
                suml += math.exp(level * d2(k, l)) * remainR[l]
            ratioL[k] = remainL[k] / suml
        for l in range(M):
            sumr = 0.0
            for k in range(N):
                sumr += math.exp(level * d2(k, l)) * ratioL[k]
            sumr *= remainR[l]
            consumption = min(remainR[l] / (sumr + 1e-9), 1.0)
            ratioR[l] = consumption * remainR[l]
            remainR[l] = max(0.0, remainR[l] - sumr)
        for k in range(N):
            suml = 0.0
            for l in range(M):
                w = math.exp(level * d2(k, l)) * ratioL[k] * ratioR[l]
                match[l][k] += w
                suml += w
            remainL[k] = max(0.0, remainL[k] - suml)
    return np.array(match)


@pytest.mark.parametrize("N,M", [(1, 1), (1, 5), (5, 1), (7, 3), (3, 7), (8, 8), (8, 4), (2, 8), (6, 5)])
def test_auction64_is_the_scalar_loop_transcription(N, M):
    for kind in ("uniform", "surface"):
        x1, x2 = er.clouds(kind, N, M, 3)
        got, want = er.auction64(x1, x2), auction_loops(x1, x2)
        assert got.shape == (M, N)
        assert np.abs(got - want).max() <= 1e-12, (kind, np.abs(got - want).max())


def test_auction64_levels_and_state():
    assert er.LEVELS == (-16384.0, -4096.0, -1024.0, -256.0, -64.0, -16.0, -4.0, -1.0, -0.25, 0.0)
    x1, x2 = er.clouds("uniform", 6, 13, 0)
    st = {}
    m = er.auction64(x1, x2, levels=er.LEVELS[:1], state=st)
    assert st["remainL"].shape == st["ratioL"].shape == (6,) and st["remainR"].shape == st["ratioR"].shape == (13,)
    # what one level ships leaves both sides: remain = multi - marginal, exactly where no clamp acted
    np.testing.assert_allclose(st["remainL"], 2.0 - m.sum(0), atol=1e-12)
    assert np.all(st["remainR"] <= 1.0) and np.all(st["remainR"] >= 0.0)


@pytest.mark.parametrize("N,M", [(1, 1), (5, 1), (7, 3), (9, 20), (65, 63)])
def test_matchcost64_and_grads64_are_float64_autograd(N, M):
    x1, x2 = er.clouds("surface", N, M, 5)
    rng = np.random.default_rng(N + M)
    match = rng.random((M, N))
    gc = -1.75
    a = torch.from_numpy(x1).double().requires_grad_(True)
    b = torch.from_numpy(x2).double().requires_grad_(True)
    cost = (torch.from_numpy(match) * ((a[None, :, :] - b[:, None, :]) ** 2).sum(-1)).sum()
    (gc * cost).backward()
    c, ap = er.matchcost64(x1, x2, match)
    g1, g2, a1, a2 = er.grads64(gc, x1, x2, match)
    assert abs(c - cost.item()) <= 1e-12 * abs(cost.item()) and abs(ap - c) <= 1e-12 * c     # every product is >= 0
    assert np.abs(g1 - a.grad.numpy()).max() <= 1e-12 * np.abs(g1).max()
    assert np.abs(g2 - b.grad.numpy()).max() <= 1e-12 * np.abs(g2).max()
    assert np.all(a1 >= np.abs(g1) - 1e-15) and np.all(a2 >= np.abs(g2) - 1e-15)
    assert a1.shape == (N, 3) and a2.shape == (M, 3)


def test_clouds_are_float32_and_what_they_say():
    x1, x2 = er.clouds("uniform", 40, 30, 1)
    assert x1.dtype == x2.dtype == f32 and x1.shape == (40, 3) and x2.shape == (30, 3)
    assert x1.min() >= 0 and x1.max() <= 1
    s1, s2 = er.clouds("surface", 40, 30, 1)
    np.testing.assert_allclose(np.linalg.norm(s1, axis=1), 1.0, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(s2, axis=1), 0.9, atol=1e-6)
    p1, p2 = er.clouds("permuted", 33, 33, 1)
    assert not np.array_equal(p1, p2) and np.array_equal(np.sort(p1, axis=0), np.sort(p2, axis=0))
    o1, _ = er.clouds("uniform", 40, 30, 1, (3.0, -2.0, 1.0))
    np.testing.assert_allclose(o1, x1.astype(np.float64) + [3.0, -2.0, 1.0], atol=3e-7)
    assert all(np.array_equal(u, v) for u, v in zip(er.clouds("surface", 9, 4, 7), er.clouds("surface", 9, 4, 7)))


def test_cases_cover_the_shapes_of_the_issue():
    want = [(1, 1), (1, 5), (5, 1), (7, 3), (63, 65), (65, 63), (64, 256), (127, 129), (129, 127), (255, 257), (257, 255),
            (130, 64), (64, 200), (300, 200), (1023, 1025), (1025, 1023), (64, 200), (129, 129)]
    assert [(c.N, c.M) for c in er.CASES] == want
    assert er.CASES[-2].offset == (3.0, -2.0, 1.0) and er.CASES[-1].kind == "permuted"
    assert len(set(IDS)) == len(IDS)
    assert er.multipliers(130, 64) == (1, 2) and er.multipliers(64, 200) == (3, 1) and er.multipliers(64, 256) == (4, 1)


# ---- invariants ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_reference_match_is_a_transport_plan(case):
    r = er.reference(case)
    m = r["match"]
    multiL, multiR = er.multipliers(case.N, case.M)
    assert m.shape == (case.M, case.N) and np.all(np.isfinite(m)) and np.all(m >= 0)
    assert m.sum(0).max() <= multiL * (1 + 1e-12), m.sum(0).max()
    assert m.sum(1).max() <= multiR * (1 + 1e-12), m.sum(1).max()
    print(f"{case.id}: shipped {m.sum():.6f} of {min(case.N * multiL, case.M * multiR)}, cost64 {r['cost']:.6g}")


def test_one_point_each_ships_everything():
    x1, x2 = er.clouds("uniform", 1, 1, 0)
    m = er.auction64(x1, x2)
    d2 = float(((x1.astype(np.float64) - x2) ** 2).sum())
    assert abs(m[0, 0] - 1.0) <= 1e-8                                # the 1e-9 of the denominators
    assert abs(er.matchcost64(x1, x2, m)[0] - d2) <= 1e-8 * d2


def test_two_point_crossed_known_answer():
    """the pair of test_emd_two_point_known_answer (tests/test_oracle_cpu.py): the crossed matching is optimal"""
    p1 = np.array([[1.7, -0.1, 0.1], [0.1, 1.2, 0.3]], f32)
    p2 = np.array([[0.3, 1.8, 0.2], [1.2, -0.2, 0.3]], f32)
    m = er.auction64(p1, p2)
    gt = ((p1[0].astype(np.float64) - p2[1]) ** 2).sum() + ((p1[1].astype(np.float64) - p2[0]) ** 2).sum()
    np.testing.assert_allclose(er.matchcost64(p1, p2, m)[0] / 2, gt / 2, rtol=1e-4)
    np.testing.assert_allclose(m, [[0, 1], [1, 0]], atol=1e-4)


# ---- the condition on the inputs -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_case_is_certified(case):
    """a quarter of the GPU tolerances -- literal: cost 2.5e-5, match 5e-4, gradients 5e-4; fast: cost 5e-5"""
    for model, lim in (("literal", er.CERT_LITERAL), ("fast", er.CERT_FAST)):
        c = er.certificate(case, model, draws_of(case))
        print(f"certificate {case.id} {model}: cost {c['cost']:.2e} (abs {c['cost_abs']:.2e}) match {c['match']:.2e} "
              f"grad {c['grad']:.2e}  (limits {lim})")
        assert not er.certificate_failures(case, model, c), (case.id, model, er.certificate_failures(case, model, c))


def test_the_permuted_case_is_the_one_that_needs_the_floor():
    """cloud 2 a permutation of cloud 1: the plan is the permutation to a few percent, the cost a 1e-6 of an ordinary one"""
    case = er.CASES[-1]
    r = er.reference(case)
    perm = np.array([np.flatnonzero((r["x2"] == p).all(1))[0] for p in r["x1"]])
    want = np.zeros((case.M, case.N))
    want[perm, np.arange(case.N)] = 1.0
    assert np.abs(r["match"] - want).max() < 0.05
    assert 0 < r["cost"] < er.cost_floor(r["x1"], r["x2"]) / er.TOL_COST


def test_perturbation_models_are_seeded_and_of_their_class():
    x = np.linspace(-3.0, 5.0, 4000).reshape(-1, 4)
    p, q = er.Perturb("literal", 1), er.Perturb("literal", 1)
    a, b = p.arg(x), q.arg(x)
    assert np.array_equal(a, b) and not np.array_equal(a, p.arg(x))  # seeded; fresh at every call
    assert 0.5 * 2.0 ** -23 < np.abs(a / x - 1).max() <= 2.0 ** -23
    assert 0.5 * 2.0 ** -22 < np.abs(p.val(x) / x - 1).max() <= 2.0 ** -22
    assert np.array_equal(p.coords(x), x)
    assert 0.5 * 2.0 ** -23 < np.abs(er.Perturb("fast", 1).coords(x) / x - 1).max() <= 2.0 ** -23


# ---- the fp32 oracle the suite already trusts -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_fp32_oracle_agrees_with_the_reference_on_certified_cases(orc, case):
    r = er.reference(case)
    x1, x2 = r["x1"][None], r["x2"][None]
    multiL, multiR = er.multipliers(case.N, case.M)
    match = orc.approxmatch(x1, x2)
    cost = float(orc.matchcost(x1, x2, match)[0])
    g1, g2 = orc.matchcost_backward(np.ones(1, f32), x1, x2, match)
    gmax = max(np.abs(r["g1"]).max(), np.abs(r["g2"]).max())
    ratios = {"cost": abs(cost - r["cost"]) / (er.TOL_COST * r["cost"] + er.cost_floor(r["x1"], r["x2"])),
              "match": np.abs(match[0] - r["match"]).max() / (er.TOL_MATCH * max(multiL, multiR)),
              "grad": max(np.abs(g1[0] - r["g1"]).max(), np.abs(g2[0] - r["g2"]).max()) / (er.TOL_GRAD * gmax)}
    print(f"oracle {case.id}: error / bound " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


# ---- the bounds of the linear kernels ----------------------------------------------------------------------------------------

def half(got32, ref, bound, what):
    ratio = float((np.abs(np.asarray(got32, dtype=np.float64) - ref) / bound).max())
    print(f"{what}: fp32 numpy / bound = {ratio:.3f}")
    assert ratio <= 0.5, (what, ratio)


def chain32(terms, axis):
    """the last element of the sequential fp32 running sum along `axis` (np.cumsum adds in index order)"""
    return np.take(np.cumsum(terms.astype(f32), axis=axis, dtype=f32), -1, axis=axis)


def wave_sum32(v):
    """fp32 sum over the 64 lanes of a wave (axis 0) in the order of the kernels' xor-shuffle butterfly: 32, 16, ..., 1"""
    v = v.astype(f32)
    while v.shape[0] > 1:
        h = v.shape[0] // 2
        v = v[:h] + v[h:]
    return v[0]


@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_fp32_numpy_linear_kernels_stay_within_half_their_bounds(case):
    """matchcost and both gradients in fp32 numpy in the order emd.hip documents for them (a row of the cost and of grad1
    runs over the whole other cloud in index order, the rows of a workgroup and the 64 strided chains of grad2 meet in a
    butterfly), on the float64 match rounded to fp32"""
    r = er.reference(case)
    x1, x2 = r["x1"], r["x2"]
    N, M = case.N, case.M
    m32 = r["match"].astype(f32)
    gc = f32(-1.75)
    T = er.chain_lengths(N, M)
    cost64, absprod = er.matchcost64(x1, x2, m32)
    g1, g2, a1, a2 = er.grads64(gc, x1, x2, m32)
    d = x2[:, None, :] - x1[None, :, :]                                # [M, N, 3] fp32
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    rows = chain32(d2 * m32, 0)                                        # per point of cloud 1, l ascending
    w = wave_sum32(np.concatenate([rows, np.zeros((-N) % 256, f32)]).reshape(-1, 4, 64).transpose(2, 0, 1))   # [nb, 4]
    parts = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])                  # one per workgroup of 256 rows
    half(chain32(parts, 0), cost64, er.linear_bound(T["cost"], absprod), f"matchcost {case.id}")
    t = (x1[None, :, :] - x2[:, None, :]) * (m32 * f32(2))[:, :, None]
    half(chain32(t, 0) * gc, g1, er.linear_bound(T["grad1"], a1), f"grad1 {case.id}")
    lanes = chain32(np.concatenate([-t, np.zeros((M, (-N) % 64, 3), f32)], 1).reshape(M, -1, 64, 3), 1)        # [M, 64, 3]
    half(wave_sum32(lanes.transpose(1, 0, 2)) * gc, g2, er.linear_bound(T["grad2"], a2), f"grad2 {case.id}")
