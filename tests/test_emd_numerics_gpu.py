"""-m gpu: every kernel of csrc/emd.hip through its C entry point, against the float64 reference of tests/emd_ref.py on the
inputs that tests/test_emd_reference_cpu.py certifies (their own sensitivity to the rounding of a correct fp32 auction stays
within a quarter of every tolerance here), at the shapes where a path can go wrong: fewer rows than lanes, one point, the
64-row and 128-row workgroup edges, the 256-element wave quarter and the 1024-element tile, multiL / multiR != 1,
coordinates away from the unit cube.  Numeric comparisons run at B = 2 with the certified pair in slot 1, so batch offsets
matter.  The tolerances are the project's: cost 1e-4 (2e-4 on the evaluation path), match 2e-3, gradients 2e-3
of their maximum; the linear kernels get bounds derived from their sums of absolute products.  What the file's comments
promise without a tolerance -- batch-size and run-to-run independence -- is compared bit for bit, and every output and the
workspace are written inside their bounds and do not depend on what the buffers held before."""
import numpy as np
import pytest
import torch

import emd_ref as er
from test_pointwise_numerics_gpu import dev, host

pytestmark = pytest.mark.gpu

f32 = np.float32
IDS = [c.id for c in er.CASES]
GC = np.array([3.0, -1.75, 0.625], f32)                             # grad_cost per batch slot
SENT = 0x7FC0BEEF                                                   # guard-band pattern (as float32: a NaN with a payload)


def lib():
    from lion_amd import _lib
    return _lib


def call(name, *args):
    lib().call(name, *args)


def out(*shape):
    """an output buffer full of NaN: whatever a kernel leaves unwritten, or accumulates into, shows"""
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def workspace(B, N, M):
    nbytes = lib().load().lion_emd_workspace_bytes(B, N, M)
    return torch.full((nbytes,), 0xFF, device="cuda", dtype=torch.uint8), nbytes      # 0xFFFFFFFF: NaN


def approxmatch(x1, x2):
    B, N, M = x1.shape[0], x1.shape[1], x2.shape[1]
    match = out(B, M, N)
    call("lion_emd_approxmatch", x1, x2, B, N, M, match, *workspace(B, N, M))
    return match


def matchcost(x1, x2, match):
    B, N, M = x1.shape[0], x1.shape[1], x2.shape[1]
    cost = out(B)
    call("lion_emd_matchcost", x1, x2, match, B, N, M, cost, *workspace(B, N, M))
    return cost


def backward(gc, x1, x2, match):
    B, N, M = x1.shape[0], x1.shape[1], x2.shape[1]
    g1, g2 = out(B, N, 3), out(B, M, 3)
    call("lion_emd_matchcost_backward", gc, x1, x2, match, B, N, M, g1, g2)
    return g1, g2


def fast_cost(x1, x2):
    B, N, M = x1.shape[0], x1.shape[1], x2.shape[1]
    cost = out(B)
    call("lion_emd_cost", x1, x2, B, N, M, cost, *workspace(B, N, M))
    return cost


def batch_of(case, B):
    """[B, N, 3], [B, M, 3] float32: the certified pair LAST, arbitrary pairs of the same shape in front of it"""
    pairs = [er.filler_clouds(case, j) for j in range(1, B)] + [er.case_clouds(case)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def report(what, err, bound):
    ratio = float(np.max(np.asarray(err, dtype=np.float64) / bound))
    print(f"{what}: worst error / bound = {ratio:.4f}")
    assert np.all(np.isfinite(err)), what
    assert ratio <= 1.0, f"{what}: {ratio:.4f} x the bound"
    return ratio


def cost_bound(r, tol):
    return tol * r["cost"] + er.cost_floor(r["x1"], r["x2"])


# ---- the literal path: approxmatch -> matchcost -> matchcost_backward ------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_literal_path_against_float64(case):
    r = er.reference(case)
    N, M = case.N, case.M
    multiL, multiR = er.multipliers(N, M)
    x1, x2 = (dev(v) for v in batch_of(case, 2))
    match = approxmatch(x1, x2)
    cost = matchcost(x1, x2, match)
    g1, g2 = backward(dev(GC[:2]), x1, x2, match)
    m = host(match).astype(np.float64)
    # a transport plan, in both slots of the batch
    assert np.all(np.isfinite(m)) and np.all(m >= 0)
    assert m.sum(1).max() <= multiL * (1 + 1e-5), m.sum(1).max()      # over l: what point k of cloud 1 ships
    assert m.sum(2).max() <= multiR * (1 + 1e-5), m.sum(2).max()      # over k: what point l of cloud 2 receives
    report(f"emd literal cost {case.id}", abs(float(cost[1]) - r["cost"]), cost_bound(r, er.TOL_COST))
    report(f"emd literal match {case.id}", np.abs(m[1] - r["match"]).max(), er.TOL_MATCH * max(multiL, multiR))
    gmax = abs(float(GC[1])) * max(np.abs(r["g1"]).max(), np.abs(r["g2"]).max())
    report(f"emd literal grad1 {case.id}", np.abs(host(g1)[1] - float(GC[1]) * r["g1"]), er.TOL_GRAD * gmax)
    report(f"emd literal grad2 {case.id}", np.abs(host(g2)[1] - float(GC[1]) * r["g2"]), er.TOL_GRAD * gmax)


# ---- the evaluation path: lion_emd_cost ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_fast_path_cost_against_float64(case):
    r = er.reference(case)
    x1, x2 = (dev(v) for v in batch_of(case, 2))
    cost = host(fast_cost(x1, x2))
    assert np.all(np.isfinite(cost)) and np.all(cost >= 0)
    report(f"emd fast cost {case.id}", abs(float(cost[1]) - r["cost"]), cost_bound(r, er.TOL_COST_FAST))


@pytest.mark.parametrize("case", [c for c in er.CASES if (c.N, c.M) in ((5, 1), (130, 64), (64, 200))], ids=lambda c: c.id)
def test_earth_mover_distance_nograd_divides_by_n_and_takes_every_input_form(case):
    """[B, 3, N] with transpose=True (a strided view the wrapper has to make contiguous), [N, 3] without a batch dimension,
    and cost / N with N the size of the FIRST cloud where the two differ"""
    from lion_amd.emd import earth_mover_distance_nograd
    r = er.reference(case)
    x1, x2 = (dev(v) for v in batch_of(case, 2))
    direct = fast_cost(x1, x2) / float(case.N)
    t1, t2 = x1.transpose(1, 2).contiguous(), x2.transpose(1, 2).contiguous()          # [B, 3, N]
    assert torch.equal(earth_mover_distance_nograd(t1, t2, transpose=True), direct)
    assert torch.equal(earth_mover_distance_nograd(x1, x2, transpose=False), direct)
    one = earth_mover_distance_nograd(x1[1], x2[1], transpose=False)
    assert one.shape == (1,) and torch.equal(one, direct[1:])
    report(f"emd nograd {case.id}", abs(float(one[0]) - r["cost"] / case.N),
           (cost_bound(r, er.TOL_COST_FAST) + er.U32 * r["cost"]) / case.N)


# ---- the linear kernels alone: conditioning plays no part --------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_matchcost_and_backward_on_a_given_match(case):
    """slot 1: the float64 match rounded to fp32; slot 0: an arbitrary dense matrix.  The references are taken on exactly
    these fp32 inputs; the bounds are (T + 8) 2^-24 of the sums of absolute products, T the longest fp32 chain (M per row of
    the cost and of grad1, ceil(N / 64) per lane of grad2, one more per workgroup partial of the cost)."""
    N, M = case.N, case.M
    x1, x2 = batch_of(case, 2)
    rng = np.random.default_rng([N, M, 7])
    match = np.stack([(rng.random((M, N)) ** 8).astype(f32), er.reference(case)["match"].astype(f32)])
    cost = host(matchcost(dev(x1), dev(x2), dev(match)))
    g1, g2 = (host(g) for g in backward(dev(GC[:2]), dev(x1), dev(x2), dev(match)))
    T = er.chain_lengths(N, M)
    for b in range(2):
        c64, absprod = er.matchcost64(x1[b], x2[b], match[b])
        r1, r2, a1, a2 = er.grads64(GC[b], x1[b], x2[b], match[b])
        report(f"emd matchcost {case.id} slot {b}", abs(float(cost[b]) - c64), er.linear_bound(T["cost"], absprod))
        report(f"emd grad1 {case.id} slot {b}", np.abs(g1[b] - r1), er.linear_bound(T["grad1"], a1))
        report(f"emd grad2 {case.id} slot {b}", np.abs(g2[b] - r2), er.linear_bound(T["grad2"], a2))


# ---- bit-exact properties -------------------------------------------------------------------------------------------------------

def everything(x1, x2, gc):
    """both paths on one batch: (match, cost, grad1, grad2, fast cost)"""
    match = approxmatch(x1, x2)
    return (match, matchcost(x1, x2, match), *backward(gc, x1, x2, match), fast_cost(x1, x2))


@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_a_pair_computes_the_same_alone_in_a_batch_and_twice(case):
    x1, x2 = (dev(v) for v in batch_of(case, 3))
    gc = dev(GC)
    whole = everything(x1, x2, gc)
    again = everything(x1, x2, gc)
    names = ("match", "cost", "grad1", "grad2", "fast cost")
    for n, a, b in zip(names, whole, again):
        assert torch.equal(a, b), f"{n}: two runs differ"
    assert len(set(whole[1].tolist())) == 3                          # the pairs ARE distinct: three different costs
    for i in range(3):
        alone = everything(x1[i:i + 1].contiguous(), x2[i:i + 1].contiguous(), gc[i:i + 1].contiguous())
        for n, a, b in zip(names, whole, alone):
            assert torch.equal(a[i:i + 1], b), f"{n}: pair {i} of a batch of 3 differs from the pair alone"


def test_pairwise_distance_equals_the_per_pair_calls():
    """3 x 5 clouds of 70 points in batches of 4 pairs: 15 pairs are no multiple of the batch"""
    from lion_amd.emd import earth_mover_distance_nograd
    from lion_amd.metrics import pairwise_distance
    rng = np.random.default_rng(70)
    s, r = dev(rng.random((3, 70, 3)).astype(f32)), dev(rng.random((5, 70, 3)).astype(f32))
    got = pairwise_distance("EMD", s, r, pair_batch=4)
    assert got.shape == (3, 5)
    for i in range(3):
        for j in range(5):
            one = earth_mover_distance_nograd(s[i:i + 1], r[j:j + 1], transpose=False)
            assert torch.equal(got[i, j:j + 1], one), (i, j)


# ---- memory: outputs and workspace written inside their bounds, whatever they held ------------------------------------------

class Guarded:
    """`n` float32 elements in the middle of a larger buffer whose 64 elements on either side hold SENT"""
    BAND = 64

    def __init__(self, n, fill):
        self.whole = torch.full((n + 2 * self.BAND,), SENT, device="cuda", dtype=torch.int32)
        self.view = self.whole.view(torch.float32)[self.BAND:self.BAND + n]
        self.view.fill_(fill)

    def fill(self, value):
        self.view.fill_(value)

    def intact(self):
        return bool((self.whole[:self.BAND] == SENT).all()) and bool((self.whole[-self.BAND:] == SENT).all())

    def bits(self):
        return self.view.view(torch.int32).clone()


def guarded_run(x1, x2, gc, fill):
    """every entry point on guarded outputs and a guarded workspace of exactly lion_emd_workspace_bytes, each refilled with
    `fill` before every call (production passes torch.empty); -> the outputs' bit patterns"""
    B, N, M = x1.shape[0], x1.shape[1], x2.shape[1]
    nbytes = lib().load().lion_emd_workspace_bytes(B, N, M)
    assert nbytes % 4 == 0
    ws = Guarded(nbytes // 4, fill)
    bufs = {n: Guarded(k, fill) for n, k in (("match", B * M * N), ("cost", B), ("g1", B * N * 3), ("g2", B * M * 3), ("fast", B))}
    v = {n: g.view for n, g in bufs.items()}
    call("lion_emd_approxmatch", x1, x2, B, N, M, v["match"], ws.view, nbytes)
    ws.fill(fill)
    call("lion_emd_matchcost", x1, x2, v["match"], B, N, M, v["cost"], ws.view, nbytes)
    call("lion_emd_matchcost_backward", gc, x1, x2, v["match"], B, N, M, v["g1"], v["g2"])
    ws.fill(fill)
    call("lion_emd_cost", x1, x2, B, N, M, v["fast"], ws.view, nbytes)
    torch.cuda.synchronize()
    assert ws.intact(), "the workspace was written outside lion_emd_workspace_bytes"
    for n, g in bufs.items():
        assert g.intact(), f"{n} was written outside its bounds"
        assert bool(torch.isfinite(g.view).all()), f"{n} was not fully written"
    return {n: g.bits() for n, g in bufs.items()}


@pytest.mark.parametrize("N,M", [(5, 1), (65, 63), (257, 255)])
def test_outputs_and_workspace_stay_in_bounds_and_ignore_what_they_held(N, M):
    case = next(c for c in er.CASES if (c.N, c.M) == (N, M))
    x1, x2 = (dev(v) for v in batch_of(case, 2))
    gc = dev(GC[:2])
    from_nan = guarded_run(x1, x2, gc, float("nan"))
    from_zero = guarded_run(x1, x2, gc, 0.0)
    for n in from_nan:
        assert torch.equal(from_nan[n], from_zero[n]), f"{n} depends on what the buffers held before the call"
    plain = everything(x1, x2, gc)
    for n, t in zip(("match", "cost", "g1", "g2", "fast"), plain):
        assert torch.equal(t.reshape(-1).view(torch.int32), from_nan[n]), f"{n} differs from the unguarded run"


def test_rejections_are_taken_on_the_host_and_write_nothing():
    """a workspace one byte short; B, N or M <= 0: each raises before any launch"""
    B, N, M = 2, 65, 63
    case = next(c for c in er.CASES if (c.N, c.M) == (N, M))
    x1, x2 = (dev(v) for v in batch_of(case, B))
    gc = dev(GC[:B])
    nbytes = lib().load().lion_emd_workspace_bytes(B, N, M)
    ws = Guarded(nbytes // 4, 0.0)
    ws.whole.fill_(SENT)
    match, cost, g1, g2 = (Guarded(k, 0.0) for k in (B * M * N, B, B * N * 3, B * M * 3))
    for g in (match, cost, g1, g2):
        g.whole.fill_(SENT)
    given = dev(np.zeros((B, M, N), f32))

    def entry_points(b, n, m, size):
        return (("lion_emd_approxmatch", x1, x2, b, n, m, match.view, ws.view, size),
                ("lion_emd_cost", x1, x2, b, n, m, cost.view, ws.view, size),
                ("lion_emd_matchcost", x1, x2, given, b, n, m, cost.view, ws.view, size),
                ("lion_emd_matchcost_backward", gc, x1, x2, given, b, n, m, g1.view, g2.view))

    for args in entry_points(B, N, M, nbytes - 1)[:3]:
        with pytest.raises(RuntimeError, match="LION_EWORKSPACE"):
            call(*args)
    for b, n, m in ((0, N, M), (B, 0, M), (B, N, 0), (-1, N, M), (B, -5, M), (B, N, -1)):
        assert lib().load().lion_emd_workspace_bytes(b, n, m) == 0
        for args in entry_points(b, n, m, nbytes):
            with pytest.raises(RuntimeError, match="LION_EINVAL"):
                call(*args)
    torch.cuda.synchronize()
    for g in (ws, match, cost, g1, g2):
        assert bool((g.whole == SENT).all())
