"""-m gpu: the EMD reconstruction loss (lion_amd.emd.emd_loss, `ddpm.loss_type` 'emd' / 'chamfer_emd';
utils/model_helper.py:82-96) -- csrc/emd.hip: lion_emd_loss_forward (emd_pass1_kernel, emd_pass2_kernel<G2>,
emd_pass3_cost_kernel<., G1, NEXT>: pass 3 with the next level's pass 1, emd_costrow_sum_kernel<true>) and
lion_emd_loss_backward.

Numeric comparisons run on the certified inputs of tests/emd_ref.py only (CASES: every row / quarter / tile edge of the
kernels, multiL / multiR != 1, offset coordinates, a vanishing cost), at B = 2 with the certified pair in slot 1, in three
layers, so that conditioning of the auction enters the last one alone:
1. the auction: the workspace state after lion_emd_loss_forward equals lion_emd_approxmatch's bit for bit (no tolerance);
2. cost and gradients as linear functionals of THAT auction: float64 on the fp32 match lion_emd_approxmatch materialises,
   bounds (T + 8) 2^-24 of the sums of absolute products (emd_ref.linear_bound) with T = the longest fp32 chain + 24: M terms
   per row (+ ceil(N / 256) of the row sum) for loss * N and g1u, N per column for g2u; the 24 covers the 10-level accumulation
   on either side (9 additions in match, 9 in the op's own sums), the roundings of a distance and of the weight products, the
   factor 2 * ratioR and the division by N -- operation counts, not measurements;
3. end to end against the float64 auction, the project's tolerances (cost 1e-4 + floor, gradients 2e-3 of their maximum).
Everything the header promises without a tolerance is compared bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

import emd_ref as er
from test_emd_numerics_gpu import GC, IDS, SENT, Guarded, batch_of, call, cost_bound, lib, out, report, workspace
from test_pointwise_numerics_gpu import dev, host

pytestmark = pytest.mark.gpu

f32 = np.float32


def loss_forward(x1, x2, g1=True, g2=True):
    """-> loss [B], g1u [B,N,3] | None, g2u [B,M,3] | None, the workspace; every buffer NaN-filled before the call"""
    B, N, M = x1.shape[0], x1.shape[1], x2.shape[1]
    loss, g1u, g2u = out(B), out(B, N, 3) if g1 else None, out(B, M, 3) if g2 else None
    ws, nbytes = workspace(B, N, M)
    call("lion_emd_loss_forward", x1, x2, B, N, M, loss, g1u, g2u, ws, nbytes)
    return loss, g1u, g2u, ws


def loss_backward(gloss, g1u, g2u, N, M):
    B = gloss.shape[0]
    gx1 = None if g1u is None else out(B, N, 3)
    gx2 = None if g2u is None else out(B, M, 3)
    call("lion_emd_loss_backward", gloss, g1u, g2u, B, N, M, gx1, gx2)
    return gx1, gx2


def auction_state(ws, B, N, M):
    """remainL, remainR, ratioL, ratioR: the first B (2N + 2M) floats of the workspace, as bit patterns"""
    return ws.view(torch.int32)[:B * (2 * N + 2 * M)].clone()


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _run(case):
    """the op (both gradients) and lion_emd_approxmatch on the case's batch of 2, once per case"""
    N, M = case.N, case.M
    x1, x2 = batch_of(case, 2)
    d1, d2 = dev(x1), dev(x2)
    loss, g1u, g2u, ws = loss_forward(d1, d2)
    match = out(2, M, N)
    ws_a, nbytes = workspace(2, N, M)
    call("lion_emd_approxmatch", d1, d2, 2, N, M, match, ws_a, nbytes)
    gx1, gx2 = loss_backward(dev(GC[:2]), g1u, g2u, N, M)
    return dict(x1=x1, x2=x2, loss=host(loss), g1u=host(g1u), g2u=host(g2u), gx1=host(gx1), gx2=host(gx2),
                state=auction_state(ws, 2, N, M).cpu(), state_approx=auction_state(ws_a, 2, N, M).cpu(), match=host(match),
                loss_bits=bits(loss).cpu(), g1u_bits=bits(g1u).cpu(), g2u_bits=bits(g2u).cpu())


# ---- 1: the auction, bit for bit -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_auction_state_equals_approxmatch_bit_for_bit(case):
    r = _run(case)
    assert r["state"].numel() == 2 * (2 * case.N + 2 * case.M)
    assert torch.equal(r["state"], r["state_approx"])
    assert np.all(np.isfinite(r["state"].view(torch.float32).numpy()))           # and it was written in full (NaN before)


# ---- 2: cost and gradients as linear functionals of that auction -------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_cost_and_gradients_are_linear_in_the_materialised_match(case):
    r = _run(case)
    N, M = case.N, case.M
    for b in range(2):
        m64 = r["match"][b].astype(np.float64)
        c64, absprod = er.matchcost64(r["x1"][b], r["x2"][b], m64)
        g1, g2, a1, a2 = er.grads64(1.0, r["x1"][b], r["x2"][b], m64)
        report(f"emd loss * N {case.id} slot {b}", abs(float(r["loss"][b]) * N - c64),
               er.linear_bound(M + math.ceil(N / 256) + 24, absprod))
        report(f"emd loss g1u {case.id} slot {b}", np.abs(r["g1u"][b] - g1), er.linear_bound(M + 24, a1))
        report(f"emd loss g2u {case.id} slot {b}", np.abs(r["g2u"][b] - g2), er.linear_bound(N + 24, a2))


# ---- 3: end to end against the float64 auction -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_loss_and_gradients_against_float64(case):
    ref, r = er.reference(case), _run(case)
    N = case.N
    assert np.all(np.isfinite(r["loss"])) and np.all(r["loss"] >= 0)
    report(f"emd loss {case.id}", abs(float(r["loss"][1]) * N - ref["cost"]), cost_bound(ref, er.TOL_COST))
    c = float(GC[1]) / N
    gmax = abs(c) * max(np.abs(ref["g1"]).max(), np.abs(ref["g2"]).max())
    report(f"emd loss grad pred {case.id}", np.abs(r["gx1"][1] - c * ref["g1"]), er.TOL_GRAD * gmax)
    report(f"emd loss grad target {case.id}", np.abs(r["gx2"][1] - c * ref["g2"]), er.TOL_GRAD * gmax)
    # the backward's documented order, one rounding per operation: c = gloss[b] / (float)N, gxyz = c * gu
    c32 = (GC[:2] / f32(N)).astype(f32)
    assert c32.dtype == f32
    for gu, gx in ((r["g1u"], r["gx1"]), (r["g2u"], r["gx2"])):
        want = c32[:, None, None] * gu
        assert want.dtype == f32 and np.array_equal(want.view(np.int32), gx.view(np.int32))


# ---- 4: NULL directions -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in er.CASES if (c.N, c.M) in ((5, 1), (65, 63), (1023, 1025))], ids=lambda c: c.id)
def test_a_null_direction_changes_nothing_else(case):
    r = _run(case)
    N, M = case.N, case.M
    d1, d2 = dev(r["x1"]), dev(r["x2"])
    for g1, g2 in ((True, False), (False, True), (False, False)):
        loss, g1u, g2u, ws = loss_forward(d1, d2, g1, g2)
        assert torch.equal(bits(loss).cpu(), r["loss_bits"]), (g1, g2)
        assert torch.equal(auction_state(ws, 2, N, M).cpu(), r["state"]), (g1, g2)
        assert (g1u is None) == (not g1) and (g2u is None) == (not g2)
        if g1:
            assert torch.equal(bits(g1u).cpu(), r["g1u_bits"])
        if g2:
            assert torch.equal(bits(g2u).cpu(), r["g2u_bits"])
        if g1 or g2:
            gx1, gx2 = loss_backward(dev(GC[:2]), g1u, g2u, N, M)
            if g1:
                assert np.array_equal(host(gx1).view(np.int32), r["gx1"].view(np.int32))
            if g2:
                assert np.array_equal(host(gx2).view(np.int32), r["gx2"].view(np.int32))
    with pytest.raises(RuntimeError, match="LION_EINVAL"):
        call("lion_emd_loss_backward", dev(GC[:2]), None, None, 2, N, M, None, None)


# ---- 5: batch and run-to-run independence -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", er.CASES, ids=IDS)
def test_a_pair_computes_the_same_alone_in_a_batch_and_twice(case):
    x1, x2 = (dev(v) for v in batch_of(case, 3))
    whole = loss_forward(x1, x2)[:3]
    again = loss_forward(x1, x2)[:3]
    names = ("loss", "g1u", "g2u")
    for n, a, b in zip(names, whole, again):
        assert torch.equal(bits(a), bits(b)), f"{n}: two runs differ"
    assert torch.equal(bits(whole[0][2:]).cpu(), _run(case)["loss_bits"][1:])     # slot 2 of 3 == slot 1 of 2
    for i in range(3):
        alone = loss_forward(x1[i:i + 1].contiguous(), x2[i:i + 1].contiguous())[:3]
        for n, a, b in zip(names, whole, alone):
            assert torch.equal(bits(a[i:i + 1]), bits(b)), f"{n}: pair {i} of a batch of 3 differs from the pair alone"


# ---- 6: memory ------------------------------------------------------------------------------------------------------------------

def guarded_run(x1, x2, gc, fill):
    """forward and backward on guarded outputs and a guarded workspace of exactly lion_emd_workspace_bytes, all filled with
    `fill` before the call; -> the outputs' bit patterns"""
    B, N, M = x1.shape[0], x1.shape[1], x2.shape[1]
    nbytes = lib().load().lion_emd_workspace_bytes(B, N, M)
    assert nbytes % 4 == 0
    ws = Guarded(nbytes // 4, fill)
    bufs = {n: Guarded(k, fill) for n, k in (("loss", B), ("g1u", B * N * 3), ("g2u", B * M * 3), ("gx1", B * N * 3),
                                             ("gx2", B * M * 3))}
    v = {n: g.view for n, g in bufs.items()}
    call("lion_emd_loss_forward", x1, x2, B, N, M, v["loss"], v["g1u"], v["g2u"], ws.view, nbytes)
    call("lion_emd_loss_backward", gc, v["g1u"], v["g2u"], B, N, M, v["gx1"], v["gx2"])
    torch.cuda.synchronize()
    assert ws.intact(), "the workspace was written outside lion_emd_workspace_bytes"
    for n, g in bufs.items():
        assert g.intact(), f"{n} was written outside its bounds"
        assert bool(torch.isfinite(g.view).all()), f"{n} was not fully written"
    return {n: g.bits() for n, g in bufs.items()}


@pytest.mark.parametrize("N,M", [(5, 1), (65, 63), (257, 255)])
def test_outputs_and_workspace_stay_in_bounds_and_ignore_what_they_held(N, M):
    case = next(c for c in er.CASES if (c.N, c.M) == (N, M))
    r = _run(case)
    x1, x2, gc = dev(r["x1"]), dev(r["x2"]), dev(GC[:2])
    from_nan = guarded_run(x1, x2, gc, float("nan"))
    from_zero = guarded_run(x1, x2, gc, 0.0)
    for n in from_nan:
        assert torch.equal(from_nan[n], from_zero[n]), f"{n} depends on what the buffers held before the call"
        assert np.array_equal(from_nan[n].cpu().numpy(), r[n].reshape(-1).view(np.int32)), f"{n} differs from the unguarded run"
    # a workspace one byte short is refused on the host and nothing is written
    nbytes = lib().load().lion_emd_workspace_bytes(2, N, M)
    ws = Guarded(nbytes // 4, 0.0)
    ws.whole.fill_(SENT)
    outs = [Guarded(k, 0.0) for k in (2, 2 * N * 3, 2 * M * 3)]
    for g in outs:
        g.whole.fill_(SENT)
    with pytest.raises(RuntimeError, match="LION_EWORKSPACE"):
        call("lion_emd_loss_forward", x1, x2, 2, N, M, *(g.view for g in outs), ws.view, nbytes - 1)
    torch.cuda.synchronize()
    for g in [ws] + outs:
        assert bool((g.whole == SENT).all())


# ---- 7: autograd and wiring ------------------------------------------------------------------------------------------------------

def test_autograd_gives_the_c_level_gradient_and_allocates_no_match_matrix():
    from lion_amd.emd import emd_loss
    case = next(c for c in er.CASES if (c.N, c.M) == (1025, 1023))
    r = _run(case)
    B, N, M = 2, case.N, case.M
    t, w = dev(r["x2"]), dev(GC[:2])
    p = dev(r["x1"]).requires_grad_()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = emd_loss(p, t)
    saved = [s for s in loss.grad_fn.saved_tensors if s is not None]
    assert len(saved) == 1 and saved[0].shape == (B, N, 3)                       # the prediction's gradient, nothing else
    (loss * w).sum().backward()
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < B * M * N * 4
    assert np.array_equal(host(loss).view(np.int32), r["loss"].view(np.int32))
    assert np.array_equal(host(p.grad).view(np.int32), r["gx1"].view(np.int32))
    assert t.grad is None
    # both directions when the target asks too; none without grad mode
    p2, t2 = dev(r["x1"]).requires_grad_(), dev(r["x2"]).requires_grad_()
    (emd_loss(p2, t2) * w).sum().backward()
    assert np.array_equal(host(p2.grad).view(np.int32), r["gx1"].view(np.int32))
    assert np.array_equal(host(t2.grad).view(np.int32), r["gx2"].view(np.int32))
    with torch.no_grad():
        quiet = emd_loss(p2, t2)
    assert quiet.grad_fn is None and torch.equal(quiet, loss.detach())
    # [B,3,N] storage behind a transposed view: made contiguous, and the gradient flows back into that storage
    pt = dev(np.ascontiguousarray(r["x1"].transpose(0, 2, 1))).requires_grad_()
    tt = dev(np.ascontiguousarray(r["x2"].transpose(0, 2, 1)))
    assert not pt.transpose(1, 2).is_contiguous()
    lt = emd_loss(pt.transpose(1, 2), tt.transpose(1, 2))
    (lt * w).sum().backward()
    assert torch.equal(lt.detach(), loss.detach()) and torch.equal(pt.grad.transpose(1, 2), p.grad)


def test_loss_fn_mixes_chamfer_and_emd_with_the_given_weight():
    from lion_amd.chamfer3d import chamfer_loss
    from lion_amd.emd import emd_loss
    from lion_amd.models.vae_adain import loss_fn
    case = next(c for c in er.CASES if (c.N, c.M) == (300, 200))
    x1, x2 = (dev(v) for v in batch_of(case, 2))
    assert torch.equal(loss_fn(x1, x2, 'emd', 3, 2), emd_loss(x1, x2))
    for w in (0.02, 0.37):
        got = loss_fn(x1.view(2, -1), x2.view(2, -1), 'chamfer_emd', 3, 2, loss_weight_emd=w)
        assert got.shape == (2,) and torch.equal(got, chamfer_loss(x1, x2, "mean") + w * emd_loss(x1, x2))
    assert torch.equal(loss_fn(x1, x2, 'chamfer_emd', 3, 2), loss_fn(x1, x2, 'chamfer_emd', 3, 2, loss_weight_emd=0.02))


# ---- 8: capture ------------------------------------------------------------------------------------------------------------------

def test_captured_step_equals_the_eager_step_bit_for_bit():
    """GraphedTrainStep around a toy whose loss is the EMD loss (B = 4, 64 predicted points against 96 target points): one
    graph, eager, and the plain loop leave identical losses and parameters after three steps, and the capture did not fall
    back"""
    from lion_amd.dist import BucketedGradAverager
    from lion_amd.emd import emd_loss
    from lion_amd.optim import Adam
    from lion_amd.training import GraphedTrainStep
    B, NP, NT = 4, 64, 96

    def run(mode):
        torch.manual_seed(3)
        net = torch.nn.Sequential(torch.nn.Linear(16, 64), torch.nn.Tanh(), torch.nn.Linear(64, 3 * NP)).cuda()
        params = list(net.parameters())
        opt = Adam(params, lr=1e-2, betas=(0.9, 0.99))
        avg = BucketedGradAverager(params, bucket_bytes=2048)
        gen = torch.Generator(device="cuda").manual_seed(5)
        xs = [torch.randn(B, 16, device="cuda", generator=gen) for _ in range(4)]
        ys = [torch.rand(B, NT, 3, device="cuda", generator=gen) for _ in range(4)]
        ws = [0.5 + torch.rand(B, device="cuda", generator=gen) for _ in range(4)]

        def fb(x, y, w):
            avg.zero_grad()
            loss = (emd_loss(net(x).view(B, NP, 3), y) * w).mean()
            loss.backward()
            return loss.detach(), None
        losses = []
        if mode == "reference":
            for i in range(1, 4):
                loss, _ = fb(xs[i], ys[i], ws[i])
                avg.finish()
                opt.step()
                losses.append(float(loss))
            torch.cuda.synchronize()
            return None, [p.detach().clone() for p in params], losses
        st = GraphedTrainStep(fb, {"x": xs[0].clone(), "y": ys[0].clone(), "w": ws[0].clone()}, params, opt, avg, mode=mode,
                              warmup=3)
        for i in range(1, 4):
            losses.append(float(st(x=xs[i], y=ys[i], w=ws[i])))
        torch.cuda.synchronize()
        return st, [p.detach().clone() for p in params], losses

    st_w, p_w, l_w = run("whole")
    st_e, p_e, l_e = run("off")
    _, p_r, l_r = run("reference")
    assert st_w.mode == "whole" and len(st_w._graphs) == 1, st_w.launch
    assert st_e.mode == "eager"
    assert l_w == l_e == l_r and all(np.isfinite(l_w))
    for a, b_, c in zip(p_w, p_e, p_r):
        assert torch.equal(a, b_) and torch.equal(a, c)


# ---- 9: VAE step -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss_type", ["emd", "chamfer_emd"])
def test_vae_train_step_with_an_emd_reconstruction(loss_type):
    """one training step of the VAE with ddpm.loss_type = 'emd' / 'chamfer_emd' (2 x 1024 points).  The loss itself runs
    under strict mode (no vendor-library path); the whole step cannot at this size, whatever the loss is (see
    test_vae_train_step_with_a_chamfer_reconstruction)."""
    from lion_amd import _fallback
    from lion_amd.chamfer3d import chamfer_loss
    from lion_amd.config import released_prior_cfg
    from lion_amd.emd import emd_loss
    from lion_amd.models.vae_adain import Model
    from lion_amd.optim import Adam
    from lion_amd.training import vae_train_step
    cfg = released_prior_cfg()
    cfg.data.tr_max_sample_points = 1024
    cfg.ddpm.dropout = 0.0
    cfg.sde.dropout = 0.0
    cfg.trainer.anneal_kl = 0
    cfg.ddpm.loss_type = loss_type
    torch.manual_seed(0)
    vae = Model(cfg).cuda()
    opt = Adam(vae.parameters(), lr=1e-4)
    x = torch.randn(2, 1024, 3, device="cuda") * 0.5
    w0 = vae.decoder.layers.classifier[2].weight.detach().clone()
    loss, res = vae_train_step(vae, opt, x, step=0)
    assert torch.isfinite(loss) and 'msg/kl' in res
    was = _fallback.strict()
    _fallback.reset()
    _fallback.strict(True)
    try:
        p = res['x_0_pred'].detach().clone().requires_grad_()
        again = emd_loss(p, x)
        if loss_type == 'chamfer_emd':
            again = chamfer_loss(p, x, "mean") + cfg.ddpm.loss_weight_emd * again
        again = again.mean()
        again.backward()
    finally:
        _fallback.strict(was)
    assert _fallback.counts() == {}
    assert torch.equal(res['rec_loss'].detach(), again.detach()), (res['rec_loss'], again)
    assert torch.isfinite(p.grad).all() and bool(p.grad.any())
    assert not torch.equal(w0, vae.decoder.layers.classifier[2].weight)


# ---- 10: the workload's size -----------------------------------------------------------------------------------------------------

def test_workload_size_runs_finite_and_repeats_its_bits():
    """32 x 2048^2, uniform clouds: finite results and equal bits on a second run -- no numeric comparison at this size (the
    auction's conditioning does not follow from the shape)"""
    from lion_amd.emd import emd_loss
    gen = torch.Generator(device="cuda").manual_seed(0)
    t = torch.rand(32, 2048, 3, device="cuda", generator=gen)
    x = torch.rand(32, 2048, 3, device="cuda", generator=gen)
    runs = []
    for _ in range(2):
        p = x.clone().requires_grad_()
        loss = emd_loss(p, t)
        loss.sum().backward()
        runs.append((loss.detach(), p.grad))
    assert bool(torch.isfinite(runs[0][0]).all()) and bool((runs[0][0] > 0).all()) and bool(torch.isfinite(runs[0][1]).all())
    assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))
