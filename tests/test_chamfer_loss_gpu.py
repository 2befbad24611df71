"""-m gpu: the Chamfer reconstruction losses (lion_amd.chamfer3d.chamfer_loss, `ddpm.loss_type` 'chamfer' / 'cd_sum';
utils/model_helper.py:43-52) -- csrc/chamfer.hip: chamfer_fwd_kernel + chamfer_loss_reduce_kernel, chamfer_loss_bwd_kernel.

References and bounds (u = 2^-24, the unit roundoff of fp32):
* float64 from the fp32 inputs.  A comparison against it is only meaningful where fp32 picks the same nearest neighbours, so
  every such test first asserts that the indices the op saved equal the float64 arg-mins for EVERY point (a condition of the
  test, not a tolerance), and that they equal the oracle's.
* loss: |loss - loss64| <= (P + 8) u loss64, P = ceil(max(N, M) / 256) the longest fp32 chain of a lane of the reduction;
  the 8 covers the roundings of a distance, of the scale and of the final cast.  All terms are >= 0: a bound, not a measurement.
* gradient, bit for bit: `_restate32` is the expression order documented in include/lion_hip.h, in numpy float32 (one rounding
  per operation): own term first, then the gathered terms in ascending index of the other cloud.
* gradient against float64, per component: |g - g64| <= (L_j + 6) u sum|terms_j|, L_j the number of gathered terms of
  receiver j (each term: the rounding of its difference, of its coefficient's two products and of the scale, and of the
  product; L_j additions whose partial sums are bounded by sum|terms_j|), magnitudes from the float64 evaluation.
* against the existing operator (chamfer_3DDist + mean + autograd, float atomics): both are fp32 evaluations of the same
  quantity, so twice the bounds above."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LANES = 256          # CHL_LANES of csrc/chamfer.hip
# both sides of the 256-receiver workgroup edge, of the 1024-point LDS tile edge and of the forward's 256-target per-wave
# quarter, in both roles; single-point clouds; the workload's own size
SHAPES = [(3, 257, 1025), (2, 1025, 257), (2, 2048, 2048), (1, 1, 5), (1, 5, 1), (2, 300, 300)]
HUB = (2, 257, 1025)


def _chain_P(n, m):
    return -(-max(n, m) // LANES)


def _scales(reduction, n, m):
    return (1.0 / n, 1.0 / m) if reduction == "mean" else (1.0, 1.0)


# ---- host references ------------------------------------------------------------------------------------------------
def _nn64(pred, target):
    """float64 squared distances of the fp32 inputs -> (dist1, idx1, dist2, idx2), lowest index on ties"""
    d1, i1, d2, i2 = [], [], [], []
    for p, t in zip(pred.astype(np.float64), target.astype(np.float64)):
        d = np.zeros((p.shape[0], t.shape[0]))
        for c in range(3):
            d += (p[:, None, c] - t[None, :, c]) ** 2
        i1.append(d.argmin(1)), d1.append(d.min(1)), i2.append(d.argmin(0)), d2.append(d.min(0))
    return np.stack(d1), np.stack(i1).astype(np.int32), np.stack(d2), np.stack(i2).astype(np.int32)


def _grad64(pred, target, idx1, idx2, gloss, s1, s2):
    """float64 gradient in gather form -> per cloud (g, sum|terms|, number of gathered terms) for pred and target"""
    out = []
    for xr, xo, ir, io, sr, so in ((pred, target, idx1, idx2, s1, s2), (target, pred, idx2, idx1, s2, s1)):
        xr, xo = xr.astype(np.float64), xo.astype(np.float64)
        g, mag, cnt = np.zeros_like(xr), np.zeros_like(xr), np.zeros(xr.shape[:2], np.int64)
        for b in range(xr.shape[0]):
            c_own, c_oth = 2.0 * float(gloss[b]) * sr, 2.0 * float(gloss[b]) * so
            own = c_own * (xr[b] - xo[b][ir[b]])
            oth = c_oth * (xr[b][io[b]] - xo[b])               # term k of the other cloud goes to receiver io[b][k]
            g[b], mag[b] = own, np.abs(own)
            np.add.at(g[b], io[b], oth)
            np.add.at(mag[b], io[b], np.abs(oth))
            np.add.at(cnt[b], io[b], 1)
        out.append((g, mag, cnt))
    return out


def _restate32(pred, target, idx1, idx2, gloss, s1, s2):
    """The kernel's documented expression order in numpy float32, one rounding per operation:
         c_own = 2 * (gloss[b] * s_own), c_oth = 2 * (gloss[b] * s_oth)
         acc[j] = c_own * (xr[j] - xo[ir[j]])                             own term first
         for k ascending:  acc[io[k]] = acc[io[k]] + c_oth * (xr[io[k]] - xo[k])
       -> (gpred, gtarget)"""
    f = np.float32
    out = []
    for xr, xo, ir, io, sr, so in ((pred, target, idx1, idx2, s1, s2), (target, pred, idx2, idx1, s2, s1)):
        assert xr.dtype == np.float32 and xo.dtype == np.float32
        g = np.empty_like(xr)
        for b in range(xr.shape[0]):
            c_own = f(2.0) * (f(gloss[b]) * f(sr))
            c_oth = f(2.0) * (f(gloss[b]) * f(so))
            acc = c_own * (xr[b] - xo[b][ir[b]])
            assert acc.dtype == np.float32
            for k in range(xo.shape[1]):
                j = io[b, k]
                acc[j] = acc[j] + c_oth * (xr[b, j] - xo[b, k])
            g[b] = acc
        out.append(g)
    return out


# ---- inputs and device runs, computed once per shape ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(shape):
    b, n, m = shape
    rng = np.random.default_rng(n * 10007 + m)
    pred = rng.random((b, n, 3), dtype=np.float32)
    target = rng.random((b, m, 3), dtype=np.float32)
    w = (0.5 + rng.random(b, dtype=np.float32)).astype(np.float32)
    return pred, target, w


@functools.lru_cache(maxsize=None)
def _hub_inputs():
    """one point of the prediction at the centre of the target's cube, the others 10 away: every target matches receiver 0
    (a chain of 1025 gathered terms across two LDS tiles), every other receiver has its own term only; roles swapped in the
    second pair"""
    b, n, m = HUB
    rng = np.random.default_rng(n * 10007 + m)
    pred = rng.random((b, n, 3), dtype=np.float32)
    target = rng.random((b, m, 3), dtype=np.float32)
    w = (0.5 + rng.random(b, dtype=np.float32)).astype(np.float32)
    pred[0, 0] = 0.5
    pred[0, 1:, 0] += 10.0
    target[1, 0] = 0.5
    target[1, 1:, 0] += 10.0
    return pred, target, w


@functools.lru_cache(maxsize=None)
def _ref64(key):
    pred, target, _ = _hub_inputs() if key == "hub" else _inputs(key)
    return _nn64(pred, target)


def _device_run(pred, target, w, reduction, target_grad=True):
    """-> loss, pred.grad, target.grad (None when not asked for), the (idx1, idx2) the op saved; all numpy"""
    from lion_amd.chamfer3d import chamfer_loss
    p = torch.from_numpy(pred).cuda().requires_grad_()
    t = torch.from_numpy(target).cuda()
    if target_grad:
        t.requires_grad_()
    loss = chamfer_loss(p, t, reduction)
    saved = loss.grad_fn.saved_tensors
    assert len(saved) == 4 and saved[2].dtype == torch.int32 and saved[3].dtype == torch.int32
    idx1, idx2 = saved[2].cpu().numpy(), saved[3].cpu().numpy()
    (loss * torch.from_numpy(w).cuda()).sum().backward()
    return (loss.detach().cpu().numpy(), p.grad.cpu().numpy(), None if t.grad is None else t.grad.cpu().numpy(), idx1, idx2)


@functools.lru_cache(maxsize=None)
def _run(key, reduction):
    return _device_run(*(_hub_inputs() if key == "hub" else _inputs(key)), reduction)


def _assert_indices(key, orc, idx1, idx2, float64=True):
    pred, target, _ = _hub_inputs() if key == "hub" else _inputs(key)
    _, _, o1, o2 = orc.chamfer_forward(pred, target)
    assert np.array_equal(idx1, o1) and np.array_equal(idx2, o2), "saved indices differ from the oracle's"
    if float64:
        _, r1, _, r2 = _ref64(key)
        assert np.array_equal(idx1, r1) and np.array_equal(idx2, r2), \
            "fp32 and float64 disagree on a nearest neighbour: the float64 comparison below would be meaningless"


def _check_loss(key, reduction, loss, factor=1.0):
    pred, target, _ = _hub_inputs() if key == "hub" else _inputs(key)
    n, m = pred.shape[1], target.shape[1]
    d1, _, d2, _ = _ref64(key)
    s1, s2 = _scales(reduction, n, m)
    loss64 = s1 * d1.sum(1) + s2 * d2.sum(1)
    bound = factor * (_chain_P(n, m) + 8) * U * loss64
    err = np.abs(loss.astype(np.float64) - loss64)
    print(f"loss {key} {reduction}: max err / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err, bound)


def _check_grad64(key, reduction, gpred, gtarget, idx1, idx2, factor=1.0):
    pred, target, w = _hub_inputs() if key == "hub" else _inputs(key)
    s1, s2 = _scales(reduction, pred.shape[1], target.shape[1])
    for name, got, (g64, mag, cnt) in zip(("pred", "target"), (gpred, gtarget), _grad64(pred, target, idx1, idx2, w, s1, s2)):
        bound = factor * (cnt[..., None] + 6) * U * mag
        err = np.abs(got.astype(np.float64) - g64)
        ok = err <= bound
        print(f"grad {name} {key} {reduction}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
        assert ok.all(), (name, np.argwhere(~ok)[:5], err[~ok][:5], bound[~ok][:5])


def _check_bits(key, reduction, gpred, gtarget, idx1, idx2):
    pred, target, w = _hub_inputs() if key == "hub" else _inputs(key)
    s1, s2 = _scales(reduction, pred.shape[1], target.shape[1])
    r_pred, r_target = _restate32(pred, target, idx1, idx2, w, s1, s2)
    assert np.array_equal(gpred, r_pred), np.argwhere(gpred != r_pred)[:5]
    assert np.array_equal(gtarget, r_target), np.argwhere(gtarget != r_target)[:5]


# ---- 1: loss value ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_loss_against_float64(orc, shape, reduction):
    loss, _, _, idx1, idx2 = _run(shape, reduction)
    assert loss.shape == (shape[0],) and loss.dtype == np.float32
    _assert_indices(shape, orc, idx1, idx2)
    _check_loss(shape, reduction, loss)


# ---- 2: gradient, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradient_is_the_documented_expression_bit_for_bit(orc, shape, reduction):
    loss, gpred, gtarget, idx1, idx2 = _run(shape, reduction)
    _assert_indices(shape, orc, idx1, idx2, float64=False)
    _check_bits(shape, reduction, gpred, gtarget, idx1, idx2)
    # a target that does not require a gradient gets none (its direction is not launched); the prediction's keeps its bits
    loss_b, gpred_b, gtarget_b, _, _ = _device_run(*_inputs(shape), reduction, target_grad=False)
    assert gtarget_b is None
    assert np.array_equal(gpred_b, gpred) and np.array_equal(loss_b, loss)


# ---- 3: gradient against float64 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradient_against_float64(orc, shape, reduction):
    _, gpred, gtarget, idx1, idx2 = _run(shape, reduction)
    _assert_indices(shape, orc, idx1, idx2)
    _check_grad64(shape, reduction, gpred, gtarget, idx1, idx2)


# ---- 4: hub and orphan ------------------------------------------------------------------------------------------------
def test_hub_and_orphans(orc):
    from lion_amd.chamfer3d import chamfer_loss
    pred, target, w = _hub_inputs()
    b, n, m = HUB
    for reduction in ("mean", "sum"):
        loss, gpred, gtarget, idx1, idx2 = _run("hub", reduction)
        _assert_indices("hub", orc, idx1, idx2)
        assert (idx2[0] == 0).all() and (idx1[1] == 0).all()     # every point of the other cloud matches receiver 0
        _check_loss("hub", reduction, loss)
        _check_bits("hub", reduction, gpred, gtarget, idx1, idx2)
        _check_grad64("hub", reduction, gpred, gtarget, idx1, idx2)
    # the same bits on every run
    p = torch.from_numpy(pred).cuda().requires_grad_()
    t = torch.from_numpy(target).cuda().requires_grad_()
    wd = torch.from_numpy(w).cuda()
    runs = []
    for _ in range(5):
        p.grad = t.grad = None
        loss = chamfer_loss(p, t, "mean")
        (loss * wd).sum().backward()
        runs.append((loss.detach().clone(), p.grad.clone(), t.grad.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b_) for a, b_ in zip(r, runs[0]))
    assert np.array_equal(runs[0][1].cpu().numpy(), _run("hub", "mean")[1])


# ---- 5: agreement with the existing operator --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_agrees_with_the_existing_operator(orc, shape):
    from lion_amd.chamfer3d import chamfer_3DDist
    pred, target, w = _inputs(shape)
    loss, gpred, gtarget, idx1, idx2 = _run(shape, "mean")
    _assert_indices(shape, orc, idx1, idx2)
    p = torch.from_numpy(pred).cuda().requires_grad_()
    t = torch.from_numpy(target).cuda().requires_grad_()
    d1, d2, i1, i2 = chamfer_3DDist()(p, t)
    old = d1.mean(1) + d2.mean(1)
    (old * torch.from_numpy(w).cuda()).sum().backward()
    assert np.array_equal(i1.cpu().numpy(), idx1) and np.array_equal(i2.cpu().numpy(), idx2)
    # each of the two is within the float64 bound: their difference within twice it
    _check_loss(shape, "mean", old.detach().cpu().numpy(), factor=2.0)
    _check_grad64(shape, "mean", p.grad.cpu().numpy(), t.grad.cpu().numpy(), idx1, idx2, factor=2.0)
    n, m = shape[1:]
    d64_1, _, d64_2, _ = _ref64(shape)
    loss64 = d64_1.mean(1) + d64_2.mean(1)
    assert (np.abs(loss.astype(np.float64) - old.detach().cpu().numpy()) <= 2 * (_chain_P(n, m) + 8) * U * loss64).all()
    s1, s2 = _scales("mean", n, m)
    for got, other, (_, mag, cnt) in zip((gpred, gtarget), (p.grad, t.grad), _grad64(pred, target, idx1, idx2, w, s1, s2)):
        diff = np.abs(got.astype(np.float64) - other.cpu().numpy())
        assert (diff <= 2 * (cnt[..., None] + 6) * U * mag).all()


# ---- 6: capture ------------------------------------------------------------------------------------------------
def test_captured_step_equals_the_eager_step_bit_for_bit():
    """GraphedTrainStep around a toy whose loss is the Chamfer loss: one graph, eager, and the plain loop leave identical
    losses and parameters after three steps -- possible only because the gradient has no atomics -- and the capture did
    not fall back."""
    from lion_amd.chamfer3d import chamfer_loss
    from lion_amd.dist import BucketedGradAverager
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
            loss = (chamfer_loss(net(x).view(B, NP, 3), y, "mean") * w).mean()
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


# ---- 7: VAE step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type,reduction", [("chamfer", "mean"), ("cd_sum", "sum")])
def test_vae_train_step_with_a_chamfer_reconstruction(loss_type, reduction):
    """one training step of the VAE with ddpm.loss_type = 'chamfer' / 'cd_sum'.  The loss itself runs under strict mode (no
    vendor-library path); the whole step cannot at this size: the VAE's own 1x1 convolutions on 16 columns leave the
    library's kernels in training whatever the loss is, so strict mode around the step was not checked."""
    from lion_amd import _fallback
    from lion_amd.chamfer3d import chamfer_loss
    from lion_amd.config import released_prior_cfg
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
    loss, out = vae_train_step(vae, opt, x, step=0)
    assert torch.isfinite(loss) and 'msg/kl' in out
    was = _fallback.strict()
    _fallback.reset()
    _fallback.strict(True)
    try:
        p = out['x_0_pred'].detach().clone().requires_grad_()
        again = chamfer_loss(p, x, reduction).mean()
        again.backward()
    finally:
        _fallback.strict(was)
    assert _fallback.counts() == {}
    assert torch.equal(out['rec_loss'].detach(), again.detach()), (out['rec_loss'], again)
    assert torch.isfinite(p.grad).all() and bool(p.grad.any())
    assert not torch.equal(w0, vae.decoder.layers.classifier[2].weight)
