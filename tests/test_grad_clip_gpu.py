"""Global gradient-norm clipping inside lion_amd.optim.Adam (csrc/optim.hip: grad_sqnorm_kernel -> grad_clip_coef_kernel ->
adam_multi_kernel<true>) -- what the reference's trainers do with torch.nn.utils.clip_grad_norm_ in front of optimizer.step()
(trainers/hvae_trainer.py:124-126, train_2prior.py:336-339).

The norm is checked against float64; the update is checked BIT FOR BIT against the unclipped optimizer fed with gradients that
torch scaled by the coefficient formed from the reported norm (so the two checks do not lean on each other); then against
clip_grad_norm_ + torch.optim.Adam end to end, with non-finite gradients, across param groups and inside captured steps."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

# tests/test_optim_gpu.py::_params plus one and two exact chunks: one element, a sub-wave tensor, a chunk edge +1 / exactly / x2,
# multi-chunk tensors with tails
SHAPES = [(1,), (7,), (33, 5), (4097,), (64, 64, 3, 3, 3), (100001,), (2, 3, 4, 5), (256, 35, 1, 1), (4096,), (8192,)]


def _params(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, device="cuda", generator=g) * 0.5) for s in SHAPES]


def _grads(params, step, seed, skip=(), scales=None):
    """tests/test_optim_gpu.py::_grads: every other gradient is a view at a 4-byte offset of a larger buffer (the scalar path)"""
    g = torch.Generator(device="cuda").manual_seed(1000 * seed + step)
    out = []
    for i, p in enumerate(params):
        if i in skip:
            out.append(None)
            continue
        big = torch.randn(p.numel() + 3, device="cuda", generator=g)
        if scales is not None:
            big *= scales[i]
        out.append(big[1:1 + p.numel()].view_as(p) if i % 2 else big[:p.numel()].view_as(p).clone())
    return out


def _norm64(grads):
    return torch.cat([g.double().flatten() for g in grads if g is not None]).norm().item()


def _coef(norm, max_norm):
    """clip_grad_norm_'s coefficient from a given fp32 norm, in torch fp32 with a true division (both operands tensors)"""
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32, device="cuda") / (norm + 1e-6), max=1.0)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _assert_same_state(oa, pa, ob, pb, ema):
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(_bits(a), _bits(b)), (i, "param")
        sa, sb = oa.state.get(a, {}), ob.state.get(b, {})
        assert set(sa) == set(sb), i
        for k in ("exp_avg", "exp_avg_sq", "step") + (("ema",) if ema else ()):
            if k in sa:
                assert torch.equal(_bits(sa[k]), _bits(sb[k])), (i, k)


# N(0,1) gradients of all ten tensors have norm ~486 (236231 elements), ~369 with tensors 2 and 5 skipped
STEP_SCALE = (0.5, 2.0, 0.5, 2.0, 2.0, 0.5)
MAX_NORM = 500.0


@pytest.mark.parametrize("spread", [False, True], ids=["normal", "scales_1e-6_to_1e6"])
def test_norm_matches_float64_and_repeats_bit_for_bit(spread):
    """relative error <= 2e-6: a sum of non-negative terms through d fp32 roundings is off by at most d 2^-24; d = 24 here (one
    square, a run of 16, a tree of 8), the square root halves it: ~8e-7.  2e-6 fails a serial fp32 sum over a tensor."""
    from lion_amd.optim import Adam
    ps = _params(3)
    scales = [10.0 ** e for e in torch.linspace(-6, 6, len(ps)).tolist()] if spread else None
    grads = _grads(ps, 0, 21, scales=scales)
    opt = Adam(ps, lr=1e-3, max_grad_norm=1.0)
    assert opt.grad_norm is None
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()
    first = opt.grad_norm.clone()
    opt.step()
    second = opt.grad_norm.clone()
    ref = _norm64(grads)
    got = float(first)
    print(f"grad_norm {got!r} float64 {ref!r} rel {abs(got - ref) / ref:.3e}")
    assert first.dim() == 0 and first.dtype == torch.float32 and first.is_cuda
    assert abs(got - ref) <= 2e-6 * ref
    assert torch.equal(_bits(first), _bits(second))


@pytest.mark.parametrize("wd,ema,skipping", [(0.0, 0.0, False), (0.01, 0.999, False), (0.01, 0.0, True), (0.0, 0.999, True)])
def test_update_given_the_norm_is_bit_exact(wd, ema, skipping):
    """the clipped optimizer == the unclipped one on g * coef, coef formed by torch from the reported norm: p, both moments, the
    step counts and the moving average after 4 steps, some of which clip and some of which do not"""
    from lion_amd.optim import Adam
    from lion_amd.training import EMA
    pa, pb = _params(3), _params(3)
    oa = Adam(pa, lr=3e-3, betas=(0.9, 0.99), weight_decay=wd, max_grad_norm=MAX_NORM)
    ob = Adam(pb, lr=3e-3, betas=(0.9, 0.99), weight_decay=wd)
    if ema:
        oa, ob = EMA(oa, ema), EMA(ob, ema)
        assert oa.grad_norm is None and ob.grad_norm is None
    norms = []
    for step in range(4):
        skip = (2, 5) if skipping and step in (1, 2) else ()
        grads = _grads(pa, step, 7, skip, scales=[STEP_SCALE[step]] * len(pa))
        kept = [None if g is None else g.clone() for g in grads]
        for p, g in zip(pa, grads):
            p.grad = g
        oa.step()
        norm = oa.grad_norm.clone()
        assert abs(float(norm) - _norm64(grads)) <= 2e-6 * _norm64(grads)
        for g, k in zip(grads, kept):                      # p.grad is left as it was: the clipped gradient lives in registers
            assert g is None or torch.equal(g, k)
        coef = _coef(norm, MAX_NORM)
        for p, g in zip(pb, grads):
            p.grad = None if g is None else g * coef
        ob.step()
        norms.append(float(norm))
    assert any(n > MAX_NORM for n in norms) and any(n < MAX_NORM for n in norms), norms
    inner_a, inner_b = (oa.optimizer, ob.optimizer) if ema else (oa, ob)
    _assert_same_state(inner_a, pa, inner_b, pb, bool(ema))
    for i, a in enumerate(pa):
        assert float(inner_a.state[a]["step"]) == (2.0 if skipping and i in (2, 5) else 4.0)


def test_inactive_clip_is_a_no_op():
    from lion_amd.optim import Adam
    pa, pb = _params(3), _params(3)
    all_grads = [_grads(pa, step, 9, scales=[STEP_SCALE[step]] * len(pa)) for step in range(3)]
    big = 10.0 * max(_norm64(gs) for gs in all_grads)
    oa = Adam(pa, lr=3e-3, betas=(0.9, 0.99), weight_decay=0.01, max_grad_norm=big)
    ob = Adam(pb, lr=3e-3, betas=(0.9, 0.99), weight_decay=0.01, max_grad_norm=None)
    for grads in all_grads:
        kept = [g.clone() for g in grads]
        for ps, o in ((pa, oa), (pb, ob)):
            for p, g in zip(ps, grads):
                p.grad = g
            o.step()
        assert float(oa.grad_norm) < big / 9.0 and ob.grad_norm is None
        for g, k in zip(grads, kept):
            assert torch.equal(g, k)
    _assert_same_state(oa, pa, ob, pb, False)


def test_two_param_groups_share_one_global_norm():
    from lion_amd.optim import Adam
    pa, pb = _params(3), _params(3)

    def groups(ps):
        return [{"params": ps[0::2], "lr": 3e-3}, {"params": ps[1::2], "lr": 1e-3, "weight_decay": 0.01}]
    oa = Adam(groups(pa), betas=(0.9, 0.99), max_grad_norm=MAX_NORM)
    ob = Adam(groups(pb), betas=(0.9, 0.99))
    norms = []
    for step in range(3):
        skip = (3,) if step == 1 else ()
        grads = _grads(pa, step, 13, skip, scales=[STEP_SCALE[step]] * len(pa))
        for p, g in zip(pa, grads):
            p.grad = g
        oa.step()
        norm = oa.grad_norm.clone()
        ref = _norm64(grads)                               # over BOTH groups
        assert abs(float(norm) - ref) <= 2e-6 * ref, (step, float(norm), ref)
        coef = _coef(norm, MAX_NORM)
        for p, g in zip(pb, grads):
            p.grad = None if g is None else g * coef
        ob.step()
        norms.append(float(norm))
    assert any(n > MAX_NORM for n in norms) and any(n < MAX_NORM for n in norms), norms
    _assert_same_state(oa, pa, ob, pb, False)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_matches_clip_grad_norm_and_torch_adam(wd):
    """1e-5 max|ref|: the 2e-6 of tests/test_optim_gpu.py plus the second moment's sensitivity to two coefficients that are each
    within 2e-6 of exact (2 x 4e-6)"""
    from lion_amd.optim import Adam
    pa, pb = _params(3), _params(3)
    oa = Adam(pa, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, max_grad_norm=MAX_NORM)
    ob = torch.optim.Adam(pb, lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd, foreach=False, fused=False)
    clipped = []
    for step in range(6):
        skip = (2, 5) if step in (1, 2) else ()
        for ps in (pa, pb):
            for p, g in zip(ps, _grads(ps, step, 7, skip, scales=[STEP_SCALE[step]] * len(ps))):
                p.grad = g
        oa.step()
        total = torch.nn.utils.clip_grad_norm_(pb, MAX_NORM)
        ob.step()
        assert abs(float(oa.grad_norm) - float(total)) <= 4e-6 * float(total)
        clipped.append(float(total) > MAX_NORM)
    assert any(clipped) and not all(clipped)
    for i, (a, b) in enumerate(zip(pa, pb)):
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"])
        for name, x, y in (("param", a, b), ("exp_avg", sa["exp_avg"], sb["exp_avg"]), ("exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"])):
            err = (x.detach() - y.detach()).abs().max().item()
            assert err <= 1e-5 * max(y.detach().abs().max().item(), 1e-6), (i, name, err)


def test_non_finite_gradient_follows_torch():
    """one +inf element: the norm is inf, the coefficient 0, g * 0 is NaN at that element and (signed) zero elsewhere -- as
    clip_grad_norm_(error_if_nonfinite=False) leaves it; nothing raises"""
    from lion_amd.optim import Adam
    pa, pb = _params(3), _params(3)
    oa = Adam(pa, lr=3e-3, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=0.999, max_grad_norm=MAX_NORM)
    ob = Adam(pb, lr=3e-3, betas=(0.9, 0.99), weight_decay=0.01, ema_decay=0.999)
    for step in range(3):
        grads = _grads(pa, step, 17)
        if step == 1:
            grads[4].view(-1)[70001] = float("inf")
        for p, g in zip(pa, grads):
            p.grad = g
        oa.step()
        norm = oa.grad_norm.clone()
        if step == 1:
            assert float(norm) == float("inf")
        coef = _coef(norm, MAX_NORM)
        for p, g in zip(pb, grads):
            p.grad = g * coef
        ob.step()
    _assert_same_state(oa, pa, ob, pb, True)
    assert bool(torch.isnan(pa[4].detach().view(-1)[70001])) and int(torch.isnan(pa[4].detach()).sum()) == 1
    assert not any(bool(torch.isnan(p.detach()).any()) for i, p in enumerate(pa) if i != 4)


def test_plan_follows_a_loaded_state_dict():
    """step(); load_state_dict(); step() under gradients that stay where they are: the pointer table must be rewritten for the
    replaced moments and step counts (its key holds their addresses)"""
    from lion_amd.optim import Adam
    pa, pb, pc = _params(3), _params(3), _params(5)
    oa = Adam(pa, lr=3e-3, betas=(0.9, 0.99))
    ob = torch.optim.Adam(pb, lr=3e-3, betas=(0.9, 0.99), foreach=False, fused=False)
    oc = torch.optim.Adam(pc, lr=3e-3, betas=(0.9, 0.99), foreach=False, fused=False)
    for step in range(2):
        for p, g in zip(pc, _grads(pc, step, 23)):
            p.grad = g
        oc.step()
    for ps in (pa, pb):
        for p in ps:
            p.grad = torch.zeros_like(p)                   # the gradients keep their addresses over both steps

    def both_step(step):
        for ps, o in ((pa, oa), (pb, ob)):
            for p, g in zip(ps, _grads(ps, step, 29)):
                p.grad.copy_(g)
            o.step()
    both_step(0)
    for o in (oa, ob):
        o.load_state_dict(copy.deepcopy(oc.state_dict()))
    both_step(1)
    for i, (a, b) in enumerate(zip(pa, pb)):
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]) == 3.0
        for name, x, y in (("param", a, b), ("exp_avg", sa["exp_avg"], sb["exp_avg"]), ("exp_avg_sq", sa["exp_avg_sq"], sb["exp_avg_sq"])):
            err = (x.detach() - y.detach()).abs().max().item()
            assert err <= 2e-6 * max(y.detach().abs().max().item(), 1e-6), (i, name, err)


def test_clip_inside_captured_training_steps():
    """the harness of tests/test_optim_gpu.py::test_adam_inside_captured_training_steps with max_grad_norm: the clip lives inside
    opt.step(), so it runs after averager.finish() in every mode and inside the optimizer graph in split mode.  The targets of
    every other step are ten times larger, which spreads the gradient norms; max_grad_norm is the geometric mean of the extremes
    of an unclipped probe run (Adam's update barely depends on a common factor of the gradients, so the clipped runs see nearly
    the same norms)."""
    from lion_amd.dist import BucketedGradAverager
    from lion_amd.optim import Adam
    from lion_amd.training import GraphedTrainStep

    def run(mode, max_norm):
        torch.manual_seed(3)
        net = torch.nn.Sequential(torch.nn.Linear(16, 64), torch.nn.Tanh(), torch.nn.Linear(64, 4)).cuda()
        unused = torch.nn.Parameter(torch.ones(7, device="cuda"))
        params = list(net.parameters()) + [unused]
        opt = Adam(params, lr=1e-2, betas=(0.9, 0.99), weight_decay=1e-3, max_grad_norm=max_norm)
        avg = BucketedGradAverager(params, bucket_bytes=2048)
        gen = torch.Generator(device="cuda").manual_seed(5)
        xs = [torch.randn(32, 16, device="cuda", generator=gen) for _ in range(8)]
        ys = [torch.randn(32, 4, device="cuda", generator=gen) * (10.0 if i % 2 else 1.0) for i in range(8)]
        norms = []

        def fb(x, y):
            avg.zero_grad()
            loss = ((net(x) - y) ** 2).mean()
            loss.backward()
            return loss.detach(), None
        if mode == "reference":
            for i in range(3, 8):
                fb(xs[i], ys[i])
                avg.finish()
                opt.step()
                norms.append(opt.grad_norm.clone())
            torch.cuda.synchronize()
            return None, [p.detach().clone() for p in net.parameters()], norms
        st = GraphedTrainStep(fb, {"x": xs[0].clone(), "y": ys[0].clone()}, params, opt, avg, mode=mode, warmup=3)
        for i in range(3, 8):
            st(x=xs[i], y=ys[i])
            norms.append(opt.grad_norm.clone())
        torch.cuda.synchronize()
        assert unused.grad is None and torch.equal(unused.detach(), torch.ones(7, device="cuda")) and unused not in opt.state
        return st, [p.detach().clone() for p in net.parameters()], norms

    _, _, probe = run("reference", 1e30)
    probe = [float(n) for n in probe]
    max_norm = (min(probe) * max(probe)) ** 0.5
    assert max(probe) > 2.0 * max_norm
    st_w, p_w, n_w = run("whole", max_norm)
    st_s, p_s, n_s = run("split", max_norm)
    _, p_r, n_r = run("reference", max_norm)
    assert st_w.mode == "whole" and len(st_w._graphs) == 1, st_w.launch
    assert st_s.mode == "split" and len(st_s._graphs) == 2, st_s.launch
    for norms in (n_w, n_s, n_r):
        vals = [float(n) for n in norms]
        assert any(v > max_norm for v in vals) and any(v < max_norm for v in vals), (vals, max_norm)
    for a, b, c in zip(n_w, n_s, n_r):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b, c in zip(p_w, p_s, p_r):
        assert torch.equal(a, b) and torch.equal(a, c)
