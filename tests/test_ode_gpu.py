"""-m gpu: the device RK45 of the probability-flow ODE (csrc/ode.hip, lion_amd/ode.py, lion_amd/diffusion_continuous.py)
against the float64 restatement of scipy's solver (tests/ode_oracle.py): kernels through the C ABI, whole solves of an
analytic denoiser and of the real priors, graph replay against the eager loop, the encode / sample round trip, the
two-prior ODE sampler, encode -> interpolate -> decode, and one continuous-time prior training step."""
import numpy as np
import pytest
import torch

import ode_oracle as oc

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _diff():
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion_continuous import make_diffusion
    return make_diffusion(released_prior_cfg().sde, device="cuda")


def _state(n, B, **ctrl):
    from lion_amd import ode
    st = ode.OdeState(n, B, "cuda")
    st.ctrl.copy_(torch.frombuffer(bytearray(ode.pack_ctrl(**ctrl)), dtype=torch.uint8))
    return st


def _ctrl(st):
    from lion_amd import ode
    torch.cuda.synchronize()
    return ode.unpack_ctrl(st.ctrl.cpu().numpy().tobytes())


def _phys(fslot):
    return [fslot] + [1, 2, 3, 4, 5] + [6 - fslot]


# ---- 1. kernels ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fslot", [0, 6])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_stage_kernel_matches_restatement(fslot, sign):
    rng = np.random.default_rng(fslot + (sign > 0))
    n, B = 32 * 128 + 3, 32
    Y, K = rng.standard_normal((2, n)), rng.standard_normal((7, n)) * 3
    t, h = -0.73125, 0.0137
    for ys in (0, 1):
        for s in range(1, 7):
            st = _state(n, B, t=t, h=h, stage=s, yslot=ys, fslot=fslot, sign=sign)
            st.Y.copy_(torch.from_numpy(Y))
            st.K.copy_(torch.from_numpy(K))
            st.stage()
            Kl = [K[r] for r in _phys(fslot)]
            v = oc.stage_state(Y[ys], Kl, h, s)
            assert np.array_equal(st.x32.cpu().numpy(), v.astype(np.float32)), s
            tm = np.float32(t + h) if s == 6 else np.float32(t + oc.C[s] * h)
            assert np.all(st.t_model.cpu().numpy() == (tm if sign > 0 else -tm))
            if s == 6:
                ynew = st.Y[1 - ys].cpu().numpy()
                assert np.all(np.abs(ynew - v) <= np.spacing(np.abs(v)))
            assert _ctrl(st)["cur"] == s


def _drift_oracle_setup(model, diff, shape, sign, cond=None, cm=False):
    """the ODE right-hand side for the float64 oracle: the model on the GPU, then the device drift (same fp32 arithmetic
    as inside a solve) -- 'the oracle driving the same drift'"""
    from lion_amd import ode
    B = shape[0]
    n = int(np.prod(shape))
    st = _state(n, B, sign=sign, stage=1, cur=1, fslot=0)
    sched, mix = diff.ode_scalars(), ode._mixing(model)
    cm = ode._channel_major(model, shape[1:])
    x = st.x32.view(shape)
    kw = {"channel_major_out": True} if cm else {}

    def fun(t, y):
        st.x32.copy_(torch.from_numpy(np.ascontiguousarray(y)).to("cuda", torch.float32))
        tf = np.float32(t)
        st.t_model.fill_(float(-tf if sign < 0 else tf))
        with torch.no_grad():
            eps = model(x=x, t=st.t_model, condition_input=cond, clip_feat=None, **kw)
        st.drift(eps, sched, mix, model.num_points if cm else 0)
        return st.K[1].cpu().numpy().copy()
    return fun


def test_drift_kernel_matches_the_reference_expression():
    """dx/dt of sample_model_ode's ode_func in float32 torch ops on the GPU, negated for the reversed span"""
    diff = _diff()
    g = torch.Generator(device="cuda").manual_seed(0)
    shape = (8, 128, 1, 1)
    y = torch.randn(shape, device="cuda", generator=g)
    eps = torch.randn(shape, device="cuda", generator=g)

    class Fixed(torch.nn.Module):
        def forward(self, x, t, **kw):
            return eps
    for t in (0.999, 0.5, 3e-3, 1e-5):
        for sign in (1.0, -1.0):
            fun = _drift_oracle_setup(Fixed(), diff, shape, sign)
            tt = torch.tensor(t, dtype=torch.float32, device="cuda")
            ref = diff.f(tt) * y + 0.5 * diff.g2(tt) * eps / torch.sqrt(diff.var(tt))
            got = fun(-t if sign < 0 else t, y.double().cpu().numpy().reshape(-1))
            want = (sign * ref).double().cpu().numpy().reshape(-1)
            np.testing.assert_array_max_ulp(got.astype(np.float32), want.astype(np.float32), maxulp=1)


def test_drift_kernel_mixing_and_channel_major_against_torch():
    """the mixed prediction (1 - sigmoid(logit)) sqrt(var) x + sigmoid(logit) eps, per latent element, and the local
    prior's channel-major [B, 4, N] output read for a point-major [B, N, 4] latent, against the torch expressions"""
    diff = _diff()
    g = torch.Generator(device="cuda").manual_seed(1)
    B, N = 3, 2048
    shape = (B, 4 * N, 1, 1)
    y = torch.randn(shape, device="cuda", generator=g)
    eps_cm = torch.randn(B, 4, N, device="cuda", generator=g)
    logit = torch.randn(1, 4 * N, 1, 1, device="cuda", generator=g) * 3

    class ChannelMajor(torch.nn.Module):
        num_points, num_classes = N, 4

        def __init__(self, mixed):
            super().__init__()
            self.mixed_prediction = mixed
            self.mixing_logit = torch.nn.Parameter(logit.clone()) if mixed else None

        def geometry_source(self, x):
            raise AssertionError("not used")

        def forward(self, x, t, channel_major_out=False, **kw):
            assert channel_major_out
            return eps_cm
    eps_pm = eps_cm.permute(0, 2, 1).reshape(shape)
    for mixed in (False, True):
        for t, sign in ((0.7, -1.0), (2e-3, 1.0)):
            fun = _drift_oracle_setup(ChannelMajor(mixed), diff, shape, sign)
            tt = torch.tensor(t, dtype=torch.float32, device="cuda")
            var = diff.var(tt)
            params = eps_pm
            if mixed:
                coeff = torch.sigmoid(logit)
                params = (1 - coeff) * diff.mixing_component(y, var, tt, True) + coeff * eps_pm
            ref = diff.f(tt) * y + 0.5 * diff.g2(tt) * params / torch.sqrt(var)
            got = fun(-t if sign < 0 else t, y.double().cpu().numpy().reshape(-1))
            want = (sign * ref).cpu().numpy().reshape(-1)
            np.testing.assert_array_max_ulp(got.astype(np.float32), want, maxulp=1)


def test_sample_model_ode_mixing_logit_override():
    """mixing_logit passed to sample_model_ode replaces the model's own, graphed and eager"""
    diff = _diff()

    class MixedGaussian(GaussianDenoiser):
        def __init__(self, logit):
            super().__init__(diff, 0.25)
            self.mixed_prediction = True
            self.mixing_logit = torch.nn.Parameter(logit)
    g = torch.Generator(device="cuda").manual_seed(4)
    other = torch.randn(1, 128, 1, 1, device="cuda", generator=g)
    a = MixedGaussian(torch.full((1, 128, 1, 1), -2.0, device="cuda"))
    b = MixedGaussian(other.clone())
    z = torch.randn(8, 128, 1, 1, device="cuda", generator=g)
    for graph in (False, True):
        xa, na, _ = diff.sample_model_ode(a, 8, [128, 1, 1], 1e-5, 1e-4, False, 1.0, noise=z, mixing_logit=other,
                                          graph=graph)
        xb, nb, _ = diff.sample_model_ode(b, 8, [128, 1, 1], 1e-5, 1e-4, False, 1.0, noise=z, graph=graph)
        xc, _, _ = diff.sample_model_ode(a, 8, [128, 1, 1], 1e-5, 1e-4, False, 1.0, noise=z, graph=graph)
        assert na == nb and torch.equal(xa, xb) and not torch.equal(xa, xc)


def _control_case(n, t, t_bound, h, en_scale, rejected, seed=0, h_abs=None):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((2, n))
    K = rng.standard_normal((7, n)) * en_scale
    st = _state(n, 4, t=t, t_bound=t_bound, direction=np.sign(t_bound - t), rtol=TOL, atol=TOL, h=h,
                h_abs=abs(h) if h_abs is None else h_abs, t_new=t + h, stage=6, step_rejected=int(rejected), sign=1.0)
    st.Y.copy_(torch.from_numpy(Y))
    st.K.copy_(torch.from_numpy(K))
    st.control()
    c = _ctrl(st)
    en = oc.error_norm(Y[0], Y[1], list(K), h, TOL, TOL)
    ok, factor = oc.step_factor(en, rejected)
    return c, en, ok, factor


def _next_attempt(t, t_bound, h_abs, new_step):
    direction = np.sign(t_bound - t)
    ms = oc.min_step(t, direction)
    if new_step:
        h_abs = max(h_abs, ms)
    if h_abs < ms:
        return None
    t_new = t + h_abs * direction
    if direction * (t_new - t_bound) > 0:
        t_new = t_bound
    return t_new - t, t_new


@pytest.mark.parametrize("case", ["zero", "accept", "reject", "accept_after_reject", "clip", "too_small"])
def test_error_norm_and_controller(case):
    n, t, tb, h = 32 * 8192, -1.0, -float(np.float32(1e-5)), 0.01
    if case == "zero":
        c, en, ok, f = _control_case(n, t, tb, h, 0.0, False)
        assert c["err_norm"] == 0.0
    elif case == "accept":
        c, en, ok, f = _control_case(n, t, tb, h, 1e-3, False)
    elif case == "reject":
        c, en, ok, f = _control_case(n, t, tb, h, 10.0, False)
    elif case == "accept_after_reject":
        c, en, ok, f = _control_case(n, t, tb, h, 1e-3, True)
        assert f == 1
    elif case == "clip":
        c, en, ok, f = _control_case(n, -0.02, tb, 0.0199, 1e-3, False)
    else:
        c, en, ok, f = _control_case(n, t, tb, 1.2e-15, 1e12, True)
        assert not ok and c["status"] == -1
    assert abs(c["err_norm"] - en) <= 1e-14 * max(en, 1e-300)
    # the new h: the device's pow (ocml) and the host's libm pow may round err_norm ** -0.2 one ulp apart, and the
    # norms themselves are sums in different orders -- the decision is exact, h is held to 2 spacings
    assert bool(c["accepted"]) == ok and c["n_accepted"] == int(ok) and c["n_rejected"] == int(not ok)
    if ok:
        t_now = t if case != "clip" else -0.02
        t_done = t_now + (h if case != "clip" else 0.0199)
        assert c["t"] == t_done
        if case == "clip":
            nxt = _next_attempt(t_done, tb, 0.0199 * f, True)
            assert nxt[1] == tb and c["t_new"] == tb
        else:
            nxt = _next_attempt(t_done, tb, abs(h) * f, True)
        assert c["status"] == 0 and c["stage"] == 1
        assert abs(c["h"] - nxt[0]) <= 2 * np.spacing(abs(nxt[0]))
    else:
        nxt = _next_attempt(t, tb, (1.2e-15 if case == "too_small" else h) * f, False)
        if nxt is None:
            assert c["status"] == -1
        else:
            assert c["status"] == 0 and c["step_rejected"] == 1 and c["t"] == t
            assert abs(c["h"] - nxt[0]) <= 2 * np.spacing(abs(nxt[0]))


# ---- 2. analytic denoiser ------------------------------------------------------------------------------------------

class GaussianDenoiser(torch.nn.Module):
    """the exact eps-prediction for data N(0, s2 I): sqrt(var_t) x / (m_t^2 s2 + var_t)"""

    def __init__(self, diff, s2):
        super().__init__()
        self.diff, self.s2 = diff, s2
        self.mixed_prediction = False

    def forward(self, x, t, condition_input=None, clip_feat=None, **kw):
        tt = t.view([-1] + [1] * (x.dim() - 1))
        var, m = self.diff.var(tt), self.diff.e2int_f(tt)
        return torch.sqrt(var) * x / (m * m * self.s2 + var)


@pytest.mark.parametrize("D", [128, 8192])
@pytest.mark.parametrize("graph", [False, True])
def test_analytic_solve_matches_oracle_and_closed_form(D, graph):
    diff = _diff()
    s2 = 0.25
    model = GaussianDenoiser(diff, s2)
    shape = (32, D, 1, 1)
    g = torch.Generator(device="cuda").manual_seed(D)
    noise = torch.randn(shape, device="cuda", generator=g)
    x, nfe, _ = diff.sample_model_ode(model, 32, [D, 1, 1], 1e-5, TOL, False, 1.0, noise=noise, graph=graph)
    c = diff.last_ode
    t0, tb, sign = diff.ode_span(1.0, 1e-5)
    ref = oc.rk45(_drift_oracle_setup(model, diff, shape, sign), t0, tb, noise.double().cpu().numpy().reshape(-1),
                  TOL, TOL)
    assert ref["status"] == "finished"
    assert (nfe, c["n_accepted"], c["n_rejected"]) == (ref["nfe"], ref["n_accepted"], ref["n_rejected"])
    got = x.cpu().numpy().reshape(-1)
    np.testing.assert_array_max_ulp(got, ref["y"].astype(np.float32), maxulp=2)
    exact = oc.gaussian_flow(noise.double().cpu().numpy().reshape(-1), 1.0, float(np.float32(1e-5)), s2)
    assert np.max(np.abs(got - exact)) <= 10 * TOL * max(1.0, np.abs(exact).max())


def test_analytic_round_trip():
    diff = _diff()
    model = GaussianDenoiser(diff, 0.25)
    g = torch.Generator(device="cuda").manual_seed(1)
    x0 = 0.5 * torch.randn(32, 128, 1, 1, device="cuda", generator=g)
    z = diff.compute_ode_nll(model, x0, 1e-5, TOL)
    back, _, _ = diff.sample_model_ode(model, 32, [128, 1, 1], 1e-5, TOL, False, 1.0, noise=z)
    assert torch.isfinite(z).all()
    assert (back - x0).abs().max().item() <= 50 * TOL * max(1.0, x0.abs().max().item())


# ---- 3. the real priors ---------------------------------------------------------------------------------------------

def _priors(scale=0.5):
    from conftest import fill_
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.latent_points_ada_localprior import PVCNN2Prior
    from lion_amd.models.score_sde.resnet import PriorSEDrop
    cfg = released_prior_cfg()
    glob = PriorSEDrop(cfg.sde, 128, cfg)
    loc = PVCNN2Prior(cfg.sde, 1, cfg)
    for m in (glob, loc):
        fill_(m)
        with torch.no_grad():   # the output layers scaled so that the drift is O(1)
            for p in list(m.parameters())[-2:]:
                p.mul_(scale)
        m.cuda().eval()
    return glob, loc


def test_real_priors_graph_equals_eager_and_oracle():
    diff = _diff()
    glob, loc = _priors()
    tol = 1e-3
    B = 4
    g = torch.Generator(device="cuda").manual_seed(2)
    zg = torch.randn(B, 128, 1, 1, device="cuda", generator=g)
    zl = torch.randn(B, 8192, 1, 1, device="cuda", generator=g)
    cond = torch.randn(B, 128, 1, 1, device="cuda", generator=g)
    for name, model, z, c in (("global", glob, zg, None), ("local", loc, zl, cond)):
        shape = list(z.shape[1:])
        xe, ne, _ = diff.sample_model_ode(model, B, shape, 1e-5, tol, False, 1.0, noise=z, condition_input=c,
                                          graph=False)
        xg, ng, _ = diff.sample_model_ode(model, B, shape, 1e-5, tol, False, 1.0, noise=z, condition_input=c,
                                          graph=True)
        # graph replay and the eager loop launch the same kernels on the same inputs: bit-identical solves
        assert ne == ng and torch.equal(xe, xg), (name, ne, ng, (xe - xg).abs().max().item())
        xg2, ng2, _ = diff.sample_model_ode(model, B, shape, 1e-5, tol, False, 1.0, noise=z, condition_input=c,
                                            graph=True)
        assert ng2 == ng and torch.equal(xg2, xg), (name, ng, ng2)
        assert torch.isfinite(xg).all()
        t0, tb, sign = diff.ode_span(1.0, 1e-5)
        ref = oc.rk45(_drift_oracle_setup(model, diff, tuple(z.shape), sign, cond=c), t0, tb,
                      z.double().cpu().numpy().reshape(-1), tol, tol)
        assert ref["nfe"] == ng, (name, ref["nfe"], ng)
        scale = max(1.0, float(np.abs(ref["y"]).max()))
        assert np.max(np.abs(xg.cpu().numpy().reshape(-1) - ref["y"])) <= 1e-5 * scale
        enc = diff.compute_ode_nll(model, xe, 1e-5, tol, condition_input=c)
        assert torch.isfinite(enc).all()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------

def _lion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.lion import LION
    torch.manual_seed(0)
    lion = LION(released_prior_cfg())
    lion.priors.eval()
    lion.vae.eval()
    return lion


def test_two_prior_ode_sampling_and_encode_interpolate():
    from lion_amd.interpolation import encode_interpolate
    from lion_amd.sampling import generate_samples_vada_2prior
    lion = _lion()
    diff = _diff()
    pts, info = generate_samples_vada_2prior(lion.vae.latent_shape(), lion.priors, diff, lion.vae, 2, ode_sample=1,
                                             ode_solver_tol=1e-3)
    assert tuple(pts.shape) == (2, 2048, 3) and torch.isfinite(pts).all()
    assert len(info["nfe"]) == 2 and all(n >= 8 for n in info["nfe"])
    clouds = torch.randn(3, 2048, 3, device="cuda") * 0.3
    tol = 1e-5
    out, inf = encode_interpolate(lion.vae, lion.priors, diff, clouds, ode_solver_tol=tol)
    assert tuple(out.shape) == (3, 2048, 3) and torch.isfinite(out).all() and len(inf["nfe"]) == 4
    eg, el = inf["latents"]
    gi, li = inf["interpolated"]
    ends = lion.vae.sample(num_samples=3, decomposed_eps=[eg.view(3, -1), el.view(3, -1)])
    scale = max(1.0, ends.abs().max().item())
    for k in (0, 2):   # the ends are left alone by the mixing: encode -> ODE there and back -> decode == encode -> decode
        lat = max((gi[k] - eg[k]).abs().max().item(), (li[k] - el[k]).abs().max().item())
        err = (out[k] - ends[k]).abs().max().item()
        assert err <= 1e-4 * scale, (k, err, lat, scale)


# ---- 6. training -----------------------------------------------------------------------------------------------------

def test_continuous_time_prior_train_step():
    """prior_train_step with DiffusionVPSDE('ll_iw') against a plain-autograd restatement of the same loss: the same draws
    (encoder sample, t, noise, dropout), t / var_t / m_t from the float64 closed forms"""
    import math
    import torch.nn.functional as F
    from lion_amd.training import prior_train_step
    lion = _lion()
    diff = _diff()
    assert diff.iw_sample_p == 'll_iw'
    priors, vae = lion.priors, lion.vae
    opt = torch.optim.Adam(priors.parameters(), lr=0.0)     # the step leaves the weights as they are
    x = torch.randn(2, 2048, 3, device="cuda") * 0.3
    torch.manual_seed(3)
    loss, parts = prior_train_step(vae, priors, diff, opt, x)
    assert torch.isfinite(loss) and len(parts) == 2
    got = [p.grad.detach().clone() if p.grad is not None else None for p in priors.parameters()]
    for p in priors.parameters():
        p.grad = None

    torch.manual_seed(3)
    vae.eval()
    priors.train()
    B = x.shape[0]
    with torch.no_grad():
        eps = vae.encode(x)[0]
    rho = torch.rand(B, device="cuda").double()
    l1, l0 = math.log(oc.vp_var(1.0)), math.log(oc.vp_var(1e-2))
    var = torch.exp(rho * l1 + (1 - rho) * l0)
    t = (-0.1 + torch.sqrt(0.01 - 2 * 19.9 * torch.log(1 - var))) / 19.9
    m = torch.exp(-0.5 * (0.1 * t + 0.5 * 19.9 * t * t))
    col = lambda v: v.float().view(-1, 1, 1, 1)
    lat = [e.reshape(B, -1, 1, 1) for e in vae.decompose_eps(eps)]
    total = 0
    for i, e in enumerate(lat):
        noise = torch.randn_like(e)
        e_t = col(m) * e + torch.sqrt(col(var)) * noise
        cond = None if i == 0 else vae.global2style(lat[0])
        pred = priors[i](e_t, t.float(), x0=e, condition_input=cond, clip_feat=None)
        total = total + F.mse_loss(pred.reshape(B, -1), noise.reshape(B, -1))
    total.backward()
    assert abs(total.item() - loss.item()) <= 1e-4 * max(1.0, abs(loss.item()))
    # the product evaluates var_t = 1 - exp(.) in float32 (the reference's arithmetic): near t = time_eps that rounding is
    # ~3e-5 relative against the float64 closed form used here, and a parameter gradient carries it with a gain of a few
    # (measured: 1.2e-4 of the largest entry on the first parameter past 1e-4).  A wrong t, var_t or m_t moves them by O(1).
    for p, g in zip(priors.parameters(), got):
        if g is None:
            assert p.grad is None or not p.grad.any()
            continue
        sc = max(g.abs().max().item(), 1e-6)
        assert (p.grad - g).abs().max().item() <= 1e-3 * sc
