"""CPU suite of the continuous-time (VPSDE) diffusion: the float64 RK45 restatement (tests/ode_oracle.py) against scipy's
solve_ivp, the VPSDE schedule and training quantities against float64 closed forms, the cfg.sde defaults and the
interpolation rules."""
import math

import numpy as np
import pytest
import torch

import ode_oracle as oc


def _scipy(fun, t0, t1, y0, tol):
    """solve_ivp as torchdiffeq's wrapper calls it, with every evaluation counted and the accepted times recorded"""
    scipy_ivp = pytest.importorskip("scipy.integrate")
    n = [0]

    def f(t, y):
        n[0] += 1
        return fun(t, y)
    solver = scipy_ivp.RK45(f, t0, np.asarray(y0, np.float64), t1, rtol=tol, atol=tol)
    ts = [solver.t]
    while solver.status == 'running':
        solver.step()
        ts.append(solver.t)
    sol = scipy_ivp.solve_ivp(fun, (t0, t1), np.asarray(y0, np.float64), method='RK45', rtol=tol, atol=tol)
    assert sol.status == 0 and sol.nfev == n[0]
    return solver, ts, n[0]


def _agree(fun, t0, t1, y0, tol=1e-5, ts_rtol=1e-9):
    ref, ts, nfe = _scipy(fun, t0, t1, y0, tol)
    got = oc.rk45(fun, t0, t1, y0, tol, tol)
    assert got['status'] == 'finished'
    assert got['nfe'] == nfe
    assert len(got['ts']) == len(ts)
    # the error estimate sum_j E_j K_j cancels: numpy's dot order moves it (and the next step size) by ~1e-11 relative
    np.testing.assert_allclose(got['ts'], ts, rtol=ts_rtol, atol=0)
    np.testing.assert_allclose(got['y'], ref.y, rtol=1e-13, atol=1e-300)
    return got


def test_restatement_equals_scipy_on_a_linear_decay():
    y0 = np.linspace(-2, 3, 17)
    got = _agree(lambda t, y: -1.7 * y, 0.0, 2.0, y0)
    np.testing.assert_allclose(got['y'], y0 * math.exp(-3.4), rtol=1e-4)


@pytest.mark.parametrize("s2", [0.04, 1.0, 9.0])
def test_restatement_equals_scipy_on_the_gaussian_pf_ode_both_directions(s2):
    rng = np.random.default_rng(0)
    y0 = rng.standard_normal(64)
    # sampling: odeint(t=[1, ode_eps]) -> torchdiffeq negates the span and wraps the drift as -f(-t, y)
    t0, t1 = [-float(np.float32(v)) for v in (1.0, 1e-5)]
    rev = lambda t, y: -oc.gaussian_drift(-t, y, s2)
    got = _agree(rev, t0, t1, y0)
    np.testing.assert_allclose(got['y'], oc.gaussian_flow(y0, 1.0, float(np.float32(1e-5)), s2), rtol=2e-4, atol=1e-4)
    # encoding: odeint(t=[ode_eps, 1]) runs forward
    x = got['y']
    back = _agree(lambda t, y: oc.gaussian_drift(t, y, s2), float(np.float32(1e-5)), 1.0, x)
    np.testing.assert_allclose(back['y'], y0, rtol=1e-3, atol=1e-3)


def test_restatement_equals_scipy_through_rejections_and_the_factor_cap():
    # a stiff-ish oscillator with a kink: the first steps overshoot and are rejected
    fun = lambda t, y: np.array([y[1], -400.0 * y[0] - 0.5 * y[1] * (1 + np.tanh(50 * (t - 0.3)))])
    got = _agree(fun, 0.0, 1.0, np.array([1.0, 0.0]), tol=1e-6, ts_rtol=1e-7)
    assert got['n_rejected'] >= 1


def test_post_rejection_factor_is_capped_at_one():
    assert oc.step_factor(0.01, True) == (True, 1)
    ok, f = oc.step_factor(0.01, False)
    assert ok and f == min(10, 0.9 * 0.01 ** -0.2) and f > 1
    assert oc.step_factor(0.0, False) == (True, 10)
    assert oc.step_factor(1e6, False) == (False, 0.2)


def _sde_cfg(**kw):
    from lion_amd.config import released_prior_cfg
    c = released_prior_cfg().sde
    c.update(kw)
    return c


def test_cfg_sde_defaults_present():
    from lion_amd.config import released_prior_cfg
    s = released_prior_cfg().sde
    assert (s.sde_type, s.beta_start, s.beta_end, s.sigma2_0) == ('vpsde', 0.1, 20.0, 0.0)
    assert (s.time_eps, s.ode_eps, s.iw_sample_p, s.iw_subvp_like_vp_sde, s.time_emb_scales) == \
        (1e-2, 1e-5, 'll_iw', False, 1.0)
    assert s.ode_sample == 0


def test_make_diffusion_accepts_vpsde_only():
    from lion_amd.diffusion_continuous import DiffusionVPSDE, make_diffusion
    assert isinstance(make_diffusion(_sde_cfg(), device='cpu'), DiffusionVPSDE)
    for kind in ('vesde', 'sub_vpsde', 'power_vpsde', 'sub_power_vpsde', 'geometric_sde'):
        with pytest.raises(NotImplementedError):
            make_diffusion(_sde_cfg(sde_type=kind), device='cpu')
    with pytest.raises(ValueError):
        make_diffusion(_sde_cfg(sde_type='nope'), device='cpu')


def test_schedule_matches_float64_closed_forms():
    from lion_amd.diffusion_continuous import make_diffusion
    d = make_diffusion(_sde_cfg(), device='cpu')
    t = torch.linspace(1e-5, 1.0, 257, dtype=torch.float64)
    tn = t.numpy()
    np.testing.assert_allclose(d.g2(t).numpy(), 0.1 + 19.9 * tn, rtol=1e-15)
    np.testing.assert_allclose(d.f(t).numpy(), -0.5 * (0.1 + 19.9 * tn), rtol=1e-15)
    np.testing.assert_allclose(d.var(t).numpy(), [oc.vp_var(v) for v in tn], rtol=1e-12)
    np.testing.assert_allclose(d.e2int_f(t).numpy(), [math.exp(oc.vp_log_mean(v)) for v in tn], rtol=1e-13)
    np.testing.assert_allclose(d.inv_var(d.var(t)).numpy(), tn, rtol=1e-9)
    # float32 as the samplers evaluate it: the round trip within float32 resolution
    t32 = t.float()
    np.testing.assert_allclose(d.inv_var(d.var(t32)).double().numpy(), tn, rtol=2e-3, atol=2e-4)
    assert torch.allclose(d.mixing_component(t32, d.var(t32), t32, True), torch.sqrt(d.var(t32)) * t32)
    assert d.mixing_component(t32, d.var(t32), t32, False) is None
    ce = d.cross_entropy_const(1e-5)   # float32 var(1e-5) = 1 - exp(-1e-6): the cancellation is the reference's too
    assert abs(float(ce) - 0.5 * (1 + math.log(2 * math.pi * oc.vp_var(1e-5)))) < 2e-2


MODES = ['ll_uniform', 'll_iw', 'drop_all_uniform', 'drop_all_iw', 'drop_sigma2t_iw', 'drop_sigma2t_uniform',
         'rescale_iw']


def _iw64(mode, u, eps_t=1e-2, b0=0.1, b1=20.0):
    """float64 restatement of the weights: (t, var, m, w_p, w_q, g2)"""
    var = lambda t: np.array([oc.vp_var(v, b0, b1) for v in np.atleast_1d(t)])
    g2 = lambda t: b0 + (b1 - b0) * t
    mean = lambda t: np.exp([oc.vp_log_mean(v, b0, b1) for v in np.atleast_1d(t)])
    inv = lambda v: (-b0 + np.sqrt(b0 * b0 - 2 * (b1 - b0) * np.log(1 - v))) / (b1 - b0)
    if mode in ('ll_uniform', 'drop_all_uniform', 'drop_sigma2t_uniform', 'rescale_iw'):
        t = u * (1 - eps_t) + eps_t
        v = var(t)
        wq = g2(t) / (2 * v)
        wp = {'ll_uniform': wq, 'drop_all_uniform': np.ones_like(t), 'drop_sigma2t_uniform': g2(t) / 2,
              'rescale_iw': 0.5 / (1 - v)}[mode]
    elif mode == 'll_iw':
        l1, l0 = math.log(oc.vp_var(1.0, b0, b1)), math.log(oc.vp_var(eps_t, b0, b1))
        v = np.exp(u * l1 + (1 - u) * l0)
        t = inv(v)
        wp = wq = 0.5 * (l1 - l0) / (1 - v)
    elif mode == 'drop_sigma2t_iw':
        s1, s0 = oc.vp_var(1.0, b0, b1), oc.vp_var(eps_t, b0, b1)
        v = u * s1 + (1 - u) * s0
        t = inv(v)
        wp = 0.5 * (s1 - s0) / (1 - v)
        wq = wp / v
    else:   # drop_all_iw: t from the inverse CDF of 1 / (1 - var_t) on [eps_t, 1]
        special = pytest.importorskip("scipy.special")
        erf, erfinv = special.erf, special.erfinv
        dbh, frac = 0.5 * (b1 - b0), b0 / (b1 - b0)
        e0, e1 = erf(math.sqrt(dbh) * (eps_t + frac)), erf(math.sqrt(dbh) * (1 + frac))
        t = math.sqrt(1 / dbh) * erfinv(u * (e1 - e0) + e0) - frac
        v = var(t)
        wp = math.exp(0.5 * frac) * math.sqrt(0.25 * math.pi / dbh) * (e1 - e0) / (1 - v)
        wq = wp * g2(t) / (2 * v)
    return t, v, mean(t), wp, wq, g2(t)


@pytest.mark.parametrize("mode", MODES)
def test_iw_quantities_shapes_ranges_and_weights(mode):
    from lion_amd.diffusion_continuous import make_diffusion
    d = make_diffusion(_sde_cfg(), device='cpu')
    u = torch.linspace(0.001, 0.999, 64)
    t, var, m, wp, wq, g2 = d.iw_quantities(64, iw_sample_mode=mode, rho=u)
    assert t.shape == (64,)
    for q in (var, m, wq, g2):
        assert q.shape == (64, 1, 1, 1) and torch.isfinite(q).all()
    assert wp.shape in ((64, 1, 1, 1), (1, 1, 1, 1))
    assert ((t >= 1e-2 - 1e-5) & (t <= 1.0 + 1e-5)).all()
    assert ((var > 0) & (var < 1)).all() and ((m > 0) & (m <= 1)).all()
    ref = _iw64(mode, u.double().numpy())
    for got, want in zip((t, var, m, wp, wq, g2), ref):
        want = np.asarray(want, np.float64).reshape(-1)[:got.numel()]
        np.testing.assert_allclose(got.reshape(-1).double().numpy(), want, rtol=5e-4)


def test_iw_quantities_defaults_come_from_cfg():
    from lion_amd.diffusion_continuous import make_diffusion
    d = make_diffusion(_sde_cfg(iw_sample_p='ll_uniform', time_eps=0.25), device='cpu')
    t = d.iw_quantities(1000)[0]
    assert t.min() >= 0.25 and t.max() <= 1.0
    with pytest.raises(ValueError):
        d.iw_quantities(4, iw_sample_mode='nope')


def test_ode_span_reproduces_torchdiffeq_time_handling():
    from lion_amd.diffusion_continuous import DiffusionVPSDE
    t0, t1, sign = DiffusionVPSDE.ode_span(1.0, 1e-5)
    assert (t0, t1, sign) == (-1.0, -float(np.float32(1e-5)), -1.0)
    t0, t1, sign = DiffusionVPSDE.ode_span(1e-5, 1.0)
    assert (t0, t1, sign) == (float(np.float32(1e-5)), 1.0, 1.0)


def test_interpolation_rules():
    from lion_amd import interpolation as it
    g = torch.Generator().manual_seed(0)
    x = torch.randn(8, 5, 1, 1, generator=g)
    for fn, rule in ((it.interpolate_noise, lambda p, a, b: np.sqrt(p) * b + np.sqrt(1 - p) * a),
                     (it.linear_interpolate_noise, lambda p, a, b: p * b + (1 - p) * a)):
        y = fn(x.clone())
        assert torch.equal(y[0], x[0]) and torch.equal(y[-1], x[-1])
        for k in range(1, 7):
            p = k / 8
            assert torch.equal(y[k], rule(p, x[0], x[-1]))
    z = it.freeze_noise(x.clone())
    assert all(torch.equal(z[k], x[0]) for k in range(8))
    w = torch.randn(16, 3, generator=g)
    s = it.subtract_noise(w.clone())
    d = w[12] - w[15]
    for k, ref in enumerate((w[12], w[15], w[9], w[10], w[9] + d, w[10] + d)):
        assert torch.equal(s[k], ref)
    assert torch.equal(s[6:], w[6:])
