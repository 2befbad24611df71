"""Continuous-time diffusion: the VPSDE of the reference's ``utils/diffusion_continuous.py`` (``make_diffusion`` :21-37,
``DiffusionVPSDE`` :571-622), the importance-sampled training quantities of continuous-time priors (``iw_quantities``
:287-380, every VPSDE-like mode) and the probability-flow ODE sampler / encoder (``sample_model_ode`` :178-255,
``compute_ode_nll`` :90-176) that ``cfg.sde.ode_sample = 1`` selects.

The schedule, for t in [0, 1] and beta(t) = b0 + (b1 - b0) t:
    g2(t) = beta(t),  f(t) = -g2(t) / 2,  m(t) = exp(-(b0 t + (b1 - b0) t^2 / 2) / 2),
    var(t) = 1 - (1 - sigma2_0) exp(-(b0 t + (b1 - b0) t^2 / 2)),  inv_var solves var(t) = v for t.
Every expression is evaluated with the reference's float32 operation order (the parity tests compare bits).

What changes on MI355X: the reference integrates the ODE with scipy's RK45 on the host, copying the batch device -> host
-> device at every evaluation of an eager model; here the same solver runs on the device (``lion_amd/ode.py``,
``csrc/ode.hip``) and the evaluations are graph replays.  Time handling follows torchdiffeq + its scipy wrapper: the span
is a float32 tensor, a descending span is negated and the model wrapped as ``-f(-t, y)``, scipy gets the float32 values
widened to float64 and the model sees the float32 rounding of scipy's t.
"""
from __future__ import annotations

from timeit import default_timer as timer

import numpy as np
import torch

from . import conv_ops
from . import ode as _ode

_NOT_PORTED = ('geometric_sde', 'sub_vpsde', 'power_vpsde', 'sub_power_vpsde', 'vesde')


def make_diffusion(args, device="cuda"):
    """cfg.sde -> its continuous diffusion; only 'vpsde' exists (the reference ships the others commented out)."""
    kind = args.sde_type
    if kind == 'vpsde':
        return DiffusionVPSDE(args, device=device)
    if kind in _NOT_PORTED:
        raise NotImplementedError(f"continuous diffusion {kind!r} is not available; use sde_type='vpsde'")
    raise ValueError(f"Unrecognized sde type: {kind}")


class DiffusionVPSDE(object):
    """Variance-preserving SDE with a linear beta(t); same constructor arguments as the reference (cfg.sde) plus
    ``device``.  ``iw_quantities(size)`` takes its remaining arguments from cfg.sde (time_eps, iw_sample_p,
    iw_subvp_like_vp_sde) so that ``training.prior_forward_backward`` trains a continuous-time prior unchanged."""

    def __init__(self, args, device="cuda"):
        self.sde_type = args.sde_type
        self.device = torch.device(device)
        self.sigma2_0 = args.sigma2_0
        self.beta_start, self.beta_end = args.beta_start, args.beta_end
        self.time_eps = getattr(args, 'time_eps', 1e-2)
        self.iw_sample_p = getattr(args, 'iw_sample_p', 'll_iw')
        self.iw_subvp_like_vp_sde = getattr(args, 'iw_subvp_like_vp_sde', False)
        # constants of the 'drop_all_iw' proposal: t = sqrt(2 / (b1 - b0)) erfinv(u * (E1 - E0) + E0) - b0 / (b1 - b0),
        # E_s = erf(sqrt((b1 - b0) / 2) (s + b0 / (b1 - b0))), normaliser (1 - sigma2_0) e^(frac / 2) sqrt(pi / 4 / dbh) (E1 - E0)
        dev, span = self.device, self.beta_end - self.beta_start
        self.delta_beta_half = torch.tensor(0.5 * span, device=dev)
        self.beta_frac = torch.tensor(self.beta_start / span, device=dev)
        root = torch.sqrt(self.delta_beta_half)
        erf_at_one = torch.erf(root * (1.0 + self.beta_frac))
        self.const_erf = torch.erf(root * (self.time_eps + self.beta_frac))
        self.const_aq = (1.0 - self.sigma2_0) * torch.exp(0.5 * self.beta_frac) * \
            torch.sqrt(0.25 * np.pi / self.delta_beta_half)
        self.const_norm = self.const_aq * (erf_at_one - self.const_erf)
        self.const_norm_2 = erf_at_one - self.const_erf

    # ---- schedule -------------------------------------------------------------------------------------------------
    def g2(self, t):
        return self.beta_start + (self.beta_end - self.beta_start) * t

    def f(self, t):
        return -0.5 * self.g2(t)

    def var(self, t):
        exponent = -self.beta_start * t - 0.5 * (self.beta_end - self.beta_start) * t * t
        return 1.0 - (1.0 - self.sigma2_0) * torch.exp(exponent)

    def e2int_f(self, t):
        return torch.exp(-0.5 * self.beta_start * t - 0.25 * (self.beta_end - self.beta_start) * t * t)

    def inv_var(self, var):
        log_ratio = torch.log((1 - var) / (1 - self.sigma2_0))
        slope = self.beta_end - self.beta_start
        return (-self.beta_start + torch.sqrt(np.square(self.beta_start) - 2 * slope * log_ratio)) / slope

    def mixing_component(self, x_noisy, var_t, t, enabled):
        """the optimal denoiser if q(z_0) were N(0, I): sqrt(var_t) * x_t (None when mixing is off)"""
        return torch.sqrt(var_t) * x_noisy if enabled else None

    def sample_q(self, x_init, noise, var_t, m_t):
        return m_t * x_init + torch.sqrt(var_t) * noise

    def cross_entropy_const(self, ode_eps):
        return 0.5 * (1.0 + torch.log(2.0 * np.pi * self.var(t=torch.tensor(ode_eps, device=self.device))))

    def ode_scalars(self):
        """the fp32 schedule constants of the device drift (lion_ode_drift)"""
        return _ode.schedule_scalars(self.beta_start, self.beta_end, self.sigma2_0)

    # ---- training: t ~ proposal, with the objective weights of p and q ---------------------------------------------
    def iw_quantities(self, size, time_eps=None, iw_sample_mode=None, iw_subvp_like_vp_sde=None, rho=None):
        """(t, var_t, m_t, weight_p, weight_q, g2_t), the last five shaped [size, 1, 1, 1].  rho (tests): the uniform
        draw to use instead of torch.rand(size)."""
        eps_t = self.time_eps if time_eps is None else time_eps
        mode = self.iw_sample_p if iw_sample_mode is None else iw_sample_mode
        u = torch.rand(size=[size], device=self.device) if rho is None else rho
        table = {'ll_uniform': self._ll_uniform, 'll_iw': self._ll_iw, 'drop_all_uniform': self._drop_all_uniform,
                 'drop_all_iw': self._drop_all_iw, 'drop_sigma2t_iw': self._drop_sigma2t_iw,
                 'drop_sigma2t_uniform': self._drop_sigma2t_uniform, 'rescale_iw': self._rescale_iw}
        if mode not in table:
            raise ValueError(f"Unrecognized importance sampling type: {mode}")
        t, var_t, m_t, w_p, w_q, g2_t = table[mode](u, eps_t)
        col = lambda v: v.view(-1, 1, 1, 1)
        return t, col(var_t), col(m_t), col(w_p), col(w_q), col(g2_t)

    def _uniform(self, u, eps_t):
        t = u * (1. - eps_t) + eps_t
        return t, self.var(t), self.e2int_f(t), self.g2(t)

    def _var_ends(self, u, eps_t):
        ones = torch.ones_like(u, device=self.device)
        return self.var(ones), self.var(eps_t * ones)

    def _ll_uniform(self, u, eps_t):
        t, var_t, m_t, g2_t = self._uniform(u, eps_t)
        w = g2_t / (2.0 * var_t)
        return t, var_t, m_t, w, w, g2_t

    def _ll_iw(self, u, eps_t):          # log var_t uniform between its ends
        v1, v0 = self._var_ends(u, eps_t)
        lv1, lv0 = torch.log(v1), torch.log(v0)
        var_t = torch.exp(u * lv1 + (1 - u) * lv0)
        t = self.inv_var(var_t)
        w = 0.5 * (lv1 - lv0) / (1.0 - var_t)
        return t, var_t, self.e2int_f(t), w, w, self.g2(t)

    def _drop_all_uniform(self, u, eps_t):
        t, var_t, m_t, g2_t = self._uniform(u, eps_t)
        return t, var_t, m_t, torch.ones(1, device=self.device), g2_t / (2.0 * var_t), g2_t

    def _drop_all_iw(self, u, eps_t):
        if self.sde_type != 'vpsde':
            raise AssertionError("importance sampling of the fully unweighted objective needs the regular VPSDE")
        t = torch.sqrt(1.0 / self.delta_beta_half) * torch.erfinv(u * self.const_norm_2 + self.const_erf) \
            - self.beta_frac
        var_t, g2_t = self.var(t), self.g2(t)
        w_p = self.const_norm / (1.0 - var_t)
        return t, var_t, self.e2int_f(t), w_p, w_p * g2_t / (2.0 * var_t), g2_t

    def _drop_sigma2t_iw(self, u, eps_t):   # var_t uniform between its ends
        v1, v0 = self._var_ends(u, eps_t)
        var_t = u * v1 + (1 - u) * v0
        t = self.inv_var(var_t)
        w_p = 0.5 * (v1 - v0) / (1.0 - var_t)
        return t, var_t, self.e2int_f(t), w_p, w_p / var_t, self.g2(t)

    def _drop_sigma2t_uniform(self, u, eps_t):
        t, var_t, m_t, g2_t = self._uniform(u, eps_t)
        return t, var_t, m_t, g2_t / 2.0, g2_t / (2.0 * var_t), g2_t

    def _rescale_iw(self, u, eps_t):
        t, var_t, m_t, g2_t = self._uniform(u, eps_t)
        return t, var_t, m_t, 0.5 / (1.0 - var_t), g2_t / (2.0 * var_t), g2_t

    # ---- probability-flow ODE ---------------------------------------------------------------------------------------
    @staticmethod
    def ode_span(t_first, t_last):
        """(t0, t_bound, sign) as solve_ivp receives them for odeint(t=torch.tensor([t_first, t_last]))"""
        ts = torch.tensor([t_first, t_last], dtype=torch.float32)
        sign = -1.0 if ts[0] > ts[1] else 1.0
        ts = ts * sign                         # torchdiffeq: a descending span is negated (exact)
        return float(ts.min()), float(ts.max()), sign

    def _integrate(self, dae, x0, t_first, t_last, tol, condition_input, clip_feat, graph, enable_autocast,
                   mixing_logit=None):
        t0, t_bound, sign = self.ode_span(t_first, t_last)
        return _ode.integrate(dae, x0.contiguous(), t0, t_bound, sign, tol, tol, self.ode_scalars(),
                              condition_input=condition_input, clip_feat=clip_feat, graph=graph,
                              enable_autocast=enable_autocast, mixing_logit=mixing_logit)

    @torch.no_grad()
    def sample_model_ode(self, dae, num_samples, shape, ode_eps, ode_solver_tol, enable_autocast, temp, noise=None,
                         condition_input=None, mixing_logit=None, init_t=1.0, return_all_sample=False, clip_feat=None,
                         graph=True, conv_precision="fp32"):
        """latent noise at init_t -> latent at ode_eps.  Returns (x, nfe, seconds), or with return_all_sample
        (x, [start, x], nfe, seconds): the two points odeint reports.  mixing_logit replaces the model's own logit in the
        mixed prediction (models with mixed_prediction only, as in the reference).
        conv_precision="half": the denoiser's voxel convolutions run at reduced precision (conv_ops.PRECISION)."""
        dae.eval()
        if noise is None:
            noise = torch.randn(size=[num_samples] + list(shape), device=self.device)
        start_x = temp * noise
        tic = timer()
        with conv_ops.requested_precision(conv_precision):
            x, ctrl = self._integrate(dae, start_x, init_t, ode_eps, ode_solver_tol, condition_input, clip_feat, graph,
                                      enable_autocast, mixing_logit)
        seconds = timer() - tic
        self.last_ode = ctrl
        if return_all_sample:
            return x, torch.stack([start_x.float(), x]), ctrl["nfe"], seconds
        return x, ctrl["nfe"], seconds

    @torch.no_grad()
    def compute_ode_nll(self, dae, eps, ode_eps, ode_solver_tol, enable_autocast=False, no_autograd=False,
                        num_samples=1, report_std=False, condition_input=None, clip_feat=None, graph=True):
        """latent at ode_eps -> noise at 1 (the encoding x_t0; the reference's NLL terms are disabled there too)."""
        dae.eval()
        x = None
        for _ in range(num_samples):
            x, self.last_ode = self._integrate(dae, eps, ode_eps, 1.0, ode_solver_tol, condition_input, clip_feat,
                                               graph, enable_autocast)
        return x
