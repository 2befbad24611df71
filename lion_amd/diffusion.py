"""Discrete diffusion process -- mirror of the reference's ``utils/diffusion_pvd.py``
(``DiffusionDiscretized`` :17; constants :118-142; ``run_denoising_diffusion`` :224-303;
``run_ddim`` :390-473; ``get_q_posterior_mean`` :475-486; ``run_denoising_diffusion_from_t`` :504-563) and ``utils/diffusion.py:28-65``
(``make_beta_schedule``).

What changes on MI355X: by default (``graph=True``, GPU tensors, eval) a chain is S replays of ONE captured
hipGraph [step prologue -> denoiser forward -> fused update with on-chip Philox noise], nothing per step comes
from the host (``lion_amd/chain.py``); the reference issues ~10 elementwise launches per step on top of the
~500 of the denoiser and draws the DDIM noise on the CPU, copying it over every step (:465-466).  The scalar
coefficients are computed exactly as the reference computes them -- float32 0-d tensor arithmetic on the same
float32 schedule -- so for identical (x, eps_hat, z) the update is bit-identical (``lion_ddim_update`` /
``lion_ddpm_update`` and the chain kernel share the arithmetic).  The noise STREAM differs by construction
(Philox on the device vs torch's CPU generator): ``graph=False, noise='cpu'`` reproduces the reference's stream
for seed-for-seed comparisons, ``graph=False`` alone the eager per-step loop.
Beyond the reference: the few-step solvers ``run_dpm_solver`` and the deterministic encoder ``run_ddim_forward`` (a stub in the
reference, :305-388), the inverse of the order-1 solver, on the same captured step.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from . import chain as _chain
from . import conv_ops
from . import diffusion_ops


def make_beta_schedule(schedule, start, end, n_timestep):
    """float64 beta schedule (values as in utils/diffusion.py:28-65)."""
    if schedule == "cust":  # airplane PVD schedule: 10 % linear warm-up to beta_T, then constant
        betas = end * np.ones(n_timestep, dtype=np.float64)
        warm = int(n_timestep * 0.1)
        betas[:warm] = np.linspace(start, end, warm, dtype=np.float64)
    elif schedule == "quad":
        betas = torch.linspace(start ** 0.5, end ** 0.5, n_timestep, dtype=torch.float64).numpy() ** 2
    elif schedule == "linear":
        betas = torch.linspace(start, end, n_timestep, dtype=torch.float64).numpy()
    elif schedule in ("warmup10", "warmup50"):
        frac = 0.1 if schedule == "warmup10" else 0.5
        betas = end * np.ones(n_timestep, dtype=np.float64)
        warm = int(n_timestep * frac)
        betas[:warm] = np.linspace(start, end, warm, dtype=np.float64)
    elif schedule == "const":
        betas = end * np.ones(n_timestep, dtype=np.float64)
    elif schedule == "jsd":
        betas = 1.0 / np.linspace(n_timestep, 1, n_timestep, dtype=np.float64)
    else:
        raise NotImplementedError(schedule)
    return torch.from_numpy(np.asarray(betas, dtype=np.float64))


@contextlib.contextmanager
def _sampling(model, conv_precision):
    """one sampler call: the requested conv precision, the model in eval mode; on the way out model.train(), unconditionally
    as the reference does -- also when an exception passes through"""
    with conv_ops.requested_precision(conv_precision):
        model.eval()
        try:
            yield
        finally:
            model.train()


def _mixed(model, pred, mixing_component):
    """utils/utils.py:1299-1305."""
    if getattr(model, "mixed_prediction", False):
        coeff = torch.sigmoid(model.mixing_logit)
        return (1 - coeff) * mixing_component + coeff * pred
    return pred


class DiffusionDiscretized(object):
    """Constants and samplers of the discrete (DDPM) process; same constructor as the reference."""

    def __init__(self, args, var_fun, cfg, device="cuda"):
        self.cfg = cfg
        self.device = torch.device(device)
        self._diffusion_steps = cfg.ddpm.num_steps
        self._denoising_stddevs = 'beta'
        self.p2_gamma = cfg.ddpm.p2_gamma
        self.p2_k = cfg.ddpm.p2_k
        self.use_p2_weight = cfg.ddpm.use_p2_weight
        self.betas = make_beta_schedule(cfg.ddpm.sched_mode, cfg.ddpm.beta_1, cfg.ddpm.beta_T,
                                        cfg.ddpm.num_steps).numpy()
        # float64 numpy -> float32 (reference :118-142).  Host copies feed the scalar arithmetic.
        alphas = 1.0 - self.betas
        alpha_bars = np.cumprod(alphas)
        snr = 1.0 / (1 - alpha_bars) - 1
        betas_post = self.betas[1:] * (1.0 - alpha_bars[:-1]) / (1.0 - alpha_bars[1:])
        betas_post_init = np.append(betas_post[0], betas_post)
        f32 = lambda a: torch.from_numpy(a).float()
        self._h_betas, self._h_alphas, self._h_alpha_bars = f32(self.betas), f32(alphas), f32(alpha_bars)
        self._betas_init = self._h_betas.to(self.device)
        self.snr = f32(snr).to(self.device)
        self._alphas = self._h_alphas.to(self.device)
        self._alpha_bars = self._h_alpha_bars.to(self.device)
        self._betas_post_init = f32(betas_post_init).to(self.device)
        self._chains = _chain.ChainCache()

    # ---- training-side quantities (reference :45-113) ------------------------------------------
    def _iw(self, B, timestep):
        timestep = timestep + 1  # [1, T]
        alpha_bars = torch.gather(self._alpha_bars, 0, timestep - 1)
        weight_init = torch.sqrt(alpha_bars)[:, None, None, None]
        weight_noise_power = (1.0 - alpha_bars)[:, None, None, None]
        if self.use_p2_weight:
            loss_weight = torch.gather(1 / (self.p2_k + self.snr) ** self.p2_gamma, 0, timestep - 1).view(B)
        else:
            loss_weight = 1.0
        return timestep, weight_noise_power, weight_init, loss_weight, None, None

    def iw_quantities_t(self, B, timestep, *args):
        return self._iw(B, timestep.view(B))

    def iw_quantities(self, B, *args):
        rho = torch.rand(size=[B], device=self.device) * self._diffusion_steps
        return self._iw(B, rho.type(torch.int64))

    def sample_q(self, x_init, noise, var_t, m_t):
        assert len(x_init.shape) == 4 and len(var_t.shape) == 4 and len(m_t.shape) == 4
        assert x_init.shape[0] == m_t.shape[0]
        return m_t * x_init + torch.sqrt(var_t) * noise

    def cross_entropy_const(self, ode_eps):
        return 0

    def get_p_log_scales(self, timestep, stddev_type):
        if stddev_type == 'beta':
            return 0.5 * torch.log(torch.gather(self._betas_init, 0, timestep - 1))
        if stddev_type == 'beta_post':
            return 0.5 * torch.log(torch.gather(self._betas_post_init, 0, timestep - 1))
        if stddev_type == 'learn':
            return None
        raise ValueError('Unknown stddev_type: {}'.format(stddev_type))

    def get_mixing_component(self, x_noisy, timestep, enabled):
        if not enabled:
            return None
        alpha_bars = torch.gather(self._alpha_bars, 0, timestep - 1)
        return torch.sqrt(1.0 - alpha_bars).view(-1, 1, 1, 1) * x_noisy

    def mixing_component(self, eps, var, t, enabled):
        return self.get_mixing_component(eps, t, enabled)

    def get_q_posterior_mean(self, x_noisy, prediction, t):
        """torch formulation of :475-486 (the samplers below use the fused kernel instead)."""
        if t == 0:
            return 1.0 / torch.sqrt(self._alpha_bars[0]) * \
                (x_noisy - torch.sqrt(1.0 - self._alpha_bars[0]) * prediction)
        return 1.0 / torch.sqrt(self._alphas[t]) * \
            (x_noisy - self._betas_init[t] * prediction / torch.sqrt(1.0 - self._alpha_bars[t]))

    # ---- step coefficients: float32 0-d tensor arithmetic, exactly the reference's expressions ----
    def ddim_coefficients(self, t, t_next, kappa):
        """(s, c, sigma) of x <- x*s + c*eps + sigma*z for the step t -> t_next (t_next None = last).
        reference :434-447."""
        ab = self._h_alpha_bars
        if t_next is None:
            alpha_next = torch.tensor(1.0)
            sigma = torch.tensor(0.0)
        else:
            alpha_next = ab[t_next]
            sigma = kappa * torch.sqrt((1 - alpha_next) / (1 - ab[t]) * (1 - ab[t] / alpha_next))
        s = torch.sqrt(alpha_next / ab[t])
        c = torch.sqrt(1 - alpha_next - sigma ** 2) - torch.sqrt(1 - ab[t]) * torch.sqrt(alpha_next / ab[t])
        return float(s), float(c), float(sigma)

    def ddpm_coefficients(self, t):
        """(t_is_zero, k_outer, k_a, k_b, scale) for the ancestral step at t (reference :475-486, :265-266)."""
        ab, al, be = self._h_alpha_bars, self._h_alphas, self._h_betas
        scale = torch.exp(0.5 * torch.log(be[t]))
        if t == 0:
            return True, float(1.0 / torch.sqrt(ab[0])), float(torch.sqrt(1.0 - ab[0])), 1.0, float(scale)
        return False, float(1.0 / torch.sqrt(al[t])), float(be[t]), float(torch.sqrt(1.0 - ab[t])), float(scale)

    @staticmethod
    def ddim_schedule(diffusion_steps, S, skip_type='uniform'):
        """descending list of the visited timesteps (reference :408-419)."""
        if S == 1:
            tau = [0]   # (the reference's expression divides by S - 1)
        elif skip_type == 'uniform':
            c = (diffusion_steps - 1.0) / (S - 1.0)
            tau = [int(np.floor(i * c)) for i in range(S)]
        elif skip_type == 'quad':
            tau = [int(s) for s in list(np.linspace(0, np.sqrt(diffusion_steps * 0.8), S) ** 2)]
        else:
            raise NotImplementedError(skip_type)
        return sorted(tau, reverse=True)

    def ddim_table(self, steps, kappa):
        """[S, 8] float32 rows {t_model, s, c, sigma, 0...} of a DDIM chain over the descending timesteps `steps`: what a
        captured chain reads its per-step scalars from (lion_amd/chain.py)"""
        table = np.zeros((len(steps), 8), np.float32)
        for i, t in enumerate(steps):
            last = i == len(steps) - 1
            s_, c_, sigma_ = self.ddim_coefficients(t, None if last else steps[i + 1], kappa)
            table[i, :4] = (t + 1, s_, c_, sigma_)
        return table

    def ddpm_table(self, t_from, temp=1.0, noise_scale=None):
        """[t_from, 8] float32 rows {t_model, k_outer, k_a, k_b, scale, temp, t == 0, 0} of the ancestral steps
        t = t_from-1 ... 0: the whole chain for t_from = T, its tail otherwise.  ``noise_scale(t)`` overrides sqrt(beta_t) at
        t > 0.  Host arithmetic only."""
        t_from = int(t_from)
        if not 1 <= t_from <= self._diffusion_steps:
            raise ValueError(f"ddpm_table: t_from = {t_from} outside [1, {self._diffusion_steps}]")
        table = np.zeros((t_from, 8), np.float32)
        for i, t in enumerate(reversed(range(t_from))):
            is0, k_outer, k_a, k_b, scale = self.ddpm_coefficients(t)
            if noise_scale is not None and not is0:
                scale = float(noise_scale(t))
            table[i] = (t + 1, k_outer, k_a, k_b, scale, temp, 1.0 if is0 else 0.0, 0.0)
        return table

    def known_levels(self, t_from):
        """[t_from, 2] float32: beside row i of ddpm_table(t_from) -- the step at t = t_from-1-i, which leaves the state at the
        noise level of index t-1 -- the two scalars (m, s) with which diffuse(x0, t-1) draws that level from a clean x0, from
        the same expressions on the float32 host schedule; the row of t = 0 holds (1, 0): the clean value itself.  What the
        known-region chain reads its forward draws' scalars from (chain.GraphedChain(known=True)).  Host arithmetic only."""
        t_from = int(t_from)
        if not 1 <= t_from <= self._diffusion_steps:
            raise ValueError(f"known_levels: t_from = {t_from} outside [1, {self._diffusion_steps}]")
        ms = np.zeros((t_from, 2), np.float32)
        for i, t in enumerate(reversed(range(t_from))):
            if t == 0:
                ms[i] = (1.0, 0.0)
            else:
                ab = self._h_alpha_bars[t - 1]
                ms[i] = (float(torch.sqrt(ab)), float(torch.sqrt(1.0 - ab)))
        return ms

    # ---- RePaint's resampling jumps: a schedule that walks up as well as down ---------------------------
    def resample_walk(self, t_from, jump_length, n_resample):
        """[(t, up), ...]: the ancestral step at index t (ddpm_table's sense), then a forward move of `up` levels (0: none).
        With n the number of steps still to go, n = t_from, and the anchors a = j, 2j, ... with a + j <= t_from, each with a
        budget of n_resample - 1: take the step at t = n - 1 (n -= 1); where n is then an anchor with budget left, spend one,
        mark that row up = j and set n += j.  RePaint's get_schedule_jump (Lugmayr et al. 2022) with the j one-step forward
        transitions of a jump composed into one move and no jump from the clean state; an anchor is consumed only when a step
        reaches it.  n_resample = 1 is the plain tail; the row count is t_from + (#anchors)*(n_resample - 1)*j.  ValueError:
        a bool or non-integer argument, jump_length or n_resample below 1, t_from outside 1 ... T, more than 16*T rows.  Host
        arithmetic only."""
        T = self._diffusion_steps
        for name, v in (("t_from", t_from), ("jump_length", jump_length), ("n_resample", n_resample)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"resample_walk: {name} = {v!r} is not an int")
        t_from, j, R = int(t_from), int(jump_length), int(n_resample)
        if j < 1 or R < 1:
            raise ValueError(f"resample_walk: jump_length = {j} and n_resample = {R} must be at least 1")
        if not 1 <= t_from <= T:
            raise ValueError(f"resample_walk: t_from = {t_from} outside [1, {T}]")
        anchors = max(t_from // j - 1, 0)                   # a = j ... with a + j <= t_from
        rows = t_from + anchors * (R - 1) * j
        if rows > 16 * T:
            raise ValueError(f"resample_walk: {rows} rows for t_from = {t_from}, jump_length = {j}, n_resample = {R}: more "
                             f"than 16*T = {16 * T}")
        budget = {a * j: R - 1 for a in range(1, anchors + 1)}
        walk, n = [], t_from
        while n > 0:
            n -= 1
            up = 0
            if budget.get(n, 0) > 0:
                budget[n] -= 1
                up = j
            walk.append((n, up))
            n += up
        assert len(walk) == rows
        return walk

    def resample_tables(self, t_from, jump_length, n_resample, temp=1.0):
        """(table [S', 8], ms [S', 2], jump [S', 2]), float32, for the S' rows (t_i, up_i) of resample_walk: table row i is
        ddpm_table's row of t_i; jump[i] = (mf, sf) is the forward move that ends the row, (1, 0) where up_i = 0 and else
        mf = sqrt(ab[t-1+up] / ab[t-1]), sf = sqrt(1 - ab[t-1+up] / ab[t-1]) on the float32 host schedule; ms[i] is
        known_levels' pair of the level the state has after the row, jump included: index t-1+up, (1, 0) after the step at
        t = 0.  With n_resample = 1 these are ddpm_table(t_from, temp), known_levels(t_from) and (1, 0) rows, bit for bit.
        What the resampling chain reads (chain.GraphedChain(known=True, resample=True)).  Host arithmetic only."""
        walk = self.resample_walk(t_from, jump_length, n_resample)
        plain, levels = self.ddpm_table(t_from, temp), self.known_levels(t_from)
        table = np.zeros((len(walk), 8), np.float32)
        ms = np.zeros((len(walk), 2), np.float32)
        jump = np.zeros((len(walk), 2), np.float32)
        ab = self._h_alpha_bars
        for i, (t, up) in enumerate(walk):
            table[i] = plain[int(t_from) - 1 - t]
            if up == 0:
                ms[i], jump[i] = levels[int(t_from) - 1 - t], (1.0, 0.0)
            else:                                           # t >= 1 here: no jump from the clean state
                ratio = ab[t - 1 + up] / ab[t - 1]
                jump[i] = (float(torch.sqrt(ratio)), float(torch.sqrt(1.0 - ratio)))
                level = ab[t - 1 + up]                      # known_levels' expressions at the index behind the jump
                ms[i] = (float(torch.sqrt(level)), float(torch.sqrt(1.0 - level)))
        return table, ms, jump

    # ---- DPM-Solver++(2M): schedule and coefficients (float64 on the widened float32 schedule, cast once) ----------------
    def _half_logsnr(self):
        """lambda[i] = log(alpha_i / sigma_i) = 0.5*(log(ab_i) - log1p(-ab_i)) in float64, with ab widened from float32"""
        ab = self._h_alpha_bars.numpy().astype(np.float64)
        return ab, 0.5 * (np.log(ab) - np.log1p(-ab))

    def solver_schedule(self, S, skip_type='logsnr', t_start=None):
        """Descending list of DISTINCT schedule indices for run_dpm_solver: starts at T-1 (S >= 2), ends at 0; S == 1 gives
        [0], as ddim_schedule does.  The list may be SHORTER than S: duplicates are removed, since a step of zero length has
        h = 0 and no second-order ratio.
        'logsnr' (default): S points uniform in the half log-SNR lambda from lambda[T-1] to lambda[0], each mapped to the
        nearest index.  This is the spacing the multistep solver is built for: its error terms are powers of the lambda step
        h, and with 'uniform' index spacing the last jump (to t = 0) is so large in lambda that the second-order step is no
        better than DDIM there (measured ratios 0.6 ... 2.8 against 5.5 ... 21 with 'logsnr').
        'uniform' / 'quad': ddim_schedule(T, S, skip_type) with duplicates removed; where its largest entry falls short of
        T-1 ('quad' stops at 0.8*T; 'uniform' where the floor rounds down) that entry is moved up to T-1, the index whose
        marginal the N(0, I) start is drawn for.  Any other string: ValueError.
        t_start (an index, 1 <= t_start <= T-1; anything else: ValueError): the tail of a chain from that index -- the same
        construction on the indices <= t_start, as if the process had t_start + 1 steps: 'logsnr' takes S points uniform in
        lambda from lambda[t_start] to lambda[0], 'uniform' / 'quad' are ddim_schedule(t_start + 1, S, skip_type).  The list
        starts at t_start and ends at 0, so a tail needs S >= 2 (S == 1: ValueError).  t_start = T-1 is the default list."""
        T, S = self._diffusion_steps, int(S)
        if skip_type not in ('logsnr', 'uniform', 'quad'):
            raise ValueError(f"solver_schedule: unknown skip_type {skip_type!r}")
        if S < 1:
            raise ValueError(f"solver_schedule: S = {S}")
        if t_start is None:
            top = T - 1
        else:
            if isinstance(t_start, bool) or not isinstance(t_start, (int, np.integer)) or not 1 <= t_start <= T - 1:
                raise ValueError(f"solver_schedule: t_start = {t_start!r} is not an index in [1, {T - 1}]")
            if S == 1:
                raise ValueError("solver_schedule: a tail from t_start visits t_start and 0: S >= 2")
            top = int(t_start)
        if S == 1:
            return [0]
        if skip_type == 'logsnr':
            _, lam = self._half_logsnr()
            lam = lam[:top + 1]
            tau = [int(np.argmin(np.abs(lam - p))) for p in np.linspace(lam[top], lam[0], S)]
        else:
            tau = self.ddim_schedule(top + 1, S, skip_type)
        tau = sorted(set(tau), reverse=True)
        if tau[0] != top:
            tau[0] = top
        if tau[-1] != 0:
            tau.append(0)
        return tau

    def dpm_solver_table(self, steps, order=2, dtype=np.float32, stochastic=False):
        """[len(steps), 8] rows {t_model, a0..a5, 0} of DPM-Solver++ (Lu et al. 2022, Algorithm 2; order 1 is DDIM with
        kappa = 0) over the descending distinct indices `steps`, the last of which is 0 -- what lion_dpmpp_update and the
        captured chain (chain.DPMPP) read:  x0 = a0*(x - a1*eps);  D = a4*x0 + a5*x0_prev;  x <- a2*x + a3*D.
        With alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha/sigma), and for the step t = steps[i] -> n = steps[i+1]
        h_i = lambda[n] - lambda[t]:  a0 = 1/alpha_t, a1 = sigma_t, a2 = sigma_n/sigma_t, a3 = -alpha_n*expm1(-h_i);
        (a4, a5) = (1, 0) for i == 0 or order 1, else (1 + 1/(2r), -1/(2r)) with r = h_{i-1}/h_i.
        The last row (t = 0) returns the data prediction, like DDIM's alpha_next = 1: a2 = 0, a3 = 1, a4 = 1, a5 = 0.
        All arithmetic in float64 on the float32 schedule widened; the result is cast to `dtype` once (float64: the values
        before the cast).
        stochastic=True: SDE-DPM-Solver++(2M) (the same paper, the SDE form of Algorithm 2), x <- a2*x + a3*D + a6*z with
        z ~ N(0, I): a2 = (sigma_n/sigma_t)*exp(-h_i), a3 = -alpha_n*expm1(-2*h_i), and the noise scale
        a6 = sigma_n*sqrt(-expm1(-2*h_i)) in column 7 (0 otherwise); a0, a1, a4, a5 and the last row (a6 = 0: it draws nothing)
        as above.  Order 1 is DDIM with kappa = 1 (a2 + a3*a0 = s, -a3*a0*a1 = c, a6 = sigma of ddim_coefficients), and
        (a2*sigma_t)^2 + a6^2 = sigma_n^2: what is left of the old noise plus the fresh noise is the new marginal's."""
        if order not in (1, 2):
            raise ValueError(f"dpm_solver_table: order = {order!r}, must be 1 or 2")
        steps = [int(t) for t in steps]
        assert len(steps) >= 1 and steps[-1] == 0, "the last step is t = 0"
        assert all(a > b for a, b in zip(steps, steps[1:])), "descending distinct indices"
        ab, lam = self._half_logsnr()
        alpha, sigma = np.sqrt(ab), np.sqrt(1.0 - ab)
        table = np.zeros((len(steps), 8), np.float64)
        h_prev = None
        for i, t in enumerate(steps):
            table[i, :3] = (t + 1, 1.0 / alpha[t], sigma[t])
            if i == len(steps) - 1:
                table[i, 3:7] = (0.0, 1.0, 1.0, 0.0)
                break
            n = steps[i + 1]
            h = lam[n] - lam[t]
            if stochastic:
                table[i, 3:5] = (sigma[n] / sigma[t] * np.exp(-h), -alpha[n] * np.expm1(-2.0 * h))
                table[i, 7] = sigma[n] * np.sqrt(-np.expm1(-2.0 * h))
            else:
                table[i, 3:5] = (sigma[n] / sigma[t], -alpha[n] * np.expm1(-h))
            if i == 0 or order == 1:
                table[i, 5:7] = (1.0, 0.0)
            else:
                r = h_prev / h
                table[i, 5:7] = (1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r))
            h_prev = h
        return table.astype(dtype)

    def encode_table(self, taus, refine=0, dtype=np.float32):
        """[len(taus)*(1 + refine), 8] rows {t_model, s, c, commit, 0...} of the deterministic encoder (run_ddim_forward) over
        the descending distinct indices `taus` that solver_schedule returns, walked from low noise to high noise -- what
        lion_ddim_encode_update and the captured chain (chain.ENCODE) read:  x <- s*base + c*eps(x, t_model);  commit: base <- x.
        With alpha = sqrt(ab), sigma = sqrt(1 - ab): the first leg takes the clean latent (alpha_low = 1, sigma_low = 0) to
        index taus[-1] = 0 with s = alpha_0, c = sigma_0, the inverse of dpm_solver_table's final data-prediction row; every
        later leg n -> t has s = alpha_t/alpha_n, c = sigma_t - sigma_n*s, the inverse of the order-1 row t -> n
        (x_n = s'*x_t + c'*eps(x_t, t) solved for x_t: x_t = s*x_n + c*eps(x_t, t), an implicit equation).
        Each leg is 1 + refine rows with the same (s, c).  Row 0, the predictor, evaluates the model where the state is known:
        t_model = the lower index + 1 (1 on the first leg) and the model's input is base -- textbook DDIM inversion.  Rows
        1..refine, the correctors, are fixed-point iterations of the implicit equation: t_model = the target index + 1 and the
        model's input is the previous row's result.  commit = 1 on the leg's last row only.
        All arithmetic in float64 on the float32 schedule widened; the result is cast to `dtype` once."""
        refine = int(refine)
        if refine < 0:
            raise ValueError(f"encode_table: refine = {refine}")
        taus = [int(t) for t in taus]
        assert len(taus) >= 1 and taus[-1] == 0, "the last index is 0"
        assert all(a > b for a, b in zip(taus, taus[1:])), "descending distinct indices"
        ab, _ = self._half_logsnr()
        alpha, sigma = np.sqrt(ab), np.sqrt(1.0 - ab)
        table = np.zeros((len(taus) * (1 + refine), 8), np.float64)
        low = None
        for leg, t in enumerate(reversed(taus)):
            if low is None:
                s, c = alpha[t], sigma[t]
            else:
                s = alpha[t] / alpha[low]
                c = sigma[t] - sigma[low] * s
            rows = table[leg * (1 + refine):(leg + 1) * (1 + refine)]
            rows[:, 0] = t + 1
            rows[0, 0] = 1 if low is None else low + 1
            rows[:, 1], rows[:, 2] = s, c
            rows[-1, 3] = 1.0
            low = t
        return table.astype(dtype)

    def _noise(self, size, source, device):
        if source == 'cpu':  # the reference's stream: torch.randn(size).to(device), :465-466
            return torch.randn(size).to(device)
        return torch.randn(size, device=device)

    # ---- samplers ------------------------------------------------------------------------------
    def _eps_hat(self, model, x, t_model, condition_input, clip_feat, enable_autocast, kwargs):
        """one model evaluation of an eager loop: the noise prediction at x for the model's timestep t_model (schedule index
        + 1) on every sample, mixed with x's component where the model asks for it; float32, contiguous"""
        timestep = torch.full((x.shape[0],), t_model, dtype=torch.int64, device=self.device)
        mixing = self.get_mixing_component(x, timestep, enabled=getattr(model, 'mixed_prediction', False))
        with torch.autocast("cuda", enabled=enable_autocast):
            pred = model(x=x, t=timestep.float(), condition_input=condition_input, clip_feat=clip_feat, **kwargs)
            return _mixed(model, pred, mixing).float().contiguous()

    def _replay(self, model, num_samples, shape, mode, x, table, seed, condition_input, clip_feat, capacity=None, keys=None,
                first_row=None, known=None, **run):
        """the graphed branch of every sampler: the captured chain of (model, mode, batch shape) from this object's cache, run
        from x over `table`; seed None: one is drawn with chain.draw_seed() once the chain is there; `run`: GraphedChain.run's
        keywords.  keys (a list of num_samples 64-bit keys) in place of seed: the keyed capture of a mode that draws.
        first_row (num_samples ints, with keys; DDPM only): the per-sample-start capture, a cache entry of its own.
        known (GraphedChain.run's triple, with first_row): the known-region capture, another entry of its own; with a fourth
        element, the jump table, the resampling capture, one more.
        Returns the final latent."""
        keyed = keys is not None and mode in _chain.KEYED_MODES
        more = {"resample": True} if known is not None and len(known) == 4 else {}
        ch = self._chains.get(model, num_samples, shape, condition_input, clip_feat, self.device, mode,
                              self._diffusion_steps if capacity is None else capacity, keyed=keyed,
                              from_rows=first_row is not None, known=known is not None, **more)
        if known is not None:
            return ch.run(x, table, keys, condition_input, clip_feat, first_row=first_row, known=known, **run)
        if first_row is not None:
            return ch.run(x, table, keys, condition_input, clip_feat, first_row=first_row, **run)
        if keyed:
            return ch.run(x, table, keys, condition_input, clip_feat, **run)
        return ch.run(x, table, _chain.draw_seed() if seed is None else seed, condition_input, clip_feat, **run)

    # ---- per-shape seeds ---------------------------------------------------------------------------------
    @staticmethod
    def _sample_keys(who, seeds, num_samples, **excluded):
        """`seeds` of a sampler call as a list of num_samples 64-bit keys (None: None).  ValueError -- before any launch -- on a
        wrong count, or where one of `excluded` (name=value: the arguments seeds cannot be combined with) is set."""
        if seeds is None:
            return None
        keys = _chain.sample_keys(seeds, num_samples, who)
        for name, value in excluded.items():
            if value is not None:
                raise ValueError(f"{who}: seeds cannot be combined with {name}")
        return keys

    # ---- per-sample start steps --------------------------------------------------------------------------
    @staticmethod
    def per_sample_indices(who, value, num_samples, lo, hi, lists=False):
        """`value` as B per-sample schedule indices: None where it is not that form (an int, or anything the caller's own check
        refuses), else a list of num_samples ints in lo ... hi.  The form is a 1-D integer tensor or numpy array; with `lists`
        a list or tuple of ints too.  ValueError -- host work only, before any launch -- on bool entries, another dtype or
        rank, a wrong count, or an entry outside the range."""
        if isinstance(value, torch.Tensor):
            ok = value.dim() == 1 and value.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
            entries = value.detach().cpu().tolist() if ok else None
        elif isinstance(value, np.ndarray):
            ok = value.ndim == 1 and value.dtype.kind in "iu"
            entries = value.tolist() if ok else None
        elif lists and isinstance(value, (list, tuple)):
            ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in value)
            entries = [int(v) for v in value] if ok else None
        else:
            return None
        if not ok:
            raise ValueError(f"{who}: per-sample indices are a 1-D integer tensor or array (no bools), got {value!r}")
        if len(entries) != int(num_samples):
            raise ValueError(f"{who}: {len(entries)} per-sample indices for {num_samples} samples")
        if any(not lo <= v <= hi for v in entries):
            raise ValueError(f"{who}: per-sample indices {entries!r} outside [{lo}, {hi}]")
        return entries

    @staticmethod
    def _call_keys(keys, seed, num_samples):
        """the keys of a per-sample-start call, which is always keyed: `keys` (from seeds=) where given, else one key per sample
        split from `seed` (None: chain.draw_seed(), so torch.manual_seed governs it)"""
        if keys is not None:
            return keys
        return _chain.split_seed(_chain.draw_seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF, int(num_samples))

    def _keyed_start(self, keys, num_samples, shape):
        """the start latent of a keyed chain: sample b under keys[b] at LION_START_STEP_WORD, stream 0"""
        return diffusion_ops.philox_normal_keyed(keys, num_samples, shape, _chain.START_STEP_WORD, device=self.device)

    def _keyed_step_noise(self, words, num_samples, shape, row):
        """the z a keyed captured chain draws at table row `row` (stream 0), for the eager loops"""
        return diffusion_ops.philox_normal_keyed(words, num_samples, shape, int(row), device=self.device)

    @torch.no_grad()
    def run_denoising_diffusion(self, model, num_samples, shape, temp=1.0, enable_autocast=False,
                                is_image=False, prior_var=1.0, condition_input=None, given_noise=None,
                                clip_feat=None, cls_emb=None, grid_emb=None, graph=True, keep_trajectory=True,
                                noise_scale=None, conv_precision="fp32", *, seeds=None, x_noisy=None):
        """Ancestral DDPM sampling, T model evaluations (reference :224-303).  ``noise_scale(t)`` overrides the
        per-step noise standard deviation sqrt(beta_t) (LION.sample's scheduler variance).
        conv_precision="half": the denoiser's voxel convolutions run at reduced precision (conv_ops.PRECISION).
        seeds: num_samples ints (a sequence or an int64 tensor, each taken mod 2^64), the Philox key of each sample's chain: the
        step at table row i adds to sample b the noise of counter word i, stream 0, under seeds[b], and the start latent is the
        draw under the same key at LION_START_STEP_WORD (unless x_noisy, the start in place of a draw, is given).  No draw of
        the call touches torch's global generators; graph=True (the keyed capture, a cache entry beside the unkeyed one) and
        graph=False (lion_philox_normal_keyed + lion_ddpm_update) give the same bits.  A sample's NOISE then depends on its
        seed alone -- not on num_samples, its position, or its batchmates.  Its result is promised bit-equal only at equal
        num_samples: other batch sizes select other kernel plans in the denoiser (the split 1x1 convolution from 8192 columns,
        the conv tile plans).  ValueError before any launch: len(seeds) != num_samples, or seeds with given_noise."""
        keys = self._sample_keys("run_denoising_diffusion", seeds, num_samples, given_noise=given_noise)
        if x_noisy is not None and given_noise is not None:
            raise ValueError("run_denoising_diffusion: x_noisy and given_noise both name the start")
        with _sampling(model, conv_precision):
            dev = self.device
            size = [num_samples] + list(shape)
            if x_noisy is not None:
                x_noisy = x_noisy.to(dev)
            elif keys is not None:
                x_noisy = self._keyed_start(keys, num_samples, shape)
            else:
                x_noisy = torch.randn(size=size, device=dev) if given_noise is None else given_noise[0].to(dev)
            x_noisy = x_noisy.contiguous()
            output_list = {'pred_x': []}
            kwargs = {'grid_emb': grid_emb} if grid_emb is not None else {}
            if cls_emb is not None:
                condition_input = cls_emb if condition_input is None else torch.cat([condition_input, cls_emb], dim=1)
            T = self._diffusion_steps
            if graph and given_noise is None and _chain.graphable(model, x_noisy, enable_autocast, kwargs):
                x_image = self._replay(model, num_samples, shape, _chain.DDPM, x_noisy, self.ddpm_table(T, temp, noise_scale),
                                       None, condition_input, clip_feat, keys=keys,
                                       trajectory=output_list['pred_x'] if keep_trajectory else None,
                                       trajectory_before_last=True)
            else:
                x_image = self._ancestral_steps(model, x_noisy, T, temp, enable_autocast, condition_input, given_noise,
                                                clip_feat, kwargs, output_list['pred_x'], keys=keys)
            if is_image:
                x_image = (x_image.clamp(min=-1., max=1.) + 1.0) / 2.0
            return x_image, output_list

    def _ancestral_steps(self, model, x_noisy, t_from, temp, enable_autocast, condition_input, given_noise, clip_feat, kwargs,
                         states, generator=None, keys=None):
        """the eager ancestral steps t = t_from-1 ... 0 from x_noisy; returns the posterior mean of the step at t = 0.  The noise
        of step t is given_noise[1][t] where given, else a device draw (from `generator` if one is passed).  `states` (a list,
        or None) receives the state after every step -- for t = 0 the state BEFORE it once more, as the reference reports it.
        keys (one 64-bit key per sample): the step at t draws what the keyed captured chain draws at its table row
        t_from - 1 - t."""
        dev, size = self.device, list(x_noisy.shape)
        x_image = None
        words = None if keys is None else _chain.key_words(keys, dev)
        for t in reversed(range(0, t_from)):
            eps_hat = self._eps_hat(model, x_noisy, t + 1, condition_input, clip_feat, enable_autocast, kwargs)
            is0, k_outer, k_a, k_b, scale = self.ddpm_coefficients(t)
            if is0:
                x_image = diffusion_ops.ddpm_update(x_noisy, eps_hat, None, True, k_outer, k_a, k_b, scale, temp)
            else:
                if words is not None:
                    z = self._keyed_step_noise(words, size[0], size[1:], t_from - 1 - t)
                else:
                    z = (torch.randn(size=size, device=dev, generator=generator) if given_noise is None
                         else given_noise[1][t].to(dev)).contiguous()
                x_noisy = diffusion_ops.ddpm_update(x_noisy, eps_hat, z, False, k_outer, k_a, k_b, scale, temp)
            if states is not None:
                states.append(x_noisy)
        return x_image

    # ---- diffuse-denoise: the forward draw at an index, and the reverse chain from there -----------------------------------
    def diffuse(self, x0, t, noise=None, seed=None, return_noise=False, *, seeds=None):
        """x_t = sqrt(alpha_bar_t) * x0 + sqrt(1 - alpha_bar_t) * z at the schedule INDEX t, 0 <= t <= T-1: what
        ``sample_q`` gives on the quantities of ``iw_quantities_t(B, full(t))`` (reference :44-113; the model's timestep there
        is t + 1).  The two scalars are those expressions on the host copy of the float32 schedule, each operation rounded
        once -- no device synchronisation; a device library's sqrt may differ from them in the last bit -- and the
        draw is one kernel (lion_chain_diffuse): z = ``noise`` if given, else N(0, 1) from the chain's Philox generator under
        ``seed`` (None: one is drawn with chain.draw_seed(), so torch.manual_seed governs it), on a stream of its own, so that
        a chain run under the same seed repeats none of it.  return_noise: (x_t, z).
        seeds: x0.shape[0] ints, one key per sample, in place of noise / seed (ValueError with either, or on a wrong count):
        sample b's z is drawn under seeds[b] at counters within the sample (lion_chain_diffuse_keyed), so it depends on
        neither the batch size nor the sample's position; torch's generators are not touched.
        t may also be B per-sample indices, a 1-D integer tensor or numpy array with entries up to T-1, a NEGATIVE entry
        meaning "skip this sample" (it comes back bit for bit and draws nothing): one launch of lion_chain_diffuse_keyed_at on
        the same host scalars, so that sample b is the bits of diffuse(x0, t[b], seeds=...).  This form is always keyed: the
        keys are `seeds`, or split_seed(seed, B) (seed None: one is drawn).  ValueError with noise, on a wrong count, bool
        entries or an entry above T-1."""
        B = x0.shape[0]
        per = self.per_sample_indices("diffuse", t, B, -2 ** 63, self._diffusion_steps - 1)
        if per is not None:
            if noise is not None:
                raise ValueError("diffuse: per-sample indices draw under per-sample keys and cannot be combined with noise")
            keys = self._call_keys(self._sample_keys("diffuse", seeds, B, seed=seed), seed, B)
            sqrt = lambda v: float(torch.sqrt(v))
            ms = [(1.0, 0.0) if i < 0 else (sqrt(self._h_alpha_bars[i]), sqrt(1.0 - self._h_alpha_bars[i])) for i in per]
            return diffusion_ops.diffuse_at(x0.contiguous(), ms, keys, return_noise=return_noise)
        if not isinstance(t, (int, np.integer)) or isinstance(t, bool) or not 0 <= t <= self._diffusion_steps - 1:
            raise ValueError(f"diffuse: t = {t!r} is not an index in [0, {self._diffusion_steps - 1}]")
        keys = self._sample_keys("diffuse", seeds, x0.shape[0], noise=noise, seed=seed)
        ab = self._h_alpha_bars[int(t)]
        m, s = float(torch.sqrt(ab)), float(torch.sqrt(1.0 - ab))
        if keys is not None:
            return diffusion_ops.diffuse(x0.contiguous(), m, s, seeds=keys, return_noise=return_noise)
        if noise is None and seed is None:
            seed = _chain.draw_seed()
        return diffusion_ops.diffuse(x0.contiguous(), m, s, noise=None if noise is None else noise.contiguous(), seed=seed,
                                     return_noise=return_noise)

    @torch.no_grad()
    def run_denoising_diffusion_from_t(self, model, num_samples, shape, time_start, x_noisy, temp=1.0, enable_autocast=False,
                                       is_image=False, prior_var=1.0, condition_input=None, given_noise=None, clip_feat=None,
                                       graph=True, keep_trajectory=True, conv_precision="fp32", *, seed=None, seeds=None,
                                       known=None, resample=None):
        """The tail of the ancestral chain from ``x_noisy`` (reference :504-563): the steps t = time_start-1 ... 0, the last of
        which returns the posterior mean; 1 <= time_start <= T, and time_start = T is the whole chain from a given start.
        Returns (x, output_list): output_list is the reference's plain list of the state after every step, whose last entry
        repeats the state before the final update (the reference appends x_noisy there, not the mean); empty with
        keep_trajectory=False.  given_noise = (unused, z) with z indexed by t, as in the reference: step t adds z[t].
        time_start = 0 returns (x_noisy, []) unchanged, where the reference would raise (its x_image is never assigned).
        is_image and prior_var are accepted and unused, as in the reference.
        graph=True: the tail is replayed on the captured chain of run_denoising_diffusion for this model and batch shape --
        the same cache entry, so a model that has sampled is not captured again -- with the schedule table's last
        time_start rows; the per-step noise is then the chain's Philox stream.
        seed (editing.diffuse_denoise): the 64-bit key of the tail's noise -- the chain's Philox key, or the seed of the eager
        loop's device generator -- in place of a draw from torch's global generators (graphed: chain.draw_seed()).
        seeds: one key per sample, as in run_denoising_diffusion: the tail's row i (t = time_start - 1 - i) adds to sample b the
        noise of counter word i under seeds[b]; graphed and eager tails give the same bits.  ValueError before any launch:
        len(seeds) != num_samples, or seeds with seed or given_noise.
        time_start may also be num_samples per-sample starts, a 1-D integer tensor or numpy array with entries in 0 ... T
        (DESIGN.md 4.6.9): sample b then comes back as from the uniform call with time_start[b] under the same seeds, bit for
        bit at equal num_samples, and a sample with start 0 as it went in.  The call runs S = max(time_start) replays of the
        per-sample-start capture (chain.GraphedChain(from_rows=True), a cache entry of its own) over ddpm_table(S, temp) with
        first_row[b] = S - time_start[b]: every sample is evaluated at every row and held -- its update discarded -- below its
        first row.  S = 0 returns (x_noisy, []) with no launch.  This form is always keyed: the keys are `seeds`, or
        split_seed(seed, num_samples) (seed None: one is drawn).  graph=False is the debug path: the uniform eager tail on the
        whole batch once per distinct start, merged per sample; the same bits.  ValueError: given_noise, a wrong count, bool
        entries, an entry outside 0 ... T.
        known = (x0, keep): region-preserving tail (RePaint's known-region conditioning, Lugmayr et al. 2022,
        Algorithm 1 without its resampling jumps).  x0 is the clean latent, [num_samples] + shape; keep a bool tensor
        [num_samples, P] over P groups of n/P consecutive elements of a sample's n (P divides n, n/P a multiple of 4: the local
        prior's P = N latent points of 4 floats).  After the step at t the kept groups are replaced by a fresh forward draw of
        x0 at the level the state now has, diffuse's scalars of index t-1 (known_levels), under the sample's key on
        chain.KNOWN_STREAM; after the step at t = 0 by x0 itself, so the kept groups of the result are x0 bit for bit.  temp
        scales the ancestral noise only.  time_start is an int or per-sample starts; both run on the known-region capture
        (GraphedChain(known=True), a cache entry of its own; an int is a first_row of zeros), and another mask, x0 or set of
        starts reuses it.  A sample below its first row is held, kept groups included.  Always keyed, like per-sample starts.
        graph=False composes lion_philox_normal_keyed, lion_chain_diffuse and a where on the mask after each eager step; the
        same bits.  ValueError before any launch: known with given_noise, an x0 of another shape, a mask that is not a bool
        tensor [num_samples, P], or a group width that is not a multiple of 4.
        resample (with known): RePaint's resampling jumps, which make the re-drawn part agree with the kept
        one.  An int R is n_resample at jump length 10 (RePaint's default), a pair is (jump_length, n_resample).  The call then
        replays the rows of resample_walk(time_start, jump_length, n_resample): after the step that reaches an anchor
        (jump_length, 2*jump_length, ... steps to go) the elements that are not kept move jump_length levels back up in ONE
        forward draw, on chain.RESAMPLE_STREAM, while the kept ones are drawn at that higher level; each anchor is visited
        n_resample times.  This runs on the resampling capture (GraphedChain(known=True, resample=True), one more cache entry)
        over resample_tables; output_list holds the state after every row, jump included.  n_resample = 1 is the call without
        resample: same capture, same launches, same bits.  graph=False adds lion_philox_normal_keyed, lion_chain_diffuse and
        a where on the elements that are not kept to the jump rows; the same bits.  ValueError before any launch: resample
        without known, with per-sample time_start (a sample's own walk would differ from its uniform call's) or with
        given_noise; a bool, a non-integer or a value below 1; a walk of more than 16*T rows."""
        who = "run_denoising_diffusion_from_t"
        keys = self._sample_keys(who, seeds, num_samples, seed=seed, given_noise=given_noise)
        starts = self.per_sample_indices(who, time_start, num_samples, 0, self._diffusion_steps)
        if resample is not None:
            resample = self.resample_pair(who, resample)
            if known is None:
                raise ValueError(f"{who}: resample needs known = (x0, keep): without a kept region there is nothing to agree with")
            if starts is not None:
                raise ValueError(f"{who}: resample cannot be combined with per-sample time_start (a sample's own walk would "
                                 f"differ from the walk of its uniform call)")
            if given_noise is not None:
                raise ValueError(f"{who}: resample draws under per-sample keys and cannot be combined with given_noise")
            if resample[1] == 1:                            # no jump is ever made: the known-region tail as it is
                resample = None
        if known is not None:
            return self._tails_known(model, num_samples, shape, starts, time_start, x_noisy, temp, enable_autocast,
                                     condition_input, given_noise, clip_feat, graph, keep_trajectory, conv_precision, seed, keys,
                                     known, resample)
        if starts is not None:
            return self._tails_from_rows(model, num_samples, shape, starts, x_noisy, temp, enable_autocast, condition_input,
                                         given_noise, clip_feat, graph, keep_trajectory, conv_precision, seed, keys)
        if isinstance(time_start, bool) or not isinstance(time_start, (int, np.integer)) \
                or not 0 <= time_start <= self._diffusion_steps:
            raise ValueError(f"run_denoising_diffusion_from_t: time_start = {time_start!r} outside [0, {self._diffusion_steps}]")
        output_list = []
        if time_start == 0:
            return x_noisy, output_list
        if not x_noisy.is_cuda:
            raise RuntimeError("lion_amd: expected a CUDA(HIP) tensor; there is no CPU path")
        if list(x_noisy.shape) != [num_samples] + list(shape):
            raise ValueError(f"run_denoising_diffusion_from_t: x_noisy {tuple(x_noisy.shape)} for {[num_samples] + list(shape)}")
        with _sampling(model, conv_precision):
            dev = self.device
            x_noisy = x_noisy.to(dev).contiguous()
            states = output_list if keep_trajectory else None
            if graph and given_noise is None and _chain.graphable(model, x_noisy, enable_autocast, {}):
                x = self._replay(model, num_samples, shape, _chain.DDPM, x_noisy, self.ddpm_table(int(time_start), temp), seed,
                                 condition_input, clip_feat, keys=keys, trajectory=states, trajectory_before_last=True)
            else:
                gen = None if seed is None else torch.Generator(device=dev).manual_seed(seed & 0x7FFFFFFFFFFFFFFF)
                x = self._ancestral_steps(model, x_noisy, int(time_start), temp, enable_autocast, condition_input, given_noise,
                                          clip_feat, {}, states, generator=gen, keys=keys)
            return x, output_list

    def _tails_from_rows(self, model, num_samples, shape, starts, x_noisy, temp, enable_autocast, condition_input, given_noise,
                         clip_feat, graph, keep_trajectory, conv_precision, seed, keys):
        """run_denoising_diffusion_from_t for per-sample starts (a list of num_samples ints in 0 ... T)"""
        who = "run_denoising_diffusion_from_t"
        if given_noise is not None:
            raise ValueError(f"{who}: per-sample starts draw under per-sample keys and cannot be combined with given_noise")
        output_list = []
        S = max(starts)
        if S == 0:
            return x_noisy, output_list
        if not x_noisy.is_cuda:
            raise RuntimeError("lion_amd: expected a CUDA(HIP) tensor; there is no CPU path")
        if list(x_noisy.shape) != [num_samples] + list(shape):
            raise ValueError(f"{who}: x_noisy {tuple(x_noisy.shape)} for {[num_samples] + list(shape)}")
        keys = self._call_keys(keys, seed, num_samples)
        first_row = [S - s for s in starts]
        with _sampling(model, conv_precision):
            x_noisy = x_noisy.to(self.device).contiguous()
            if graph and _chain.graphable(model, x_noisy, enable_autocast, {}):
                x = self._replay(model, num_samples, shape, _chain.DDPM, x_noisy, self.ddpm_table(S, temp), None,
                                 condition_input, clip_feat, keys=keys, first_row=first_row,
                                 trajectory=output_list if keep_trajectory else None, trajectory_before_last=True)
                return x, output_list
            # the uniform eager tail on the WHOLE batch once per distinct start (equal batch size: equal kernel plans); sample b
            # takes its result, and its state at row i, from the run of its own start, at that run's row i - first_row[b]
            x = x_noisy.clone()
            states = [x_noisy.clone() for _ in range(S)] if keep_trajectory else None
            for s in sorted(set(starts) - {0}):
                mine = [b for b in range(num_samples) if starts[b] == s]
                run_states = [] if keep_trajectory else None
                x_s = self._ancestral_steps(model, x_noisy, s, temp, enable_autocast, condition_input, None, clip_feat, {},
                                            run_states, keys=keys)
                x[mine] = x_s[mine]
                for j in range(s if keep_trajectory else 0):
                    states[S - s + j][mine] = run_states[j][mine]
            if keep_trajectory:
                output_list.extend(states)
            return x, output_list

    # ---- region-preserving tails ------------------------------------------------------------------------
    @staticmethod
    def known_region(who, known, num_samples, shape):
        """`known` of a sampler call as (x0, keep, elements per group): x0 [num_samples] + shape, keep a bool tensor
        [num_samples, P] with P dividing the per-sample element count n and n/P a multiple of 4.  ValueError otherwise.  Host
        work only: shapes and dtypes."""
        try:
            x0, keep = known
        except (TypeError, ValueError) as e:
            raise ValueError(f"{who}: known = (x0, keep), got {type(known).__name__}") from e
        size, n = [int(num_samples)] + list(shape), int(np.prod(shape))
        if not isinstance(x0, torch.Tensor) or list(x0.shape) != size:
            raise ValueError(f"{who}: known x0 {tuple(getattr(x0, 'shape', ()))} for {size}")
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or keep.dim() != 2 or keep.shape[0] != int(num_samples) \
                or keep.shape[1] == 0 or n % keep.shape[1] != 0:
            raise ValueError(f"{who}: known keep is a bool tensor [{num_samples}, P] with P dividing {n}, got "
                             f"{getattr(keep, 'dtype', type(keep).__name__)} {tuple(getattr(keep, 'shape', ()))}")
        width = n // int(keep.shape[1])
        if width % 4 != 0:
            raise ValueError(f"{who}: known keep has groups of {width} elements, must be a multiple of 4 (one mask byte per quad)")
        return x0, keep, width

    @staticmethod
    def resample_pair(who, resample):
        """`resample` of a sampler or editing call as (jump_length, n_resample): an int R is (10, R), RePaint's default jump
        length.  ValueError on anything else, a bool, or a value below 1.  Host work only."""
        pair = (10, resample) if isinstance(resample, (int, np.integer)) else resample
        if not isinstance(pair, (tuple, list)) or len(pair) != 2 \
                or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1 for v in pair):
            raise ValueError(f"{who}: resample = {resample!r}: an int n_resample >= 1 or a pair (jump_length, n_resample) of them")
        return int(pair[0]), int(pair[1])

    def _tails_known(self, model, num_samples, shape, starts, time_start, x_noisy, temp, enable_autocast, condition_input,
                     given_noise, clip_feat, graph, keep_trajectory, conv_precision, seed, keys, known, resample=None):
        """run_denoising_diffusion_from_t(known=): starts is the list of per-sample starts, or None where time_start is an int;
        resample is None or (jump_length, n_resample) with n_resample > 1, and then starts is None"""
        who = "run_denoising_diffusion_from_t"
        if given_noise is not None:
            raise ValueError(f"{who}: known draws under per-sample keys and cannot be combined with given_noise")
        x0, keep, width = self.known_region(who, known, num_samples, shape)
        if starts is None:
            if isinstance(time_start, bool) or not isinstance(time_start, (int, np.integer)) \
                    or not 0 <= time_start <= self._diffusion_steps:
                raise ValueError(f"{who}: time_start = {time_start!r} outside [0, {self._diffusion_steps}]")
            starts = [int(time_start)] * int(num_samples)
        output_list = []
        S = max(starts)
        if S == 0:
            return x_noisy, output_list
        # the walk's three tables, here so that a walk that is too long is refused before anything else happens
        tables = None if resample is None else self.resample_tables(S, *resample, temp=temp)
        if not x_noisy.is_cuda:
            raise RuntimeError("lion_amd: expected a CUDA(HIP) tensor; there is no CPU path")
        if list(x_noisy.shape) != [num_samples] + list(shape):
            raise ValueError(f"{who}: x_noisy {tuple(x_noisy.shape)} for {[num_samples] + list(shape)}")
        keys = self._call_keys(keys, seed, num_samples)
        first_row = [S - s for s in starts]
        if tables is None:
            tables = self.ddpm_table(S, temp), self.known_levels(S)
        table, ms, jump = tables[0], tables[1], tables[2:]
        # the resampling capture holds the longest walk it has run, and at least the plain chain
        more = {"capacity": max(self._diffusion_steps, int(table.shape[0]))} if jump else {}
        with _sampling(model, conv_precision):
            x_noisy = x_noisy.to(self.device).contiguous()
            x0, keep = x0.to(self.device).contiguous(), keep.to(self.device)
            states = output_list if keep_trajectory else None
            if graph and _chain.graphable(model, x_noisy, enable_autocast, {}):
                quads = keep.repeat_interleave(width // 4, dim=1)   # one byte per quad
                x = self._replay(model, num_samples, shape, _chain.DDPM, x_noisy, table, None, condition_input, clip_feat,
                                 keys=keys, first_row=first_row, known=(x0, quads, ms) + jump, trajectory=states,
                                 trajectory_before_last=True, **more)
            else:
                elems = keep.repeat_interleave(width, dim=1).view(x0.shape)
                x = self._known_steps(model, x_noisy, first_row, table, ms, enable_autocast, condition_input, clip_feat, states,
                                      keys, x0, elems, *jump)
            return x, output_list

    def _known_steps(self, model, x, first_row, table, ms, enable_autocast, condition_input, clip_feat, states, keys, x0, elems,
                     jump=None):
        """the eager form of the known-region chain, one row of `table` (ddpm_table) and `ms` (known_levels) at a time on the
        whole batch: the keyed ancestral update for the samples at or past their first row, under their own row count, then for
        their kept elements (`elems`, bool like x) the forward draw of x0 at the row's level -- lion_philox_normal_keyed on
        chain.KNOWN_STREAM into lion_chain_diffuse -- or x0 itself where s == 0; each a `where` on the batch.  `jump`
        (resample_tables' third array): where row i has sf != 0 the elements that are not kept then go through the same pair of
        launches on chain.RESAMPLE_STREAM with (mf, sf), from their update.  The step of row i is the one at t = table[i, 0] - 1.
        `states` as in _ancestral_steps."""
        dev, B, shape = self.device, x.shape[0], list(x.shape[1:])
        words = _chain.key_words(keys, dev)
        S = int(table.shape[0])
        per_sample = lambda flags: torch.tensor(flags, device=dev).view([B] + [1] * len(shape))
        for i in range(S):
            t = int(table[i, 0]) - 1                        # S - 1 - i on a plain tail
            eps_hat = self._eps_hat(model, x, t + 1, condition_input, clip_feat, enable_autocast, {})
            is0, k_outer, k_a, k_b, scale = self.ddpm_coefficients(t)
            m, s = float(ms[i, 0]), float(ms[i, 1])
            mf, sf = (1.0, 0.0) if jump is None else (float(jump[i, 0]), float(jump[i, 1]))
            new = x
            for f in sorted({f for f in first_row if f <= i}):      # the samples that count this row as their row i - f
                mine = per_sample([r == f for r in first_row])
                z = None if is0 else self._keyed_step_noise(words, B, shape, i - f)
                new = torch.where(mine, diffusion_ops.ddpm_update(x, eps_hat, z, is0, k_outer, k_a, k_b, scale,
                                                                  float(table[i, 5])), new)
                fresh = x0
                if s != 0.0:
                    z = diffusion_ops.philox_normal_keyed(words, B, shape, i - f, stream_id=_chain.KNOWN_STREAM, device=dev)
                    fresh = diffusion_ops.diffuse(x0, m, s, noise=z)
                new = torch.where(mine & elems, fresh, new)
                if sf != 0.0:                               # the jump: the other elements move back up from their update
                    z = diffusion_ops.philox_normal_keyed(words, B, shape, i - f, stream_id=_chain.RESAMPLE_STREAM, device=dev)
                    new = torch.where(mine & ~elems, diffusion_ops.diffuse(new, mf, sf, noise=z), new)
            if states is not None:
                states.append(x if i == S - 1 else new)             # the last entry repeats the state before the final update
            x = new
        return x

    @torch.no_grad()
    def run_ddim(self, model, num_samples, shape, temp=1.0, enable_autocast=False, is_image=True,
                 prior_var=1.0, condition_input=None, ddim_step=100, skip_type='uniform', kappa=1.0,
                 clip_feat=None, grid_emb=None, x_noisy=None, dae_index=-1, noise='device',
                 keep_trajectory=True, graph=True, given_noise=None, state_hook=None, conv_precision="fp32", *, seeds=None):
        """DDIM sampling with ``ddim_step`` model evaluations; kappa is DDIM's eta (reference :390-473).
        noise='cpu': EVERY draw of the chain -- the start and the per-step noise -- comes from torch's CPU generator, so
        that one seed gives one chain on any device (the reference draws the per-step noise there, :465-466, and the
        start on its device).  given_noise = (start, [z_0, z_1, ...]): run the eager loop on exactly these draws (the
        counterpart of run_denoising_diffusion's given_noise; tests replay a graphed chain's recorded noise with it).
        state_hook(i, x): called before the i-th model evaluation with the chain's latent, which it may overwrite in place
        (device-side launches only; known-region replacement, bench.py's forced clouds).
        conv_precision="half": the supported reduced-precision mode -- the denoiser's voxel convolutions at r = 16 / 32 run
        one fp16 product per operand pair on the project's own kernel, inside the captured chain (conv_ops.PRECISION;
        DESIGN.md 4.3).  enable_autocast is unrelated to it and keeps its behaviour.
        seeds: one key per sample, as in run_denoising_diffusion: the i-th step adds to sample b the noise of counter word i,
        stream 0, under seeds[b]; the start latent, unless x_noisy is given, is the draw under the same key at
        LION_START_STEP_WORD.  Graphed (the keyed capture) and eager (lion_philox_normal_keyed + lion_ddim_update) runs give the
        same bits, and torch's generators are not touched.  A sample's noise depends on its seed alone; its result is promised
        bit-equal only at equal num_samples (other batch sizes select other kernel plans).  ValueError before any launch:
        len(seeds) != num_samples, or seeds with given_noise or noise='cpu'."""
        keys = self._sample_keys("run_ddim", seeds, num_samples, given_noise=given_noise,
                                 **{"noise='cpu'": True if noise == 'cpu' else None})
        with _sampling(model, conv_precision):
            dev = self.device
            size = [num_samples] + list(shape)
            if given_noise is not None:
                x_noisy, noise = given_noise[0], 'given'
            if x_noisy is None and keys is not None:
                x_noisy = self._keyed_start(keys, num_samples, shape)
            if x_noisy is None:
                x_noisy = torch.randn(size=size).to(dev) if noise == 'cpu' else torch.randn(size=size, device=dev)
            x_noisy = x_noisy.to(dev).contiguous()
            steps = self.ddim_schedule(self._diffusion_steps, ddim_step, skip_type)
            kwargs = {'grid_emb': grid_emb} if grid_emb is not None else {}
            output_list = []
            if graph and noise == 'device' and _chain.graphable(model, x_noisy, enable_autocast, kwargs):
                x_noisy = self._replay(model, num_samples, shape, _chain.DDIM, x_noisy, self.ddim_table(steps, kappa), None,
                                       condition_input, clip_feat, keys=keys, trajectory=output_list if keep_trajectory else None,
                                       state_hook=state_hook)
                return x_noisy, output_list
            words = None if keys is None else _chain.key_words(keys, dev)
            for i, t in enumerate(steps):
                last = i == len(steps) - 1
                if last:
                    assert t == 0
                if state_hook is not None:
                    state_hook(i, x_noisy)
                s, c, sigma = self.ddim_coefficients(t, None if last else steps[i + 1], kappa)
                eps_hat = self._eps_hat(model, x_noisy, t + 1, condition_input, clip_feat, enable_autocast, kwargs)
                # the reference draws (and adds, scaled by sigma == 0) noise on the last step as well
                if noise == 'given':
                    z = given_noise[1][i].to(dev).contiguous() if sigma != 0.0 else None
                elif words is not None:
                    z = self._keyed_step_noise(words, num_samples, shape, i) if sigma != 0.0 else None
                else:
                    z = self._noise(size, noise, dev).contiguous() if (sigma != 0.0 or noise == 'cpu') else None
                x_noisy = diffusion_ops.ddim_update(x_noisy, eps_hat, z if sigma != 0.0 else None, s, c, sigma)
                if keep_trajectory:
                    output_list.append(x_noisy)
            return x_noisy, output_list

    @torch.no_grad()
    def run_dpm_solver(self, model, num_samples, shape, steps=20, order=2, skip_type='logsnr', x_noisy=None,
                       condition_input=None, clip_feat=None, enable_autocast=False, keep_trajectory=True, graph=True,
                       state_hook=None, conv_precision="fp32", stochastic=False, t_start=None, seed=None, *, seeds=None):
        """Deterministic few-step sampling with DPM-Solver++(2M) (Lu et al. 2022, Algorithm 2): the second-order multistep
        solver of the probability-flow ODE that run_ddim(kappa=0) integrates to first order.  At most ``steps`` model
        evaluations (solver_schedule removes duplicate indices), one per visited index of
        ``solver_schedule(steps, skip_type)``; coefficients from ``dpm_solver_table``; ``order=1`` is DDIM with kappa = 0.
        skip_type='logsnr' (default) spaces the indices uniformly in log-SNR: with 'uniform' index spacing the last
        jump in lambda is so large that the second-order step is no better than DDIM.
        No noise enters after the start (x_noisy, or N(0, I) drawn on the device), so one start gives one result.
        Returns (x, output_list): output_list the state after every step (empty with keep_trajectory=False).
        graph=True: S replays of one captured step [prologue -> denoiser -> lion_chain_update_multistep], the latent and
        the previous data prediction in device memory (chain.DPMPP; a cache entry of its own beside the DDIM / DDPM
        captures of the same model).  Otherwise -- graph=False, mixed_prediction models, autocast -- the eager per-step loop
        on lion_dpmpp_update; from the same start the two give the same bits.
        state_hook(i, x) and conv_precision: as in run_ddim.
        stochastic=True: SDE-DPM-Solver++(2M), the same multistep update with the SDE's exponents and fresh noise at every
        step but the last (dpm_solver_table(stochastic=True); order 1 is DDIM with kappa = 1).  At equal steps it is LESS
        accurate than the deterministic solver: it buys stochasticity, which diffuse-denoise relies on.
        The noise comes from the chain's Philox generator under ``seed`` (None: chain.draw_seed(), so torch.manual_seed
        governs it), step i at counter word i, stream 0.  graph=True replays the chain.SDE_DPMPP capture [prologue -> denoiser
        -> lion_chain_update_multistep_noise], otherwise the eager loop runs lion_sde_dpmpp_update on the same seed, step
        words and stream: from the same start and seed the two give the same bits.
        t_start (an index in 1 ... T-1; needs x_noisy, else ValueError): the tail of the chain from x_noisy, taken as a draw
        of the marginal at index t_start (DiffusionDiscretized.diffuse(x0, t_start)), over
        solver_schedule(steps, skip_type, t_start).  Either solver runs it.
        seeds: one key per sample in place of seed, as in run_denoising_diffusion: the start latent, unless x_noisy is given, is
        sample b's draw under seeds[b] at LION_START_STEP_WORD, and with stochastic=True row i adds the noise of counter word i,
        stream 0, under seeds[b] (the keyed chain.SDE_DPMPP capture, or eagerly lion_philox_normal_keyed +
        lion_sde_dpmpp_update(noise=z): the same bits).  The deterministic solver draws nothing after the start and replays its
        existing capture.  torch's generators are not touched.  A sample's noise depends on its seed alone; its result is
        promised bit-equal only at equal num_samples (other batch sizes select other kernel plans).  ValueError before any
        launch: len(seeds) != num_samples, or seeds with seed."""
        keys = self._sample_keys("run_dpm_solver", seeds, num_samples, seed=seed)
        if t_start is not None and x_noisy is None:
            raise ValueError("run_dpm_solver: t_start needs x_noisy, the state at that index")
        taus = self.solver_schedule(steps, skip_type, t_start)
        table = self.dpm_solver_table(taus, order, stochastic=bool(stochastic))
        if stochastic and keys is None:
            seed = _chain.draw_seed() if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        with _sampling(model, conv_precision):
            dev = self.device
            if x_noisy is None and keys is not None:
                x_noisy = self._keyed_start(keys, num_samples, shape)
            if x_noisy is None:
                x_noisy = torch.randn(size=[num_samples] + list(shape), device=dev)
            x_noisy = x_noisy.to(dev).contiguous()
            output_list = []
            if graph and _chain.graphable(model, x_noisy, enable_autocast, {}):
                x = self._replay(model, num_samples, shape, _chain.SDE_DPMPP if stochastic else _chain.DPMPP, x_noisy, table,
                                 seed if stochastic else 0, condition_input, clip_feat,   # 0: the deterministic step draws nothing
                                 keys=keys if stochastic else None,
                                 trajectory=output_list if keep_trajectory else None, state_hook=state_hook)
                return x, output_list
            x, hist = x_noisy.clone(), None     # the hook may overwrite the latent in place: never the caller's tensor
            keyed = stochastic and keys is not None
            words = (_chain.key_words(keys, dev) if keyed else diffusion_ops.seed_words(seed, dev)) if stochastic else None
            for i, t in enumerate(taus):
                if state_hook is not None:
                    state_hook(i, x)
                eps_hat = self._eps_hat(model, x, t + 1, condition_input, clip_feat, enable_autocast, {})
                if keyed:        # row i of the keyed chain: counter word i, stream 0, under each sample's key; a6 == 0 draws nothing
                    z = self._keyed_step_noise(words, num_samples, shape, i) if table[i, 7] != 0 else None
                    x, hist = diffusion_ops.sde_dpmpp_update(x, eps_hat, hist, *[float(v) for v in table[i, 1:8]], noise=z)
                elif stochastic:   # step i of the captured chain: counter word i, stream 0
                    x, hist = diffusion_ops.sde_dpmpp_update(x, eps_hat, hist, *[float(v) for v in table[i, 1:8]], seed=words,
                                                             step=i)
                else:
                    x, hist = diffusion_ops.dpmpp_update(x, eps_hat, hist, *[float(v) for v in table[i, 1:7]])
                if keep_trajectory:
                    output_list.append(x)
            return x, output_list

    @torch.no_grad()
    def run_ddim_forward(self, dae, eps, ddim_step=20, ddim_skip_type='logsnr', condition_input=None, clip_feat=None, refine=0,
                         graph=True, keep_trajectory=False, enable_autocast=False, conv_precision="fp32"):
        """Deterministic few-step encoder: the latent ``eps`` [B, *shape] -> the noise x_T that regenerates it (the reference's
        run_ddim_forward, utils/diffusion_pvd.py:305-388, is an unfinished stub of this; its name and leading arguments are kept).
        Its decoder is ``run_dpm_solver(dae, B, shape, steps=ddim_step, order=1, skip_type=ddim_skip_type, x_noisy=x_T)``:
        the legs of ``solver_schedule(ddim_step, ddim_skip_type)`` are walked from the clean latent up to index T-1, each leg
        inverting the decoder's step over the same two indices (``encode_table``).
        refine=0 is textbook DDIM inversion: one model evaluation per leg, at the leg's LOW end -- not the inverse of the
        decoder, which evaluates at the high end.  refine=K adds K fixed-point iterations of the decoder step's implicit
        inverse x_t = s*x_n + c*eps(x_t, t) per leg, each one more model evaluation: at most ddim_step*(1 + K) in all.  The
        iteration contracts where |c|*Lip(eps) < 1; shown on a toy only, nothing is claimed for trained weights (DESIGN.md
        4.6.5).
        Returns (x_T, trajectory): trajectory the state after every leg (empty with keep_trajectory=False).  ``eps`` is never
        written.  graph=True: replays of one captured step [prologue -> denoiser -> lion_chain_update_encode] with the
        iterate and the leg's base in device memory (chain.ENCODE, a cache entry of its own).  Otherwise -- graph=False,
        mixed_prediction models, autocast -- the eager loop on lion_ddim_encode_update; the two give the same bits.
        conv_precision: as in run_ddim."""
        if not eps.is_cuda:
            raise RuntimeError("lion_amd: expected a CUDA(HIP) tensor; there is no CPU path")
        table = self.encode_table(self.solver_schedule(ddim_step, ddim_skip_type), refine)
        with _sampling(dae, conv_precision):
            num_samples, shape = eps.shape[0], list(eps.shape[1:])
            start = eps.detach().to(self.device).contiguous()
            output_list = []
            if graph and _chain.graphable(dae, start, enable_autocast, {}):
                x = self._replay(dae, num_samples, shape, _chain.ENCODE, start, table, 0, condition_input, clip_feat,
                                 capacity=max(self._diffusion_steps, len(table)),   # seed 0: the step draws nothing
                                 trajectory=output_list if keep_trajectory else None,
                                 trajectory_rows=lambda i: table[i, 3] != 0)
                return x, output_list
            x, base = start.clone(), start.clone()          # never the caller's tensor
            for row in table:
                eps_hat = self._eps_hat(dae, x, int(row[0]), condition_input, clip_feat, enable_autocast, {})
                commit = row[3] != 0
                diffusion_ops.ddim_encode_update(base, eps_hat, float(row[1]), float(row[2]), commit, out=x,
                                                 base_out=base if commit else None)
                if keep_trajectory and commit:
                    output_list.append(x.clone())
            return x, output_list
