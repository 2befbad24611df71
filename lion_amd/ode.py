"""Probability-flow ODE solver of the continuous-time samplers -- scipy's RK45 with its state on the device.

The reference (utils/diffusion_continuous.py:90-255) integrates the PF-ODE with ``solve_ivp(method='RK45')`` through
torchdiffeq's scipy wrapper: the batch is ONE system of B*D unknowns in float64, and every function evaluation copies
the latent device -> host -> device around an eager model forward.  Here (csrc/ode.hip) y, the stage derivatives, the
stage combinations, the error norm and the step-size controller live in device memory:

    one evaluation      lion_ode_stage -> denoiser forward -> lion_ode_drift        (stage index in device memory)
    one attempted step  6 evaluations -> lion_ode_error_partials -> lion_ode_control -> ONE read of the control struct

With ``graph=True`` an evaluation is lion_ode_stage followed by the replay of [forward -> drift], which ``OdeGraph``
captures on its own buffers with ``chain.CapturedStep`` (split geometry stream, re-capture when the weights or the
kernel-selecting switches change); ``graph=False`` runs the same launches eagerly.  The solver's own reductions have a fixed order (no float atomics): a solve repeats
itself bit for bit whenever the model does.
"""
from __future__ import annotations

import struct

import numpy as np
import torch

from . import _lib
from . import chain as _chain

RUNNING, FINISHED, TOO_SMALL_STEP = 0, 1, -1
_CTRL = struct.Struct("<12d12i")   # lion_ode_ctrl (include/lion_hip.h)
CTRL_FIELDS = ("t", "h_abs", "t_bound", "direction", "rtol", "atol", "h", "t_new", "err_norm", "h0", "d1", "sign",
               "stage", "cur", "status", "step_rejected", "yslot", "fslot", "nfe", "n_accepted", "n_rejected",
               "accepted", "pad0", "pad1")
STAGE_F0 = 7   # the first evaluation of a solve: f0 = fun(t0, y0)


def pack_ctrl(**fields) -> bytes:
    vals = {k: 0 for k in CTRL_FIELDS}
    vals.update(fields)
    return _CTRL.pack(*(vals[k] for k in CTRL_FIELDS))


def unpack_ctrl(buf) -> dict:
    return dict(zip(CTRL_FIELDS, _CTRL.unpack(bytes(buf))))


def schedule_scalars(beta_start, beta_end, sigma2_0):
    """the fp32 constants torch applies to a float32 t in DiffusionVPSDE.g2 / var (diffusion_continuous.py:599-612)"""
    f = lambda v: float(np.float32(v))
    return (f(beta_start), f(beta_end - beta_start), f(-beta_start), f(0.5 * (beta_end - beta_start)), f(1.0 - sigma2_0))


class OdeState:
    """The device buffers of one solve of n unknowns (B samples): Y f64[2, n], K f64[7, n], the norm partials and the
    control struct, plus a pinned host mirror of the struct and the event the host waits on once per attempted step."""

    def __init__(self, n, B, device):
        self.n, self.B, self.device = int(n), int(B), torch.device(device)
        self.Y = torch.zeros(2, self.n, dtype=torch.float64, device=self.device)
        self.K = torch.zeros(7, self.n, dtype=torch.float64, device=self.device)
        self.partials = torch.zeros(max(1, _lib.load().lion_ode_partials_bytes(self.n) // 8), dtype=torch.float64,
                                    device=self.device)
        self.ctrl = torch.zeros(_CTRL.size, dtype=torch.uint8, device=self.device)
        self.host = torch.zeros(_CTRL.size, dtype=torch.uint8).pin_memory()
        self.event = torch.cuda.Event()
        self.x32 = torch.zeros(self.n, device=self.device)       # the model's inputs, written by the stage kernel
        self.t_model = torch.zeros(self.B, device=self.device)

    def reset(self, y0, t0, t_bound, rtol, atol, sign):
        """solve_ivp(fun, (t0, t_bound), y0, method='RK45', rtol, atol) from stage f0; y0 is widened to float64."""
        self.Y[0].copy_(y0.reshape(-1).to(torch.float64))
        direction = float(np.sign(t_bound - t0)) if t_bound != t0 else 1.0
        raw = pack_ctrl(t=float(t0), t_bound=float(t_bound), direction=direction, rtol=float(rtol), atol=float(atol),
                        sign=float(sign), stage=STAGE_F0)
        self.ctrl.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8), non_blocking=False)

    def stage(self):
        _lib.call("lion_ode_stage", self.Y, self.K, self.n, self.ctrl, self.x32, self.t_model, self.B)

    def drift(self, eps, sched, mix=None, cm_points=0):
        eps = eps.float().contiguous()
        a, b = (None, None) if mix is None else mix
        _lib.call("lion_ode_drift", eps, int(cm_points), self.x32, self.n, self.t_model, *sched, a, b,
                  0 if a is None else a.numel(), self.K, self.ctrl)

    def control(self):
        _lib.call("lion_ode_error_partials", self.Y, self.K, self.n, self.ctrl, self.partials)
        _lib.call("lion_ode_control", self.partials, self.n, self.ctrl)

    def read(self) -> dict:
        """the host's one synchronisation per attempted step: async copy to pinned memory + one event wait"""
        self.host.copy_(self.ctrl, non_blocking=True)
        self.event.record(torch.cuda.current_stream(self.device))
        self.event.synchronize()
        return unpack_ctrl(self.host.numpy().tobytes())

    def result(self, c) -> torch.Tensor:
        return self.Y[c["yslot"]]


def solve(state: OdeState, evaluate, max_attempts=1_000_000) -> dict:
    """Drive a reset ``state`` to the end of its span; ``evaluate()`` runs [stage -> model -> drift] once.
    Returns the final control struct; raises as solve_ivp reports a failure."""
    evaluate()                  # f0
    state.control()             # d0, d1 -> h0
    evaluate()                  # f1 at y0 + h0 * direction * f0
    state.control()             # d2 -> h_abs, the first attempt
    c = state.read()
    attempts = 0
    while c["status"] == RUNNING:
        for _ in range(6):
            evaluate()
        state.control()
        c = state.read()
        attempts += 1
        if attempts >= max_attempts:
            raise RuntimeError("lion_amd.ode: no end of the span after %d attempted steps" % attempts)
    if c["status"] == TOO_SMALL_STEP:
        raise RuntimeError("lion_amd.ode: the ODE solver failed: Required step size is less than spacing between "
                           "numbers (t = %r, h = %r)" % (c["t"], c["h_abs"]))
    return c


# ---- the denoiser as the right-hand side ---------------------------------------------------------------------------

_channel_major = _chain.channel_major   # the chain's rule, without its "not mixed_prediction": the drift mixes itself


def _mixing(model, mixing_logit=None):
    """(1 - sigmoid(logit), sigmoid(logit)) as torch computes them (get_mixed_prediction), or None when the model does
    not mix; ``mixing_logit`` replaces the model's own logit (sample_model_ode's override)"""
    if not getattr(model, "mixed_prediction", False):
        return None
    logit = model.mixing_logit if mixing_logit is None else mixing_logit
    coeff = torch.sigmoid(logit.detach()).float()
    return (1 - coeff).reshape(-1).contiguous(), coeff.reshape(-1).contiguous()


class OdeGraph:
    """[forward -> drift] of one (model, batch shape, schedule) captured once on this object's buffers: the model's
    inputs x / t / cond / clip and the solve's OdeState, whose stage kernel writes x and t."""

    def __init__(self, model, num_samples, shape, condition_input, clip_feat, device, sched):
        self.model, self.sched = model, sched
        self.cm = _channel_major(model, shape)
        self.cond = None if condition_input is None else condition_input.detach().clone().contiguous()
        self.clip = None if clip_feat is None else clip_feat.detach().clone().contiguous()
        # the warm-up / capture passes evaluate stage f0 of an all-zero state: finite, and reset before every solve
        self.state = OdeState(num_samples * int(np.prod(shape)), num_samples, device)
        self.x, self.t = self.state.x32.view([num_samples] + list(shape)), self.state.t_model
        self.state.reset(self.x, 1.0, 0.0, 1e-5, 1e-5, 1.0)
        self.mix = _mixing(model)   # the captured drift reads these two buffers: set_mixing() refreshes them per solve
        kw = {"channel_major_out": True} if self.cm else {}

        # the stage kernel is launched before the replay, not captured: in the split-geometry mode the replay starts the
        # FPS / ball-query graphs on a second stream from the model input (x), which must already hold this stage
        def step():
            pred = model(x=self.x, t=self.t, condition_input=self.cond, clip_feat=self.clip, **kw)
            self.state.drift(pred, self.sched, self.mix, model.num_points if self.cm else 0)
        self.step = _chain.CapturedStep(model, step, self.x)

    def matches(self, condition_input, clip_feat, sched):
        return _chain.same_conditioning(self, condition_input, clip_feat) and self.step.valid() and self.sched == sched

    def set_mixing(self, mixing_logit=None):
        mix = _mixing(self.model, mixing_logit)
        if mix is not None:
            if mix[0].numel() != self.mix[0].numel():
                raise ValueError("mixing_logit has %d elements, the model's has %d" % (mix[0].numel(), self.mix[0].numel()))
            self.mix[0].copy_(mix[0])
            self.mix[1].copy_(mix[1])

    def evaluate(self):
        self.state.stage()
        self.step.replay()


def eager_evaluator(st, model, shape, sched, condition_input=None, clip_feat=None, enable_autocast=False,
                    mixing_logit=None):
    """evaluate() of the eager loop: lion_ode_stage -> model forward -> lion_ode_drift on ``st``'s buffers"""
    cm = _channel_major(model, shape)
    mix = _mixing(model, mixing_logit)
    x = st.x32.view([st.B] + list(shape))
    kw = {"channel_major_out": True} if cm else {}

    def evaluate():
        st.stage()
        with torch.autocast("cuda", enabled=enable_autocast):
            pred = model(x=x, t=st.t_model, condition_input=condition_input, clip_feat=clip_feat, **kw)
        st.drift(pred, sched, mix, model.num_points if cm else 0)
    return evaluate


_GRAPHS = _chain.LRU()


def graph_for(model, num_samples, shape, condition_input, clip_feat, device, sched) -> OdeGraph:
    return _GRAPHS.lookup((id(model), int(num_samples), tuple(shape), str(device)),
                          lambda g: g.model is model and g.matches(condition_input, clip_feat, sched),
                          lambda: OdeGraph(model, num_samples, shape, condition_input, clip_feat, device, sched))


clear_graphs = _GRAPHS.clear


@torch.no_grad()
def integrate(model, y0, t0, t_bound, sign, rtol, atol, sched, condition_input=None, clip_feat=None, graph=True,
              enable_autocast=False, mixing_logit=None):
    """solve_ivp(RK45) of the VPSDE PF-ODE of ``model`` from y0 (any shape [B, ...]) over (t0, t_bound) -- the times as
    torchdiffeq hands them to scipy, ``sign`` = -1 for a reversed span; ``mixing_logit`` overrides the model's own.
    Returns (y at t_bound in fp32, control struct)."""
    B, shape = y0.shape[0], list(y0.shape[1:])
    use_graph = graph and y0.is_cuda and not enable_autocast
    if use_graph:
        g = graph_for(model, B, shape, condition_input, clip_feat, y0.device, sched)
        if g.cond is not None:
            g.cond.copy_(condition_input)
        if g.clip is not None:
            g.clip.copy_(clip_feat)
        g.set_mixing(mixing_logit)
        st = g.state
        st.reset(y0, t0, t_bound, rtol, atol, sign)
        c = solve(st, g.evaluate)
    else:
        st = OdeState(y0.numel(), B, y0.device)
        st.reset(y0, t0, t_bound, rtol, atol, sign)
        c = solve(st, eager_evaluator(st, model, shape, sched, condition_input, clip_feat, enable_autocast, mixing_logit))
    return st.result(c).float().view_as(y0).clone(), c
