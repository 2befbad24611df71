"""hipGraph replay of one denoiser evaluation, for callers that keep their own sampling loop.

One PVCNN2Prior forward is ~740 kernel launches; at ~4-5 us of host time per launch the eager step is host-bound for
several milliseconds.  Every operator of liblion_hip.so is capture-safe by contract (caller's stream, no allocation, no
synchronisation), so the forward is captured once per (model, batch shape) by ``chain.CapturedStep`` -- one graph on one
stream, the packed weights it points at pinned -- and replayed per call; only the inputs are copied into static buffers.
"""
from .chain import CapturedStep


class GraphedDenoiser:
    """callable with the denoisers' signature: model(x=..., t=..., condition_input=..., clip_feat=...)."""

    def __init__(self, model, x, t, condition_input=None, clip_feat=None, warmup: int = 2):
        self.model, self.warmup = model, warmup
        self.x = x.detach().clone()
        self.t = t.detach().clone()
        self.cond = None if condition_input is None else condition_input.detach().clone()
        self.clip = None if clip_feat is None else clip_feat.detach().clone()
        self.mixed_prediction = getattr(model, "mixed_prediction", False)
        self.mixing_logit = getattr(model, "mixing_logit", None)
        self.capture()

    def capture(self):
        def step():
            self.out = self.model(x=self.x, t=self.t, condition_input=self.cond, clip_feat=self.clip)
        self.step = None   # a stale capture gives its pool back before the new one takes its own
        self.step = CapturedStep(self.model, step, self.x, warmup=self.warmup, split=False)

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def __call__(self, x, t, condition_input=None, clip_feat=None, **kwargs):
        if not self.step.valid():   # the weights or a kernel-selecting switch changed: a fresh graph, never a stale one
            self.capture()
        self.x.copy_(x)
        self.t.copy_(t)
        if self.cond is not None and condition_input is not None and condition_input.data_ptr() != self.cond.data_ptr():
            self.cond.copy_(condition_input)
        if self.clip is not None and clip_feat is not None and clip_feat.data_ptr() != self.clip.data_ptr():
            self.clip.copy_(clip_feat)
        self.step.replay()
        return self.out
