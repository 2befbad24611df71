"""Whole-step capture of a sampling chain -- what ``DiffusionDiscretized.run_ddim`` /
``run_denoising_diffusion`` / ``LION.sample`` run by default on the GPU.

One denoiser evaluation of the local prior is ~500 kernel launches; the reference's samplers
(utils/diffusion_pvd.py:224-303, :390-473) additionally issue ~10 elementwise launches, a ``torch.full`` and a
host-side ``randn`` + H2D copy per step.  Here a captured step holds
    lion_chain_begin_step  ->  denoiser forward  ->  the mode's update kernel (UPDATE below)
and a chain of S steps is S replays of it.  Two things live here, apart:
  * ``CapturedStep``: warm-up, capture and replay of ANY step given as a callable -- the one capture path of the package
    (this chain, ode.OdeGraph, graph.GraphedDenoiser).  One hipGraph for models without set abstraction (the global prior);
    for the point-voxel denoiser three single-branch graphs on the main stream and the step's FPS / ball-query chain as two
    graphs on a second stream, ordered by events between the launches.  A graph bakes in the packed-weight pointers of its
    model: it pins them, and ``valid()`` fails once any parameter (optimizer step, EMA swap, checkpoint load) or a
    kernel-selecting switch (``policy_key()``) changed -- the owner then captures again.
  * ``GraphedChain``: the chain's state, all of it in device memory -- the schedule table (timestep for the model + the
    update's coefficients, S x 8 floats uploaded once per chain), the step counter, the Philox seed, the latent ``x``
    (updated in place).  The host issues one to five ``hipGraphLaunch`` per step and never synchronises inside the chain.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from . import _lib, _wcache

# The chain's modes.  DDIM / DDPM: run_ddim / the ancestral chain and its tails.  DPMPP: the deterministic multistep solver
# DPM-Solver++(2M) (run_dpm_solver); the chain also owns `hist`, the previous step's data prediction.  SDE_DPMPP: its stochastic
# form (run_dpm_solver(stochastic=True)), which draws the step's noise like DDIM / DDPM and reads its scale from column 7 of the
# schedule table.  ENCODE: the deterministic encoder (run_ddim_forward: refined DDIM inversion, low noise -> high noise),
# x <- a0*base + a1*eps and, on a leg's last row, base <- x; the chain owns `base`, the state at the current leg's low end, beside
# `x`, the iterate the model reads.  DPMPP and ENCODE draw nothing: neither the seed nor `z` is read.
DDIM, DDPM, DPMPP, SDE_DPMPP, ENCODE = range(5)
# The kernel that ends a mode's captured step: the entry point and its arguments in order.  A name is that buffer of the chain
# (`z`: None unless the noise is recorded), a number goes as it is (the update's mode; Philox stream 0), "eps" is the model's
# output and "size" the element count -- where the model hands back its channel-major output (`cm_out`) the entry point is the
# "_cm" one of the same name and takes (num_samples, n_pts) there instead.
UPDATE = {
    DDIM: ("lion_chain_update_noise", (DDIM, "x", "eps", "size", "cur", "seed", 0, "x", "z")),
    DDPM: ("lion_chain_update_noise", (DDPM, "x", "eps", "size", "cur", "seed", 0, "x", "z")),
    DPMPP: ("lion_chain_update_multistep", ("x", "eps", "hist", "size", "cur", "x", "hist")),
    SDE_DPMPP: ("lion_chain_update_multistep_noise", ("x", "eps", "hist", "size", "cur", "table", "seed", 0, "x", "hist", "z")),
    ENCODE: ("lion_chain_update_encode", ("base", "eps", "size", "cur", "x", "base")),
}
# Per-sample keys (GraphedChain(keyed=True)): the modes that draw end their step with the "_keyed" entry point
# of the same name, which takes the chain's `keys` (int32[B, 2]: a 64-bit Philox key per sample) where the spec says "seed" and
# (num_samples, elements per sample) where it says "size".  DPMPP and ENCODE draw nothing and have no keyed form.
KEYED_MODES = (DDIM, DDPM, SDE_DPMPP)
# Per-sample start steps (GraphedChain(keyed=True, from_rows=True)): the keyed ancestral step ends with the
# "_from" entry point of the same name instead, which takes the chain's `first_row` (int32[B]) before the keys: sample b is held
# at the rows below first_row[b] and counts its own rows from there.  The same launch count as the keyed step.
FROM_ROWS_MODES = (DDPM,)
# Known region (GraphedChain(keyed=True, from_rows=True, known=True)): the per-sample-start step ends with the
# "_known" entry point instead, which takes the chain's `known_x0` (the clean latent), `keep` (uint8, a byte per quad) and
# `known_ms` (float32[capacity, 2], the forward process's scalars of the level the state has after each row) and this stream id
# behind the step's own: a kept quad is re-drawn from its clean value after every row, on a Philox stream of its own -- chain
# steps draw on stream 0, the forward draw (diffusion_ops.diffuse) on stream 1.  The same launch count as the keyed step.
KNOWN_STREAM = 2
# Resampling jumps (GraphedChain(..., known=True, resample=True)): the known-region step ends with the
# "_known_resample" entry point instead, which also takes the chain's `known_jump` (float32[capacity, 2], the forward move that
# ends each row, (1, 0) where there is none) and this stream id behind the known region's: the quads that are not kept are moved
# back up the chain by a draw on a Philox stream of its own.  The same launch count as the keyed step.
RESAMPLE_STREAM = 3
# the step words no chain step can have (a step's word is its row index < the table's capacity): include/lion_hip.h
START_STEP_WORD, DIFFUSE_STEP_WORD = 0xFFFFFFFE, 0xFFFFFFFF
_MASK64 = 0xFFFFFFFFFFFFFFFF


def split_seed(seed: int, n: int):
    """n 64-bit keys from one (SplitMix64, Steele et al. 2014): one seed -> a key per purpose, or per shape"""
    out, state = [], seed & _MASK64
    for _ in range(n):
        state = (state + 0x9E3779B97F4A7C15) & _MASK64
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
        out.append(z ^ (z >> 31))
    return out


def sample_keys(seeds, num_samples, who="seeds") -> list:
    """`seeds` -- a sequence or an integer tensor of num_samples ints -- as a list of Python ints mod 2^64; ValueError where the
    count is not num_samples.  Host work only."""
    if isinstance(seeds, torch.Tensor):
        seeds = seeds.detach().cpu().reshape(-1).tolist()
    elif isinstance(seeds, np.ndarray):
        seeds = seeds.reshape(-1).tolist()
    try:
        keys = [int(s) & _MASK64 for s in seeds]
    except TypeError as e:
        raise ValueError(f"{who}: a sequence or tensor of {num_samples} ints, got {seeds!r}") from e
    if len(keys) != int(num_samples):
        raise ValueError(f"{who}: {len(keys)} seeds for {num_samples} samples")
    return keys


def first_rows(first_row, num_samples) -> list:
    """`first_row` of a from_rows chain as a list of num_samples ints in 0 ... 2^31 - 1; ValueError otherwise.  Host work only."""
    rows = [int(r) for r in first_row]
    if len(rows) != int(num_samples) or any(not 0 <= r < 2 ** 31 for r in rows):
        raise ValueError(f"GraphedChain: first_row = {rows!r}: {num_samples} ints in [0, 2^31)")
    return rows


def key_words(keys, device=None):
    """a list of 64-bit keys as int32[B, 2], the (lo, hi) words the keyed kernels read from device memory (device None: host)"""
    k = np.array([[s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF] for s in keys], dtype=np.uint32).view(np.int32)
    t = torch.from_numpy(k)
    return t if device is None else t.to(device)


# tests: a list here makes every chain run append (start latent, [the noise each step drew]) -- what an eager loop needs
# to repeat a graphed chain draw for draw (run_ddim(given_noise=...)); chains are then captured with the noise output on
RECORD = None
TEMB_TABLE = __import__("os").environ.get("LION_TEMB_TABLE", "1") != "0"   # A/B: 0 = every step recomputes its time embedding
CHANNEL_MAJOR_EPS = __import__("os").environ.get("LION_CHAIN_CM_EPS", "1") != "0"   # A/B: 0 = the model transposes its output

def policy_key() -> tuple:
    """The module-level switches that decide WHICH kernels a forward launches: a captured graph is only valid for the
    setting it was captured under (flipping one of them re-captures instead of silently replaying the old launches)."""
    from . import conv_ops, fused_ops, geometry
    from .models import pvcnn2_ada
    return (pvcnn2_ada.SPARSE_CONV1, pvcnn2_ada.FUSE_INFERENCE, pvcnn2_ada.OVERLAP_POINT_BRANCH, geometry.ENABLED,
            geometry.SPLIT_GRAPH, conv_ops.SPLIT, fused_ops.PW_SPLIT, pvcnn2_ada.VOX_PLAN, TEMB_TABLE, fused_ops.MAX_RECOMPUTE,
            pvcnn2_ada.SKIP_UNREAD, pvcnn2_ada.SKIP_UNREAD_LEVEL2, CHANNEL_MAJOR_EPS, pvcnn2_ada.SA_GATHER, conv_ops.PRECISION)


def channel_major(model, shape) -> bool:
    """the model hands back its channel-major [B, 4, N] output and the step's last kernel reads it in that layout"""
    n_pts, n_cls = getattr(model, "num_points", 0), getattr(model, "num_classes", 0)
    return CHANNEL_MAJOR_EPS and hasattr(model, "geometry_source") and n_cls == 4 and int(np.prod(shape)) == n_pts * n_cls


def same_conditioning(owner, condition_input, clip_feat) -> bool:
    """owner.cond / owner.clip, the static conditioning buffers of a capture, can take these inputs"""
    same = lambda buf, new: (buf is None) == (new is None) and (buf is None or buf.shape == new.shape)
    return same(owner.cond, condition_input) and same(owner.clip, clip_feat)


class LRU:
    """a handful of captured objects by key (each holds the private memory pool of one forward pass)"""

    def __init__(self, capacity=4):
        self._entries, self._capacity = OrderedDict(), capacity

    def lookup(self, key, usable, build):
        """the entry of `key` if usable(entry); else it is dropped and build() takes its place"""
        hit = self._entries.get(key)
        if hit is not None and usable(hit):
            self._entries.move_to_end(key)
            return hit
        self._entries.pop(key, None)
        hit = self._entries[key] = build()
        while len(self._entries) > self._capacity:
            self._entries.popitem(last=False)
        return hit

    def clear(self):
        self._entries.clear()


class CapturedStep:
    """The capture machinery of every graphed driver (the chain below, ode.OdeGraph, graph.GraphedDenoiser).  ``step`` is a
    zero-argument callable that issues one step's launches on the current stream, reading and writing only buffers its
    caller owns; ``x`` is the static tensor ``model.geometry_source(x)`` derives the coordinates from.  Warm-up, capture
    (``split=None``: the split-geometry form where the switches and the model allow it; ``False``: always one graph) and
    the pinned packed weights live here, with what the graphs are valid for: ``fingerprint`` and ``policy``."""

    def __init__(self, model, step, x, *, warmup=2, split=None):
        self.model, self.x = model, x
        self.fingerprint, self.policy = _wcache.fingerprint(model), policy_key()
        self.pinned = []         # strong references to every packed / mirrored weight the captured launches point at
        dev = x.device
        # Split-graph geometry overlap (geometry.SPLIT_GRAPH, models with a geometry_source()): the FPS / ball-query chain of
        # a step depends on the coordinates of x alone, is latency bound (0.7 ms on 32 CUs) and, on one stream, serial.
        # A parallel BRANCH inside one hipGraph replays slower than one stream on ROCm 7.2 (geometry.py), but separate
        # graphs on separate streams do overlap.  So a step becomes three single-branch graphs:
        #     geometry stream:  [geo: coordinates of x -> FPS / ball-query chain]            (waits for the previous step)
        #     main stream:      [A: step prologue, forward up to the first use of a geometry result]
        #                       wait(geo)  [B: the rest of the forward, update + noise]
        # ordered with two events per step.  Models without set abstraction never reach "first use": one graph, as before.
        from . import geometry
        src = getattr(model, "geometry_source", None)
        self.geo_graphs = self.graph_b = self.graphs = self.waits = self.geo_plan = None
        if split is None:
            split = geometry.SPLIT_GRAPH and src is not None and not geometry.ENABLED
        main = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(main)
        with _wcache.pinning(self.pinned):
            with torch.no_grad(), torch.cuda.stream(side):
                for _ in range(warmup):   # first calls pack weights, set kernel attributes, fill caches
                    step()
            main.wait_stream(side)
            if split:
                # NORMAL priority: on a high-priority stream (geometry._side_stream) the same graphs take 15.3 ms per
                # step instead of 7.4 -- the main stream's queue starves while the 0.7-ms FPS kernels run (measured, round 3)
                self.geo_stream = torch.cuda.Stream(device=dev)
                self.ev_step = torch.cuda.Event()

                def geo(boundary=None):
                    mods, coords = src(x)
                    return geometry.compute_chain(mods, coords, boundary=boundary)
                self.geo_stream.wait_stream(main)
                with torch.no_grad(), torch.cuda.stream(self.geo_stream):
                    geo()
                main.wait_stream(self.geo_stream)
                torch.cuda.synchronize(dev)
                # geometry graphs: [stage 0: the 2048 -> 1024 FPS, 0.55 of the chain's 0.76 ms, and its ball queries] and
                # [the later stages] -- the forward waits for the first one only where it needs it (SA-1's grouping); the
                # second is long done when SA-2 asks (two cuts of the main graph instead of one: 0.2 ms less exposed)
                self.geo_graphs = [torch.cuda.CUDAGraph()]
                gs = torch.cuda.Stream(device=dev)
                gs.wait_stream(main)

                def geo_cut(i):
                    if i == 1:
                        self.geo_graphs[-1].capture_end()
                        self.geo_graphs.append(torch.cuda.CUDAGraph())
                        self.geo_graphs[-1].capture_begin(pool=self.geo_graphs[0].pool())
                with torch.no_grad(), torch.cuda.stream(gs):
                    self.geo_graphs[0].capture_begin()
                    try:
                        self.geo_plan = geo(geo_cut)
                    finally:
                        self.geo_graphs[-1].capture_end()
                main.wait_stream(gs)
                torch.cuda.synchronize(dev)
                self.geo_stage_of_graph = [0, self.geo_plan["stages"] - 1][:len(self.geo_graphs)]  # last stage each graph holds
                self.ev_geo = [torch.cuda.Event() for _ in self.geo_graphs]
                graphs, waits = [torch.cuda.CUDAGraph()], []   # main graphs; waits[k]: geometry graphs awaited before graphs[k+1]

                def on_use(first, last):   # called inside the forward, on the capturing stream
                    need = [g for g, st_ in enumerate(self.geo_stage_of_graph)
                            if st_ >= first and (g == 0 or self.geo_stage_of_graph[g - 1] < last)]
                    need = [g for g in need if not any(g in w for w in waits)]
                    if not need:
                        return
                    graphs[-1].capture_end()
                    waits.append(need)
                    graphs.append(torch.cuda.CUDAGraph())
                    graphs[-1].capture_begin(pool=graphs[0].pool())
                cap = torch.cuda.Stream(device=dev)
                cap.wait_stream(main)
                with torch.no_grad(), torch.cuda.stream(cap), geometry.external(self.geo_plan, on_use):
                    graphs[0].capture_begin()
                    try:
                        step()
                    finally:
                        graphs[-1].capture_end()
                main.wait_stream(cap)
                self.graph = graphs[0]
                if waits:
                    self.graphs, self.waits = graphs, waits
                    self.graph_b = graphs[1]
                else:              # the forward never asked for a geometry result: one graph, no geometry stream
                    self.geo_graphs = self.geo_plan = None
            else:
                self.graph = torch.cuda.CUDAGraph()
                with torch.no_grad(), torch.cuda.graph(self.graph):
                    step()
        self.pinned = list({id(v): v for v in self.pinned}.values())   # one reference per distinct object

    def replay(self):
        """one step on the current stream (+ the geometry stream in split mode)"""
        if self.graph_b is None:
            self.graph.replay()
            return
        main = torch.cuda.current_stream(self.x.device)
        self.ev_step.record(main)                 # x of this step is final (and last step's readers of the plan are done)
        self.geo_stream.wait_event(self.ev_step)
        with torch.cuda.stream(self.geo_stream):
            for g, ev in zip(self.geo_graphs, self.ev_geo):
                g.replay()
                ev.record(self.geo_stream)
        self.graphs[0].replay()                   # overlaps the geometry chain
        for k, need in enumerate(self.waits):
            for g in need:
                main.wait_event(self.ev_geo[g])
            self.graphs[k + 1].replay()

    def valid(self):
        """the graphs still point at the model's current weights and were captured under the current switches"""
        return self.fingerprint == _wcache.fingerprint(self.model) and self.policy == policy_key()


class GraphedChain:
    def __init__(self, model, num_samples, shape, condition_input, clip_feat, device, mode, capacity, warmup=2,
                 record_noise=False, keyed=False, from_rows=False, known=False, resample=False):
        """keyed: sample b draws its noise under its own key, seed[b], at counters that count within the sample (the "_keyed"
        update kernels) -- `seed` is then int32[num_samples, 2] and prepare() / run() take num_samples keys.
        from_rows (keyed DDPM chains only, else ValueError): the chain owns `first_row`, int32[num_samples], which prepare()
        uploads with the table; sample b is held at the rows below first_row[b] and then runs as a chain of its own that starts
        there (the "_from" update kernel).
        known (keyed from_rows chains only, else ValueError): the chain also owns `known_x0`, `keep` and `known_ms`, which
        prepare() fills; the quads marked in `keep` are replaced after every row by a forward draw of known_x0 at that row's
        level, after the last row by known_x0 itself (the "_known" update kernel).
        resample (known chains only, else ValueError): the chain also owns `known_jump`, which prepare() fills; the quads that
        are not kept end a row with the forward move it holds for that row (the "_known_resample" update kernel)."""
        self.model, self.mode, self.capacity, self.keyed = model, mode, int(capacity), bool(keyed)
        self.from_rows, self.known, self.resample = bool(from_rows), bool(known), bool(resample)
        dev = torch.device(device)
        size = [num_samples] + list(shape)
        per_sample = int(np.prod(shape))
        if self.from_rows and not (keyed and mode in FROM_ROWS_MODES):
            raise ValueError(f"GraphedChain: from_rows needs a keyed DDPM chain, got mode {mode}, keyed={bool(keyed)}")
        if self.known and not (keyed and self.from_rows):
            raise ValueError(f"GraphedChain: known needs keyed=True and from_rows=True, got keyed={bool(keyed)}, "
                             f"from_rows={self.from_rows}")
        if self.resample and not self.known:
            raise ValueError("GraphedChain: resample needs known=True")
        if keyed and mode not in KEYED_MODES:
            raise ValueError(f"GraphedChain: mode {mode} draws nothing and has no keyed form")
        if keyed and per_sample % 4 != 0:
            raise ValueError(f"GraphedChain: keyed noise needs a multiple of 4 elements per sample, got {per_sample}")
        self.x = torch.zeros(size, device=dev)
        self.t = torch.zeros(num_samples, device=dev)
        self.cond = None if condition_input is None else condition_input.detach().clone().contiguous()
        self.clip = None if clip_feat is None else clip_feat.detach().clone().contiguous()
        self.table = torch.zeros(self.capacity, 8, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        # two 32-bit words of the Philox key -- of the chain, or (keyed) of every sample
        self.seed = torch.zeros((num_samples, 2) if keyed else 2, dtype=torch.int32, device=dev)
        self.cur = torch.zeros(8, device=dev)
        self.first_row = torch.zeros(num_samples, dtype=torch.int32, device=dev) if self.from_rows else None   # 0: never held
        # known region: nobody kept and level (1, 0) until prepare() fills them -- the warm-up runs the plain "_from" update
        self.known_x0 = torch.zeros(size, device=dev) if self.known else None
        self.keep = torch.zeros(num_samples, per_sample // 4, dtype=torch.uint8, device=dev) if self.known else None
        self.known_ms = torch.tensor([1.0, 0.0], device=dev).repeat(self.capacity, 1) if self.known else None
        self.known_jump = torch.tensor([1.0, 0.0], device=dev).repeat(self.capacity, 1) if self.resample else None   # no jumps
        self.z = torch.zeros(size, device=dev) if record_noise and mode != ENCODE else None   # tests: the noise each step used
        self.hist = torch.zeros(size, device=dev) if mode in (DPMPP, SDE_DPMPP) else None   # the previous step's data prediction
        self.base = torch.zeros(size, device=dev) if mode == ENCODE else None   # ENCODE: the state at the leg's low end
        # identity rows until run() uploads a schedule: the warm-up / capture passes must run on finite values (an
        # all-zero DDPM row is 0/0 -> the second warm-up forward would voxelize NaN latents).  For the multistep update the
        # same row is x0 = x, D = 0, out = x, and column 7 is 0: SDE_DPMPP's warm-up draws nothing.  For ENCODE it is a0 = 1,
        # a1 = 0, commit = 1: x = base (zeros until prepare) and base = x.
        self.table[:, 0] = 1.0   # t_model
        self.table[:, 1] = 1.0   # a0: x passes through
        self.table[:, 3] = 1.0   # a2: DDPM divisor (DDIM: z has weight 1 -- finite)
        # The time embedding of a step depends on the step's timestep alone: its rows for the whole chain are computed once
        # per run() (model.time_embedding over the schedule) and a replayed step picks its row by the device-resident step
        # index -- instead of 7 (global prior) / 3 (local prior) launches per step that recompute it for every sample.
        self.temb_table = None
        if TEMB_TABLE and hasattr(model, "time_embedding") and not getattr(model, "embed_dim", 1) == 0:
            with torch.no_grad():
                row = model.time_embedding(torch.ones(1, device=dev))
            self.temb_table = torch.zeros((self.capacity,) + tuple(row.shape[1:]), device=dev)
            self.temb_row = torch.zeros((1,) + tuple(row.shape[1:]), device=dev)
        # the local prior hands back its channel-major [B, 4, N] output; the update reads it in that layout (round 6: no
        # transposing ATen copy at the end of a step)
        n_pts, n_cls = getattr(model, "num_points", 0), getattr(model, "num_classes", 0)
        self.cm_out = channel_major(model, shape) and not getattr(model, "mixed_prediction", False)

        def step():
            extra = {}
            if self.temb_table is not None:   # the step's time-embedding row, copied by the prologue kernel itself
                _lib.call("lion_chain_begin_step_temb", self.table, self.capacity, self.counter, self.t, num_samples, self.cur,
                          self.temb_table, self.temb_row.numel(), self.temb_row)
                extra["temb"] = self.temb_row
            else:
                _lib.call("lion_chain_begin_step", self.table, self.capacity, self.counter, self.t, num_samples, self.cur)
            if self.cm_out:
                extra["channel_major_out"] = True
            eps = model(x=self.x, t=self.t, condition_input=self.cond, clip_feat=self.clip, **extra).float().contiguous()
            assert not self.cm_out or tuple(eps.shape) == (num_samples, n_cls, n_pts)
            entry, spec = UPDATE[mode]
            given = {"eps": [eps], "size": [num_samples, n_pts] if self.cm_out else [self.x.numel()]}
            if self.keyed:
                spec = tuple("keys" if a == "seed" else a for a in spec)
                given["keys"] = [self.seed]
                if not self.cm_out:
                    given["size"] = [num_samples, per_sample]
            if self.from_rows:
                given["keys"] = [self.first_row, self.seed]
            if self.known:   # behind the step's stream id: the known region's buffers and its stream
                k = spec.index("keys") + 2
                spec = spec[:k] + ("known_x0", "keep", "known_ms", KNOWN_STREAM) \
                    + (("known_jump", RESAMPLE_STREAM) if self.resample else ()) + spec[k:]
            args = []
            for a in spec:
                args += given[a] if a in given else [getattr(self, a) if isinstance(a, str) else a]
            _lib.call(entry + ("_cm" if self.cm_out else "") + ("_keyed" if self.keyed else "")
                      + ("_known_resample" if self.resample else "_known" if self.known else "_from" if self.from_rows else ""),
                      *args)
        self.step = CapturedStep(model, step, self.x, warmup=warmup)

    def matches(self, condition_input, clip_feat):
        return same_conditioning(self, condition_input, clip_feat) and self.step.valid()

    @torch.no_grad()
    def run(self, x_init, table: np.ndarray, seed, condition_input=None, clip_feat=None, trajectory=None,
            trajectory_before_last=False, noise_trajectory=None, state_hook=None, trajectory_rows=None, first_row=None,
            known=None):
        """x_init: the chain's start; table [S, 8] float32 rows {t_model, a0..a5, a6} (a6: SDE_DPMPP's noise scale, 0 in
        every other mode); seed: the chain's 64-bit key -- of a keyed chain, a sequence or tensor of one key per sample.  Returns the final latent (a fresh tensor).  `trajectory`: list that receives a copy of x after
        every step (before the last step's update if `trajectory_before_last`, as run_denoising_diffusion reports it); with
        `trajectory_rows(i)`, a predicate on the step's index, only after the steps it holds for (the encoder: a leg's last
        row).
        `state_hook(i, x)`: called before step i's replay with the chain's latent buffer, which it may overwrite IN PLACE
        with launches on the current stream (no host synchronisation): inpainting / known-region replacement, or a
        benchmark forcing the states a trained model would visit (bench.py's forced clouds).
        `first_row` (a from_rows chain, where it is required): num_samples ints, the first table row each sample takes part in
        (S or more: held throughout).
        `known` (a known chain, where it is required): (x0, keep, ms) -- the clean latent, shaped like x_init; the mask, a
        device tensor [num_samples, elements per sample / 4], non-zero = kept; ms [S, 2] float32 on the host, row i the forward
        process's (m, s) of the level the state has after row i.  On a resample chain it is (x0, keep, ms, jump) with jump
        [S, 2] float32 on the host, row i the forward move (mf, sf) that ends row i, (1, 0) for none."""
        S = self.prepare(x_init, table, seed, condition_input, clip_feat, first_row, known)
        if RECORD is not None and self.z is not None and noise_trajectory is None:
            noise_trajectory = []
            RECORD.append((x_init.detach().clone(), noise_trajectory))
        for i in range(S):
            if trajectory is not None and trajectory_before_last and i == S - 1:
                trajectory.append(self.x.clone())
            if state_hook is not None:
                state_hook(i, self.x)
            self.replay()
            if noise_trajectory is not None and self.z is not None:
                noise_trajectory.append(self.z.clone())
            if trajectory is not None and not (trajectory_before_last and i == S - 1) \
                    and (trajectory_rows is None or trajectory_rows(i)):
                trajectory.append(self.x.clone())
        return self.x.clone()

    @torch.no_grad()
    def prepare(self, x_init, table: np.ndarray, seed, condition_input=None, clip_feat=None, first_row=None, known=None) -> int:
        """everything a chain needs in device memory before its first replay (on the current stream): the start latent, the
        conditioning, the schedule table, the time-embedding rows, the step counter and the Philox key (keyed: the keys, a
        sequence or tensor of one per sample; from_rows: `first_row`, one non-negative int per sample; known: the clean latent, the
        quad mask and the level table, as run() describes them).  Returns S."""
        S = int(table.shape[0])
        assert 1 <= S <= self.capacity and table.shape[1] == 8
        if self.from_rows != (first_row is not None):
            raise ValueError("GraphedChain: first_row goes with a from_rows chain, and only with it")
        if self.from_rows:
            rows = first_rows(first_row, self.x.shape[0])
            self.first_row.copy_(torch.tensor(rows, dtype=torch.int32))
        if self.known != (known is not None):
            raise ValueError("GraphedChain: known goes with a known chain, and only with it")
        if self.known:
            if len(known) != (4 if self.resample else 3):
                raise ValueError("GraphedChain: known = (x0, keep, ms), and (x0, keep, ms, jump) on a resample chain")
            x0, keep, ms = known[:3]
            ms = np.ascontiguousarray(ms, dtype=np.float32)
            if tuple(x0.shape) != tuple(self.x.shape) or tuple(keep.shape) != tuple(self.keep.shape) or ms.shape != (S, 2):
                raise ValueError(f"GraphedChain: known = (x0 {tuple(x0.shape)}, keep {tuple(keep.shape)}, ms {ms.shape}) for "
                                 f"{tuple(self.x.shape)}, {tuple(self.keep.shape)}, {(S, 2)}")
            self.known_x0.copy_(x0)
            self.keep.copy_(keep)
            self.known_ms[:S].copy_(torch.from_numpy(ms))
        if self.resample:
            jump = np.ascontiguousarray(known[3], dtype=np.float32)
            if jump.shape != (S, 2):
                raise ValueError(f"GraphedChain: known jump {jump.shape} for {(S, 2)}")
            self.known_jump[:S].copy_(torch.from_numpy(jump))
        self.x.copy_(x_init)
        if self.cond is not None:
            self.cond.copy_(condition_input)
        if self.clip is not None:
            self.clip.copy_(clip_feat)
        self.table[:S].copy_(torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)), non_blocking=False)
        if self.temb_table is not None:
            was_training = self.model.training
            self.model.eval()
            self.temb_table[:S].copy_(self.model.time_embedding(self.table[:S, 0].contiguous()))
            self.model.train(was_training)
        self.counter.zero_()
        if self.hist is not None:
            self.hist.zero_()
        if self.base is not None:
            self.base.copy_(self.x)
        if self.keyed:
            self.seed.copy_(key_words(sample_keys(seed, self.x.shape[0], "GraphedChain")))
        else:
            words = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
            self.seed.copy_(torch.from_numpy(words))
        return S


for _name in ("replay", "graph", "graphs", "graph_b", "geo_graphs", "pinned", "policy", "fingerprint"):   # the capture's
    setattr(GraphedChain, _name, property(lambda self, _name=_name: getattr(self.step, _name)))


class ChainCache(LRU):
    """the captured chains of one DiffusionDiscretized: (model, mode, batch shape, keyed, from_rows, known, resample) ->
    GraphedChain.  A keyed
    and an unkeyed capture of one (model, mode, shape) coexist, each in a slot of its own; the modes that draw nothing have the
    unkeyed capture only and serve a keyed call with it.  The per-sample-start capture (from_rows: keyed DDPM only, ValueError
    otherwise) is a third entry beside them and takes one of the four slots, and the known-region capture (known: keyed
    from_rows only, ValueError otherwise) a fourth.  The resampling capture (resample: known only, ValueError otherwise) is one
    more entry: a model that runs all five evicts the least recently used of them from the four slots."""

    def get(self, model, num_samples, shape, condition_input, clip_feat, device, mode, table_capacity, keyed=False,
            from_rows=False, known=False, resample=False):
        rec = RECORD is not None
        from_rows, known, resample = bool(from_rows), bool(known), bool(resample)
        keyed = bool(keyed) and (mode in KEYED_MODES or from_rows)   # from_rows on a mode without a keyed form: refused below
        return self.lookup(
            (id(model), mode, int(num_samples), tuple(shape), str(device), rec, keyed, from_rows, known, resample),
            lambda hit: hit.model is model and hit.capacity >= table_capacity and hit.matches(condition_input, clip_feat),
            lambda: GraphedChain(model, num_samples, shape, condition_input, clip_feat, device, mode, table_capacity,
                                 record_noise=rec, keyed=keyed, from_rows=from_rows, known=known, resample=resample))


def draw_seed() -> int:
    """64-bit Philox key for one chain, drawn from torch's default CPU generator: torch.manual_seed() keeps
    governing reproducibility, as it does for the reference's per-step randn."""
    return int(torch.empty((), dtype=torch.int64).random_().item()) & 0xFFFFFFFFFFFFFFFF


def graphable(model, x, enable_autocast, extra_kwargs) -> bool:
    """the chain graph covers the plain sampling configuration of every released model; anything else (mixed
    prediction, autocast, grid embeddings, CPU tensors) takes the eager loop."""
    return (x.is_cuda and not enable_autocast and not extra_kwargs
            and not getattr(model, "mixed_prediction", False) and not torch.is_grad_enabled())
