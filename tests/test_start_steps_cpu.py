"""CPU suite of per-sample start steps: the three entry points are declared, bound, exported, named in
INTEGRATION.md and refuse bad arguments before any launch; every host refusal of the feature fires before anything touches a
device; first_row = max(start) - start, and a batch of zeros comes back untouched."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_check import ROOT, declared_bound_and_exported

NEW = ("lion_chain_update_noise_keyed_from", "lion_chain_update_noise_cm_keyed_from", "lion_chain_diffuse_keyed_at")
EINVAL = -1


def test_symbols_declared_bound_exported_and_documented():
    declared_bound_and_exported(NEW)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, f"{name} is not named in INTEGRATION.md"


def test_entry_points_refuse_bad_arguments_before_launching():
    from lion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15                  # 16-byte aligned, never dereferenced: every call returns first

    def flat(mode=1, x=a, eps=a, B=2, n=8, cur=a, first=a, keys=a, out=a, z=None):
        return lib.lion_chain_update_noise_keyed_from(mode, x, eps, B, n, cur, first, keys, 0, out, z, None)

    def cm(mode=1, x=a, eps=a, B=2, n=2, cur=a, first=a, keys=a, out=a, z=None):
        return lib.lion_chain_update_noise_cm_keyed_from(mode, x, eps, B, n, cur, first, keys, 0, out, z, None)

    def at(x=a, B=2, n=8, ms=a, keys=a, out=a, z=None):
        return lib.lion_chain_diffuse_keyed_at(x, B, n, ms, keys, 1, out, z, None)

    for f in (flat, cm):
        for name in ("x", "eps", "cur", "first", "keys", "out"):                # every required pointer, first_row among them
            assert f(**{name: None}) == EINVAL, (f.__name__, name)
        for mode in (-1, 2):
            assert f(mode=mode) == EINVAL
        assert f(x=a + 4) == EINVAL and f(out=a + 8) == EINVAL and f(z=a + 4) == EINVAL      # alignment, as the keyed forms
    assert flat(eps=a + 4) == EINVAL
    for name in ("x", "ms", "keys", "out"):
        assert at(**{name: None}) == EINVAL, name
    for f in (flat, cm, at):
        for B in (0, -1, 65536):                                                # B outside 1 ... 65535
            assert f(B=B) == EINVAL, (f.__name__, B)
        for n in (0, -4):
            assert f(n=n) == EINVAL, (f.__name__, n)
    for f in (flat, at):                                    # a channel-major sample holds 4*N elements: always whole quads
        for n in (1, 2, 3, 5, 6, 1022):
            assert f(n=n) == EINVAL, (f.__name__, n)


# ---- host refusals, on CPU tensors: ValueError before the "no CPU path" error ------------------------------------------------------
def _diffusion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    return DiffusionDiscretized(None, None, released_prior_cfg(), device="cpu")


class _Vae:
    def latent_shape(self):
        return [[128, 1, 1], [8192, 1, 1]]


def test_per_sample_indices_form_and_refusals():
    d = _diffusion()
    f = lambda v, **kw: d.per_sample_indices("who", v, 3, 0, 9, **kw)
    assert f(5) is None and f(np.int64(5)) is None and f(True) is None and f("abc") is None     # not the form: the caller's check
    assert f([1, 2, 3]) is None and f((1, 2, 3)) is None                    # a list is the form only where the caller says so
    assert f(torch.tensor([3, 0, 9])) == [3, 0, 9] and f(np.array([1, 2, 3], dtype=np.int32)) == [1, 2, 3]
    assert f([3, 0, 2], lists=True) == [3, 0, 2] and f((3, 0, 2), lists=True) == [3, 0, 2]
    assert all(type(v) is int for v in f(torch.tensor([3, 0, 9])))
    bad = [torch.tensor([1, 2]), np.array([1, 2, 3, 4]),                    # a wrong count
           torch.tensor([1, 2, 10]), np.array([-1, 2, 3]),                  # an index out of range
           torch.tensor([True, False, True]), np.array([True, False, True]),            # bool entries
           torch.tensor([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0]), torch.zeros(3, 1, dtype=torch.int64),
           torch.tensor(3), np.zeros((1, 3), dtype=np.int64)]
    for v in bad:
        with pytest.raises(ValueError):
            f(v)
    for v in ([1, 2], [1, 2, 10], [True, False, True], [1, 2.0, 3], [1, [2], 3]):
        with pytest.raises(ValueError):
            f(v, lists=True)


def test_sampler_refusals_come_before_any_launch():
    d = _diffusion()
    T = d._diffusion_steps
    model, B, shape = torch.nn.Identity(), 3, [128, 1, 1]
    x = torch.zeros([B] + shape)
    noise = (x, [x] * 4)
    t = torch.tensor
    bad = [
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0]), x),                       # a wrong count
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0, T + 1]), x),                # out of range
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, np.array([3, -1, 2]), x),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([True, False, True]), x),          # bool entries
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0, 2]), x, given_noise=noise),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0, 2]), x, seeds=[1, 2, 3], given_noise=noise),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0, 2]), x, seeds=[1, 2]),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0, 2]), x, seeds=[1, 2, 3], seed=5),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, [3, 0, 2], x),                       # a list is not the form
        lambda: d.diffuse(x, t([3, 0])),
        lambda: d.diffuse(x, t([3, 0, T])),
        lambda: d.diffuse(x, np.array([True, False, True])),
        lambda: d.diffuse(x, t([3, 0, 2]), noise=x),
        lambda: d.diffuse(x, t([3, 0, 2]), seeds=[1, 2]),
        lambda: d.diffuse(x, t([3, 0, 2]), seeds=[1, 2, 3], seed=5),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was accepted")
    good = [
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0, T]), x),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, np.array([3, 0, 2]), x, seeds=[1, 2, 3]),
        lambda: d.run_denoising_diffusion_from_t(model, B, shape, t([3, 0, 2], dtype=torch.int32), x, seed=5),
        lambda: d.diffuse(x, t([3, -1, T - 1])),
        lambda: d.diffuse(x, np.array([3, 0, 2]), seeds=[1, 2, 3]),
        lambda: d.diffuse(x, t([3, 0, 2]), seed=7),
    ]
    for f in good:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()


def test_diffuse_denoise_refusals_come_before_any_launch():
    from lion_amd.editing import diffuse_denoise
    d, vae = _diffusion(), _Vae()
    T = d._diffusion_steps
    dae = [torch.nn.Identity(), torch.nn.Identity()]
    x = torch.zeros(3, 2048, 3)
    t = torch.tensor
    bad = [
        t([3, 0]), np.array([3, 0, 2, 1]), (t([3, 0]), 2), (2, [3, 0]),     # a wrong count
        t([3, 0, T]), (2, (3, 0, T)), (np.array([3, -1, 2]), 2),            # an index out of range
        t([True, False, True]), (2, [True, False, True]), (np.array([True, False, True]), 2),          # bool entries
        [3, 0, 2], (3, 0, 2), [3], [],                                      # a top-level list of length != 2
        ([3, 0, 2], [1, 2, 0], [1, 1, 1]),
        t([3.0, 0.0, 2.0]), (2, [3, 0.5, 2]),
    ]
    for v in bad:
        with pytest.raises(ValueError, match="time_start|per-sample"):
            diffuse_denoise(vae, dae, d, x, v, seeds=[1, 2, 3])
    for v in (t([3, 0, 2]), ((3, 0, 2), 4), (4, np.array([1, 2, 0]))):      # per-sample indices with solver_steps
        with pytest.raises(ValueError, match="solver_steps"):
            diffuse_denoise(vae, dae, d, x, v, seeds=[1, 2, 3], solver_steps=3)
    good = [t([3, 0, 2]), np.array([3, 0, 2]), ((3, 0, 2), (1, 2, 0)), ([3, 0, 2], 4), (4, t([1, 2, 0])), (3, 0), [3, 0], 5]
    for v in good:
        with pytest.raises(RuntimeError, match="no CPU path"):
            diffuse_denoise(vae, dae, d, x, v, seeds=[1, 2, 3])
    # B = 2: a top-level pair of ints stays the (global, local) pair, whatever B is
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffuse_denoise(vae, dae, d, x[:2], (3, 0), seeds=[1, 2])


def test_from_rows_chain_construction_refusals():
    from lion_amd import chain
    ident = torch.nn.Identity()
    assert chain.FROM_ROWS_MODES == (chain.DDPM,)
    with pytest.raises(ValueError, match="from_rows"):                      # without keyed
        chain.GraphedChain(ident, 2, [128, 1, 1], None, None, "cpu", chain.DDPM, 8, from_rows=True)
    for mode in (chain.DDIM, chain.DPMPP, chain.SDE_DPMPP, chain.ENCODE):   # in another mode
        with pytest.raises(ValueError, match="from_rows"):
            chain.GraphedChain(ident, 2, [128, 1, 1], None, None, "cpu", mode, 8, keyed=True, from_rows=True)
    cache = chain.ChainCache()
    for mode, keyed in ((chain.DDPM, False), (chain.DDIM, True), (chain.DPMPP, True), (chain.ENCODE, False)):
        with pytest.raises(ValueError, match="from_rows"):
            cache.get(ident, 2, [128, 1, 1], None, None, "cpu", mode, 8, keyed=keyed, from_rows=True)
    assert chain.first_rows([0, 2, 5], 3) == [0, 2, 5] and chain.first_rows(np.array([1, 0]), 2) == [1, 0]
    for bad, n in (([0, 2], 3), ([0, -1, 2], 3), ([0, 2 ** 31, 2], 3)):
        with pytest.raises(ValueError, match="first_row"):
            chain.first_rows(bad, n)


# ---- first_row arithmetic and the S = 0 early return -------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """a host tensor that says it lives on the device: lets the host half of a graphed call run up to its _replay"""
    is_cuda = True


def test_first_row_is_max_start_minus_start(monkeypatch):
    from lion_amd import chain
    d = _diffusion()
    model, B, shape = torch.nn.Identity(), 4, [128, 1, 1]
    x = torch.arange(B * 128, dtype=torch.float32).view([B] + shape).as_subclass(_OnDevice)
    calls = []

    def replay(model_, num_samples, shape_, mode, x_, table, seed, cond, clip, **kw):
        calls.append(dict(kw, mode=mode, table=table, seed=seed, num_samples=num_samples))
        return x_.clone()
    monkeypatch.setattr(d, "_replay", replay)
    monkeypatch.setattr(chain, "graphable", lambda *a: True)
    for starts in ((3, 0, 2, 3), (1, 1, 1, 1), (0, 0, 7, 0), (d._diffusion_steps, 0, 1, 5)):
        calls.clear()
        out, states = d.run_denoising_diffusion_from_t(model, B, shape, torch.tensor(starts), x, temp=0.75,
                                                       seeds=[11, 12, 13, 14], keep_trajectory=False)
        S = max(starts)
        assert len(calls) == 1 and states == []
        c = calls[0]
        assert c["first_row"] == [S - s for s in starts] and min(c["first_row"]) == 0
        assert c["mode"] == chain.DDPM and c["keys"] == [11, 12, 13, 14] and c["seed"] is None
        assert c["table"].shape == (S, 8) and np.array_equal(c["table"], d.ddpm_table(S, 0.75))
        # row i of the table is the step at t = S - 1 - i: sample b's own row j = i - first_row[b] is the step at
        # t = start[b] - 1 - j, the row j of ITS uniform table
        for b, s in enumerate(starts):
            if s:
                assert np.array_equal(c["table"][S - s:], d.ddpm_table(s, 0.75))
    # without seeds the call is keyed all the same: one key per sample split from the seed
    calls.clear()
    d.run_denoising_diffusion_from_t(model, B, shape, np.array([3, 0, 2, 3]), x, seed=99, keep_trajectory=False)
    assert calls[0]["keys"] == chain.split_seed(99, B) and calls[0]["first_row"] == [0, 3, 1, 0]
    calls.clear()
    torch.manual_seed(5)
    want = chain.split_seed(chain.draw_seed(), B)
    torch.manual_seed(5)
    d.run_denoising_diffusion_from_t(model, B, shape, np.array([3, 0, 2, 3]), x, keep_trajectory=False)
    assert calls[0]["keys"] == want                         # neither seeds nor seed: torch.manual_seed governs the call
    # an int start takes the path it took before: no first_row
    calls.clear()
    d.run_denoising_diffusion_from_t(model, B, shape, 3, x, seeds=[11, 12, 13, 14], keep_trajectory=False)
    assert len(calls) == 1 and "first_row" not in calls[0]


def test_all_zero_starts_return_the_input_untouched():
    d = _diffusion()
    model, B, shape = torch.nn.Identity(), 3, [128, 1, 1]
    x = torch.randn([B] + shape)                            # a host tensor: any launch would raise
    for zeros in (torch.zeros(B, dtype=torch.int64), np.zeros(B, dtype=np.int32)):
        out, states = d.run_denoising_diffusion_from_t(model, B, shape, zeros, x, seeds=[1, 2, 3])
        assert out is x and states == []
        out, states = d.run_denoising_diffusion_from_t(model, B, shape, zeros, x)
        assert out is x and states == []
    assert model.training                                   # no sampling context was entered either
