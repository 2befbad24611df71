"""CPU suite of region-preserving diffuse-denoise: the two "_known" entry points are declared, bound,
exported, named in INTEGRATION.md and refuse bad arguments before any launch; every host refusal of the feature fires before
anything touches a device; the level table is diffuse's host scalars row by row and ends with (1, 0); the host half of the
sampler hands the chain first_row, the quad mask and that table."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_check import ROOT, declared_bound_and_exported

NEW = ("lion_chain_update_noise_keyed_known", "lion_chain_update_noise_cm_keyed_known")
EINVAL = -1


def test_symbols_declared_bound_exported_and_documented():
    declared_bound_and_exported(NEW)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, f"{name} is not named in INTEGRATION.md"
    from lion_amd import chain
    assert chain.KNOWN_STREAM == 2


def test_entry_points_refuse_bad_arguments_before_launching():
    from lion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15                  # 16-byte aligned, never dereferenced: every call returns first

    def flat(mode=1, x=a, eps=a, B=2, n=8, cur=a, first=a, keys=a, sid=0, x0=a, keep=a, ms=a, ksid=2, out=a, z=None):
        return lib.lion_chain_update_noise_keyed_known(mode, x, eps, B, n, cur, first, keys, sid, x0, keep, ms, ksid, out, z,
                                                       None)

    def cm(mode=1, x=a, eps=a, B=2, n=2, cur=a, first=a, keys=a, sid=0, x0=a, keep=a, ms=a, ksid=2, out=a, z=None):
        return lib.lion_chain_update_noise_cm_keyed_known(mode, x, eps, B, n, cur, first, keys, sid, x0, keep, ms, ksid, out, z,
                                                          None)

    for f in (flat, cm):
        for name in ("x", "eps", "cur", "keys", "out", "x0", "keep", "ms"):     # every required pointer; first_row may be NULL
            assert f(**{name: None}) == EINVAL, (f.__name__, name)
        for mode in (-1, 2):
            assert f(mode=mode) == EINVAL
        for sid in (0, 2, 7):                                                   # the known stream is not the step's stream
            assert f(sid=sid, ksid=sid) == EINVAL
        assert f(x=a + 4) == EINVAL and f(out=a + 8) == EINVAL and f(z=a + 4) == EINVAL      # alignment, as the keyed forms
        assert f(x0=a + 4) == EINVAL
        for B in (0, -1, 65536):                                                # B outside 1 ... 65535
            assert f(B=B) == EINVAL, (f.__name__, B)
        for n in (0, -4):
            assert f(n=n) == EINVAL, (f.__name__, n)
    assert flat(eps=a + 4) == EINVAL
    for n in (1, 2, 3, 5, 6, 1022):                         # a channel-major sample holds 4*N elements: always whole quads
        assert flat(n=n) == EINVAL, n


# ---- host refusals, on CPU tensors: ValueError before the "no CPU path" error ------------------------------------------------------
def _diffusion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    return DiffusionDiscretized(None, None, released_prior_cfg(), device="cpu")


class _Vae:
    def latent_shape(self):
        return [[128, 1, 1], [8192, 1, 1]]


def test_level_table_is_diffuses_host_scalars():
    d = _diffusion()
    T = d._diffusion_steps
    for S in (1, 2, 7, T):
        ms = d.known_levels(S)
        assert ms.shape == (S, 2) and ms.dtype == np.float32
        assert tuple(ms[-1]) == (1.0, 0.0)                  # the row of t = 0: the clean value itself
        for i in range(S - 1):
            t = S - 1 - i
            ab = d._h_alpha_bars[t - 1]                     # what diffuse(x0, t - 1) computes
            assert ms[i, 0] == np.float32(float(torch.sqrt(ab))) and ms[i, 1] == np.float32(float(torch.sqrt(1.0 - ab)))
            assert ms[i, 1] != 0.0
        assert np.array_equal(d.known_levels(S), ms)
    # the tail of a longer table: row i of known_levels(S) is the row of the same t in known_levels(T)
    assert np.array_equal(d.known_levels(T)[T - 7:], d.known_levels(7))
    for bad in (0, -1, T + 1):
        with pytest.raises(ValueError):
            d.known_levels(bad)


def test_sampler_refusals_come_before_any_launch():
    d = _diffusion()
    model, B, shape = torch.nn.Identity(), 3, [128, 1, 1]
    x = torch.zeros([B] + shape)
    keep = torch.zeros(B, 32, dtype=torch.bool)
    t = torch.tensor
    run = lambda start=3, **kw: d.run_denoising_diffusion_from_t(model, B, shape, start, x, **kw)
    bad = [
        lambda: run(known=(x, keep), given_noise=(x, [x] * 4)),                                    # known with given_noise
        lambda: run(t([3, 0, 2]), known=(x, keep), given_noise=(x, [x] * 4)),
        lambda: run(known=(x, keep.to(torch.uint8))), lambda: run(known=(x, keep.float())),        # the mask's dtype
        lambda: run(known=(x, keep.numpy())), lambda: run(known=(x, None)),
        lambda: run(known=(x, keep[:2])), lambda: run(known=(x, keep[0])),                         # ... and shape
        lambda: run(known=(x, keep.view(B, 32, 1))), lambda: run(known=(x, torch.zeros(B, 0, dtype=torch.bool))),
        lambda: run(known=(x, torch.zeros(B, 24, dtype=torch.bool))),                              # P does not divide n
        lambda: run(known=(x, torch.zeros(B, 64, dtype=torch.bool))),                              # groups of 2: not whole quads
        lambda: run(known=(x, torch.zeros(B, 128, dtype=torch.bool))),
        lambda: run(known=(x[:2], keep)), lambda: run(known=(x.view(B, 128), keep)),               # x0 of the wrong shape
        lambda: run(known=(None, keep)), lambda: run(known=x), lambda: run(known=(x, keep, keep)),
        lambda: run(t([3, 0]), known=(x, keep)), lambda: run(t([3, 0, d._diffusion_steps + 1]), known=(x, keep)),
        lambda: run(-1, known=(x, keep)), lambda: run(True, known=(x, keep)),
        lambda: run(known=(x, keep), seeds=[1, 2]), lambda: run(known=(x, keep), seeds=[1, 2, 3], seed=5),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was accepted")
    good = [
        lambda: run(known=(x, keep)), lambda: run(known=(x, keep), seeds=[1, 2, 3]), lambda: run(known=(x, keep), seed=5),
        lambda: run(t([3, 0, 2]), known=(x, keep)), lambda: run(known=(x, torch.ones(B, 1, dtype=torch.bool))),
        lambda: run(known=(x, torch.ones(B, 16, dtype=torch.bool)), graph=False),
    ]
    for f in good:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
    # nobody starts: the input comes back untouched, with no launch
    for zero in (0, torch.zeros(B, dtype=torch.int64)):
        out, states = run(zero, known=(x, keep))
        assert out is x and states == []


def test_diffuse_denoise_refusals_come_before_any_launch():
    from lion_amd.editing import diffuse_denoise
    d, vae = _diffusion(), _Vae()
    dae = [torch.nn.Identity(), torch.nn.Identity()]
    B, N = 3, 2048
    x = torch.zeros(B, N, 3)
    ok = torch.zeros(B, N, dtype=torch.bool)
    bad = [ok.to(torch.uint8), ok.float(), ok.numpy().astype(np.int64), ok[:2], ok[:, :1024], ok.view(B, N, 1), ok[0, :5],
           torch.zeros(N, 1, dtype=torch.bool), [1, 2, 3], "legs", 1]
    for v in bad:
        with pytest.raises(ValueError, match="keep"):
            diffuse_denoise(vae, dae, d, x, (0, 3), seeds=[1, 2, 3], keep=v)
    for steps in (2, 5):
        with pytest.raises(ValueError, match="solver_steps"):
            diffuse_denoise(vae, dae, d, x, (0, 3), seeds=[1, 2, 3], keep=ok, solver_steps=steps)

    class Odd(_Vae):                                        # 6 floats per point: a point is not a whole number of quads
        def latent_shape(self):
            return [[128, 1, 1], [N * 6, 1, 1]]
    with pytest.raises(ValueError, match="quads"):
        diffuse_denoise(Odd(), dae, d, x, (0, 3), seeds=[1, 2, 3], keep=ok)
    for v in (ok, ok[0], ok.numpy(), ok[0].numpy(), ok.tolist()):
        with pytest.raises(RuntimeError, match="no CPU path"):
            diffuse_denoise(vae, dae, d, x, (0, 3), seeds=[1, 2, 3], keep=v)


def test_known_chain_construction_refusals():
    from lion_amd import chain
    ident = torch.nn.Identity()
    combos = [dict(), dict(keyed=True), dict(from_rows=True)]               # anything but keyed + from_rows
    for kw in combos:
        with pytest.raises(ValueError, match="known|from_rows"):
            chain.GraphedChain(ident, 2, [128, 1, 1], None, None, "cpu", chain.DDPM, 8, known=True, **kw)
    for mode in (chain.DDIM, chain.DPMPP, chain.SDE_DPMPP, chain.ENCODE):   # from_rows exists for DDPM only
        with pytest.raises(ValueError):
            chain.GraphedChain(ident, 2, [128, 1, 1], None, None, "cpu", mode, 8, keyed=True, from_rows=True, known=True)
    cache = chain.ChainCache()
    for kw in (dict(), dict(keyed=True), dict(from_rows=True)):
        with pytest.raises(ValueError):
            cache.get(ident, 2, [128, 1, 1], None, None, "cpu", chain.DDPM, 8, known=True, **kw)


# ---- what the host half hands to the chain -----------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """a host tensor that says it lives on the device: lets the host half of a graphed call run up to its _replay"""
    is_cuda = True


def test_host_half_hands_first_row_quad_mask_and_levels(monkeypatch):
    from lion_amd import chain
    d = _diffusion()
    model, B, shape = torch.nn.Identity(), 4, [128, 1, 1]
    x = torch.arange(B * 128, dtype=torch.float32).view([B] + shape).as_subclass(_OnDevice)
    x0 = torch.ones([B] + shape)
    keep = torch.zeros(B, 16, dtype=torch.bool)             # 16 groups of 8 elements: two quads each
    keep[1, 3] = keep[2, 15] = keep[3, 0] = True
    calls = []

    def replay(model_, num_samples, shape_, mode, x_, table, seed, cond, clip, **kw):
        calls.append(dict(kw, mode=mode, table=table, seed=seed))
        return x_.clone()
    monkeypatch.setattr(d, "_replay", replay)
    monkeypatch.setattr(chain, "graphable", lambda *a: True)
    for starts, want_rows in ((torch.tensor([3, 0, 2, 3]), [0, 3, 1, 0]), (3, [0, 0, 0, 0])):
        calls.clear()
        d.run_denoising_diffusion_from_t(model, B, shape, starts, x, temp=0.75, seeds=[11, 12, 13, 14], known=(x0, keep),
                                         keep_trajectory=False)
        assert len(calls) == 1
        c = calls[0]
        assert c["first_row"] == want_rows and c["mode"] == chain.DDPM and c["keys"] == [11, 12, 13, 14] and c["seed"] is None
        assert np.array_equal(c["table"], d.ddpm_table(3, 0.75))            # temp scales the ancestral noise only
        kx0, quads, ms = c["known"]
        assert torch.equal(kx0, x0) and np.array_equal(ms, d.known_levels(3))
        assert quads.shape == (B, 32) and torch.equal(quads, keep.repeat_interleave(2, dim=1))
        assert quads[1].nonzero().flatten().tolist() == [6, 7] and quads[3].nonzero().flatten().tolist() == [0, 1]
    # without seeds the call is keyed all the same
    calls.clear()
    d.run_denoising_diffusion_from_t(model, B, shape, 3, x, seed=99, known=(x0, keep), keep_trajectory=False)
    assert calls[0]["keys"] == chain.split_seed(99, B)
    # a call without known hands the chain what it handed it before
    calls.clear()
    d.run_denoising_diffusion_from_t(model, B, shape, 3, x, seeds=[11, 12, 13, 14], keep_trajectory=False)
    assert "known" not in calls[0] and "first_row" not in calls[0]
    calls.clear()
    d.run_denoising_diffusion_from_t(model, B, shape, torch.tensor([3, 0, 2, 3]), x, seeds=[11, 12, 13, 14], keep_trajectory=False)
    assert "known" not in calls[0] and calls[0]["first_row"] == [0, 3, 1, 0]
