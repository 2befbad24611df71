"""CPU suite of RePaint's resampling jumps on region-preserving diffuse-denoise: the walk against literal
lists and its invariants; the three host tables against ddpm_table / known_levels and the float32 expressions of the jump; the
exact two-coordinate Gaussian toy, which shows what the jumps are for; the two "_known_resample" entry points declared, bound,
exported, documented and refusing bad arguments before any launch; every host refusal of the feature; and what the host half of
the sampler hands to the chain."""
import ctypes
import os

import numpy as np
import pytest
import torch

from abi_check import ROOT, declared_bound_and_exported

NEW = ("lion_chain_update_noise_keyed_known_resample", "lion_chain_update_noise_cm_keyed_known_resample")
EINVAL = -1


def _diffusion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    return DiffusionDiscretized(None, None, released_prior_cfg(), device="cpu")


# ---- the walk ------------------------------------------------------------------------------------------------------------------
WALKS = {
    (5, 2, 2): [(4, 0), (3, 0), (2, 2), (3, 0), (2, 0), (1, 0), (0, 0)],
    (4, 2, 3): [(3, 0), (2, 2), (3, 0), (2, 2), (3, 0), (2, 0), (1, 0), (0, 0)],
    (3, 1, 2): [(2, 1), (2, 0), (1, 1), (1, 0), (0, 0)],
    (3, 5, 4): [(2, 0), (1, 0), (0, 0)],                    # no anchor: the plain tail
}


def test_walk_literals():
    d = _diffusion()
    for args, want in WALKS.items():
        assert d.resample_walk(*args) == want, args


def test_walk_invariants_and_row_count():
    d = _diffusion()
    T = d._diffusion_steps
    cases = [(t, j, R) for t in (1, 2, 9, 10, 19, 20, 21, 200, T) for j in (1, 3, 10, 250) for R in (1, 2, 4)]
    for t_from, j, R in cases:
        walk = d.resample_walk(t_from, j, R)
        anchors = [a for a in range(j, t_from + 1, j) if a + j <= t_from]
        assert len(walk) == t_from + len(anchors) * (R - 1) * j, (t_from, j, R)
        assert walk[0][0] == t_from - 1 and walk[-1] == (0, 0)
        for (t, up), (t_next, _) in zip(walk, walk[1:]):
            assert t_next == t - 1 + up and up in (0, j)
        assert all(0 <= t < t_from for t, _ in walk)
        for a in anchors:                                   # every anchor is jumped from R - 1 times, nothing else is
            assert sum(1 for t, up in walk if up and t == a) == R - 1
        assert sum(1 for _, up in walk if up) == len(anchors) * (R - 1)
        if R == 1:
            assert walk == [(t, 0) for t in range(t_from - 1, -1, -1)]
    assert d.resample_walk(np.int64(5), np.int32(2), np.int64(2)) == WALKS[(5, 2, 2)]


def test_walk_refusals():
    d = _diffusion()
    T = d._diffusion_steps
    bad = [(5, 0, 2), (5, -1, 2), (5, 2, 0), (5, 2, -3),                               # below 1
           (5.0, 2, 2), (5, 2.0, 2), (5, 2, 2.0), ("5", 2, 2), (5, None, 2),           # not integers
           (True, 2, 2), (5, True, 2), (5, 2, True),                                   # bools
           (0, 2, 2), (-1, 2, 2), (T + 1, 2, 2),                                       # t_from outside 1 ... T
           (T, 10, 17), (T, 1, 17)]                                                    # more than 16*T rows
    for args in bad:
        with pytest.raises(ValueError):
            d.resample_walk(*args)
            pytest.fail(f"{args} was accepted")
    assert len(d.resample_walk(T, 10, 16)) == T + 99 * 15 * 10 <= 16 * T               # the longest R at j = 10 that fits
    with pytest.raises(ValueError):
        d.resample_tables(T, 10, 17)


# ---- the tables ----------------------------------------------------------------------------------------------------------------
def test_tables_without_resampling_are_the_plain_tables():
    d = _diffusion()
    for t_from, j, temp in ((1, 1, 1.0), (7, 2, 0.7), (200, 10, 1.0), (3, 5, 0.5)):
        table, ms, jump = d.resample_tables(t_from, j, 1, temp)
        for a in (table, ms, jump):
            assert a.dtype == np.float32
        assert table.tobytes() == d.ddpm_table(t_from, temp).tobytes()
        assert ms.tobytes() == d.known_levels(t_from).tobytes()
        assert jump.tobytes() == np.tile(np.float32([1.0, 0.0]), (t_from, 1)).tobytes()
    table, ms, jump = d.resample_tables(3, 5, 4)            # no anchor
    assert table.tobytes() == d.ddpm_table(3).tobytes() and ms.tobytes() == d.known_levels(3).tobytes()


def test_tables_follow_the_walk():
    d = _diffusion()
    T = d._diffusion_steps
    ab = d._h_alpha_bars
    worst = 0.0
    for t_from, j, R, temp in ((5, 2, 2, 1.0), (4, 2, 3, 0.9), (3, 1, 2, 1.0), (200, 10, 2, 1.0), (T, 10, 2, 1.0), (T, 250, 3, 1.0),
                               (T, 1, 2, 1.0)):
        walk = d.resample_walk(t_from, j, R)
        table, ms, jump = d.resample_tables(t_from, j, R, temp)
        assert table.shape == (len(walk), 8) and ms.shape == jump.shape == (len(walk), 2)
        plain, levels = d.ddpm_table(T, temp), d.known_levels(T)
        for i, (t, up) in enumerate(walk):
            assert table[i].tobytes() == plain[T - 1 - t].tobytes(), (t_from, j, R, i)
            if up == 0:
                assert tuple(jump[i]) == (1.0, 0.0)
                assert ms[i].tobytes() == levels[T - 1 - t].tobytes()
            else:
                assert t >= 1
                ratio = ab[t - 1 + up] / ab[t - 1]          # float32 0-d tensor arithmetic, as known_levels forms its scalars
                assert jump[i, 0] == np.float32(float(torch.sqrt(ratio)))
                assert jump[i, 1] == np.float32(float(torch.sqrt(1.0 - ratio))) and jump[i, 1] != 0.0
                level = ab[t - 1 + up]
                assert ms[i, 0] == np.float32(float(torch.sqrt(level))) and ms[i, 1] == np.float32(float(torch.sqrt(1.0 - level)))
                if t + up < T:                              # the level of an ordinary row: known_levels' row of the step at t + up
                    assert ms[i].tobytes() == levels[T - 1 - (t + up)].tobytes()
                unit = abs(float(jump[i, 0]) ** 2 + float(jump[i, 1]) ** 2 - 1.0)       # in float64
                worst = max(worst, unit)
    print(f"max |mf^2 + sf^2 - 1| = {worst:.3e}")
    assert worst <= float(np.spacing(np.float32(1.0)))


# ---- the exact toy: what the jumps are for ---------------------------------------------------------------------------------------
# An independent float64 restatement of RePaint's Algorithm 1 (Lugmayr et al. 2022) on a zero-mean two-coordinate Gaussian with
# unit variances and correlation rho, where the noise prediction is known in closed form: x_t ~ N(0, C_t) with
# C_t = ab_t*Sigma + (1 - ab_t)*I and eps(x_t, t) = sqrt(1 - ab_t) * C_t^-1 x_t.  Every operation of the algorithm is affine in
# the state with independent Gaussian noise, so the state's mean and covariance are propagated exactly -- no sampling.
# Coordinate 0 is kept (value KEPT), coordinate 1 is free (the input had FREE there).  Only the order of the rows comes from the
# project, resample_walk, and the beta schedule from the diffusion object.
KEPT, FREE = 1.5, -1.0


def _toy(betas, walk, t_from, rho):
    """mean and variance of the free coordinate after the walk's rows"""
    betas = np.asarray(betas, np.float64)
    alphas = 1.0 - betas
    ab = np.cumprod(alphas)
    sigma = np.array([[1.0, rho], [rho, 1.0]])
    eye = np.eye(2)

    def eps_matrix(t):
        return np.sqrt(1.0 - ab[t]) * np.linalg.inv(ab[t] * sigma + (1.0 - ab[t]) * eye)
    # the start: the forward process of the input (KEPT, FREE) at the level the first step takes its state to have, t_from - 1
    lv = ab[t_from - 1]
    mu = np.sqrt(lv) * np.array([KEPT, FREE])
    cov = (1.0 - lv) * eye
    for t, up in walk:
        if t == 0:                                          # the last step returns the mean: x0 = (x - sqrt(1 - ab_0) eps)/sqrt(ab_0)
            a, noise = (eye - np.sqrt(1.0 - ab[0]) * eps_matrix(0)) / np.sqrt(ab[0]), 0.0
        else:                                               # x_{t-1} = (x - beta_t/sqrt(1 - ab_t) eps)/sqrt(alpha_t) + sqrt(beta_t) z
            a, noise = (eye - betas[t] / np.sqrt(1.0 - ab[t]) * eps_matrix(t)) / np.sqrt(alphas[t]), betas[t]
        mu, cov = a @ mu, a @ cov @ a.T + noise * eye
        if up:                                              # lines 9-10, the j transitions composed: ab[t-1+up] / ab[t-1]
            r = ab[t - 1 + up] / ab[t - 1]
            mu[1], cov[1, 1] = np.sqrt(r) * mu[1], r * cov[1, 1] + (1.0 - r)
        # line 5 and 8: the kept coordinate is a fresh forward draw of its clean value at the state's level, or the value itself
        lv = 1.0 if t == 0 else ab[t - 1 + up]
        mu[0] = np.sqrt(lv) * KEPT
        cov[0, 0], cov[0, 1], cov[1, 0] = 1.0 - lv, 0.0, 0.0
    return float(mu[1]), float(cov[1, 1])


def test_toy_resampling_moves_the_free_coordinate_to_its_conditional_mean():
    d = _diffusion()
    T = d._diffusion_steps
    betas = d._h_betas.numpy().astype(np.float64)
    assert betas.shape == (T,)
    print("time_start rho  R  rows   mean    error  ratio  variance (conditional variance)")
    for t_from in (200, T):
        for rho in (0.5, 0.9):
            target, errors = rho * KEPT, []
            for R in (1, 2, 4, 8):
                walk = d.resample_walk(t_from, 10, R)
                mean, var = _toy(betas, walk, t_from, rho)
                errors.append(abs(mean - target))
                print(f"{t_from:10d} {rho:.1f} {R:2d} {len(walk):5d} {mean:7.3f} {errors[-1]:8.4f} {errors[-1] / errors[0]:6.3f} "
                      f"{var:8.4f} ({1.0 - rho * rho:.4f})")
            assert all(b < a for a, b in zip(errors, errors[1:])), (t_from, rho, errors)
            assert errors[-1] <= 0.25 * errors[0], (t_from, rho, errors)
    # jump length 1 tells the same story
    for rho in (0.5, 0.9):
        e1 = abs(_toy(betas, d.resample_walk(200, 1, 1), 200, rho)[0] - rho * KEPT)
        e8 = abs(_toy(betas, d.resample_walk(200, 1, 8), 200, rho)[0] - rho * KEPT)
        print(f"jump length 1, time_start 200, rho {rho}: ratio {e8 / e1:.3f}")
        assert e8 <= 0.25 * e1


# ---- the entry points --------------------------------------------------------------------------------------------------------------
def test_symbols_declared_bound_exported_and_documented():
    declared_bound_and_exported(NEW)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in doc, f"{name} is not named in INTEGRATION.md"
    from lion_amd import chain
    assert chain.RESAMPLE_STREAM == 3 and chain.KNOWN_STREAM == 2
    assert "4.6.11" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_entry_points_refuse_bad_arguments_before_launching():
    from lion_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    a = (ctypes.addressof(buf) + 15) & ~15                  # 16-byte aligned, never dereferenced: every call returns first

    def flat(mode=1, x=a, eps=a, B=2, n=8, cur=a, first=a, keys=a, sid=0, x0=a, keep=a, ms=a, ksid=2, jump=a, rsid=3, out=a,
             z=None):
        return lib.lion_chain_update_noise_keyed_known_resample(mode, x, eps, B, n, cur, first, keys, sid, x0, keep, ms, ksid,
                                                                jump, rsid, out, z, None)

    def cm(mode=1, x=a, eps=a, B=2, n=2, cur=a, first=a, keys=a, sid=0, x0=a, keep=a, ms=a, ksid=2, jump=a, rsid=3, out=a,
           z=None):
        return lib.lion_chain_update_noise_cm_keyed_known_resample(mode, x, eps, B, n, cur, first, keys, sid, x0, keep, ms, ksid,
                                                                   jump, rsid, out, z, None)

    for f in (flat, cm):
        for name in ("x", "eps", "cur", "keys", "out", "x0", "keep", "ms", "jump"):         # first_row may be NULL
            assert f(**{name: None}) == EINVAL, (f.__name__, name)
        for mode in (-1, 2):
            assert f(mode=mode) == EINVAL
        for sid in (0, 2, 7):                                                   # what the "_known" pair refuses
            assert f(sid=sid, ksid=sid, rsid=sid + 1) == EINVAL
        assert f(sid=0, ksid=2, rsid=0) == EINVAL and f(sid=0, ksid=2, rsid=2) == EINVAL    # the jumps' stream is its own
        assert f(sid=5, ksid=1, rsid=5) == EINVAL and f(sid=5, ksid=1, rsid=1) == EINVAL
        assert f(x=a + 4) == EINVAL and f(out=a + 8) == EINVAL and f(z=a + 4) == EINVAL and f(x0=a + 4) == EINVAL
        for B in (0, -1, 65536):
            assert f(B=B) == EINVAL, (f.__name__, B)
        for n in (0, -4):
            assert f(n=n) == EINVAL, (f.__name__, n)
    assert flat(eps=a + 4) == EINVAL
    for n in (1, 2, 3, 5, 6, 1022):
        assert flat(n=n) == EINVAL, n


# ---- host refusals, on CPU tensors: ValueError before the "no CPU path" error ------------------------------------------------------
class _Vae:
    def latent_shape(self):
        return [[128, 1, 1], [8192, 1, 1]]


def test_sampler_refusals_come_before_any_launch():
    d = _diffusion()
    T = d._diffusion_steps
    model, B, shape = torch.nn.Identity(), 3, [128, 1, 1]
    x = torch.zeros([B] + shape)
    keep = torch.zeros(B, 32, dtype=torch.bool)
    t = torch.tensor
    run = lambda start=30, **kw: d.run_denoising_diffusion_from_t(model, B, shape, start, x, **kw)
    bad = [
        lambda: run(resample=2), lambda: run(resample=(2, 2)), lambda: run(resample=1),             # resample without known
        lambda: run(t([30, 0, 20]), known=(x, keep), resample=2),                                   # per-sample starts
        lambda: run(np.array([30, 30, 30]), known=(x, keep), resample=(2, 2)),
        lambda: run(t([30, 0, 20]), known=(x, keep), resample=1),
        lambda: run(known=(x, keep), resample=2, given_noise=(x, [x] * 31)),                        # given_noise
        lambda: run(known=(x, keep), resample=0), lambda: run(known=(x, keep), resample=-1),        # values
        lambda: run(known=(x, keep), resample=True), lambda: run(known=(x, keep), resample=2.0),
        lambda: run(known=(x, keep), resample=(0, 2)), lambda: run(known=(x, keep), resample=(2, 0)),
        lambda: run(known=(x, keep), resample=(2, True)), lambda: run(known=(x, keep), resample=(2.0, 2)),
        lambda: run(known=(x, keep), resample=(2,)), lambda: run(known=(x, keep), resample=(2, 2, 2)),
        lambda: run(known=(x, keep), resample="4"), lambda: run(known=(x, keep), resample=t([2, 2])),
        lambda: run(T, known=(x, keep), resample=17), lambda: run(T, known=(x, keep), resample=(1, 17)),   # more than 16*T rows
        lambda: run(known=(x, keep.float()), resample=2),                                           # what known refuses
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {i} was accepted")
    good = [
        lambda: run(known=(x, keep), resample=2), lambda: run(known=(x, keep), resample=(2, 2), seeds=[1, 2, 3]),
        lambda: run(known=(x, keep), resample=[5, 3], seed=5), lambda: run(known=(x, keep), resample=1),
        lambda: run(known=(x, keep), resample=(7, 1)), lambda: run(known=(x, keep), resample=np.int64(2), graph=False),
        lambda: run(T, known=(x, keep), resample=16),
    ]
    for f in good:
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
    out, states = run(0, known=(x, keep), resample=2)       # nothing to do: the input comes back untouched, with no launch
    assert out is x and states == []


def test_diffuse_denoise_refusals_come_before_any_launch():
    from lion_amd.editing import diffuse_denoise
    d, vae = _diffusion(), _Vae()
    dae = [torch.nn.Identity(), torch.nn.Identity()]
    B, N = 3, 2048
    x = torch.zeros(B, N, 3)
    ok = torch.zeros(B, N, dtype=torch.bool)
    run = lambda start=(0, 30), **kw: diffuse_denoise(vae, dae, d, x, start, seeds=[1, 2, 3], **kw)
    with pytest.raises(ValueError, match="keep"):
        run(resample=2)
    for steps in (2, 5):
        with pytest.raises(ValueError, match="solver_steps"):
            run(keep=ok, resample=2, solver_steps=steps)
    for start in ((0, [30, 0, 20]), torch.tensor([30, 0, 20]), ([1, 1, 1], 30)):
        with pytest.raises(ValueError, match="per-sample"):
            run(start, keep=ok, resample=2)
    for v in (0, -2, True, 2.0, (2,), (0, 2), (2, 0), "2"):
        with pytest.raises(ValueError, match="resample"):
            run(keep=ok, resample=v)
    with pytest.raises(ValueError, match="rows"):
        run((0, d._diffusion_steps - 1), keep=ok, resample=(1, 18))
    for v in (2, (2, 2), 1, (5, 1)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            run(keep=ok, resample=v)


def test_resample_chain_construction_refusals():
    from lion_amd import chain
    ident = torch.nn.Identity()
    for kw in (dict(), dict(keyed=True), dict(from_rows=True), dict(keyed=True, from_rows=True)):   # known=False
        with pytest.raises(ValueError):
            chain.GraphedChain(ident, 2, [128, 1, 1], None, None, "cpu", chain.DDPM, 8, resample=True, **kw)
    for kw in (dict(), dict(keyed=True), dict(from_rows=True)):                                     # what known refuses
        with pytest.raises(ValueError):
            chain.GraphedChain(ident, 2, [128, 1, 1], None, None, "cpu", chain.DDPM, 8, known=True, resample=True, **kw)
    cache = chain.ChainCache()
    with pytest.raises(ValueError, match="resample"):
        cache.get(ident, 2, [128, 1, 1], None, None, "cpu", chain.DDPM, 8, keyed=True, from_rows=True, resample=True)
    assert not cache._entries


# ---- what the host half hands to the chain -----------------------------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """a host tensor that says it lives on the device: lets the host half of a graphed call run up to its _replay"""
    is_cuda = True


def test_host_half_hands_the_walks_tables_zero_first_rows_and_the_quad_mask(monkeypatch):
    from lion_amd import chain
    d = _diffusion()
    T = d._diffusion_steps
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
    run = lambda start, **kw: d.run_denoising_diffusion_from_t(model, B, shape, start, x, seeds=[11, 12, 13, 14], known=(x0, keep),
                                                               keep_trajectory=False, **kw)
    for start, resample, pair in ((30, 2, (10, 2)), (5, (2, 2), (2, 2)), (T, [10, 16], (10, 16))):
        calls.clear()
        run(start, temp=0.75, resample=resample)
        assert len(calls) == 1
        c = calls[0]
        table, ms, jump = d.resample_tables(start, *pair, temp=0.75)
        assert c["first_row"] == [0, 0, 0, 0] and c["mode"] == chain.DDPM and c["keys"] == [11, 12, 13, 14] and c["seed"] is None
        assert np.array_equal(c["table"], table) and c["capacity"] == max(T, len(table))
        kx0, quads, kms, kjump = c["known"]
        assert torch.equal(kx0, x0) and np.array_equal(kms, ms) and np.array_equal(kjump, jump) and (kjump[:, 1] != 0).any()
        assert quads.shape == (B, 32) and torch.equal(quads, keep.repeat_interleave(2, dim=1))
    # n_resample = 1 hands the chain what the call without resample hands it: the triple, the plain tables, no capacity
    calls.clear()
    run(30)
    run(30, resample=1)
    run(30, resample=(3, 1))
    assert len(calls) == 3
    for c in calls:
        assert len(c["known"]) == 3 and "capacity" not in c and sorted(c) == sorted(calls[0])
        assert np.array_equal(c["table"], d.ddpm_table(30)) and np.array_equal(c["known"][2], d.known_levels(30))
