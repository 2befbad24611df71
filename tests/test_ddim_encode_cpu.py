"""CPU suite of the deterministic few-step encoder (DiffusionDiscretized.encode_table / run_ddim_forward, lion_ddim_encode_update,
lion_chain_update_encode[_cm]): the C ABI agrees across header, ctypes table and library and refuses bad arguments on the host;
the schedule table against a float64 restatement written here; the encoder as the algebraic inverse of the order-1 decoder on a
nonlinear toy; and the round-trip error ladder over the refinement count on the Gaussian toy (float64 numpy, the kernel's
expression)."""
import ctypes
import os

import numpy as np
import pytest

import abi_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lion_ddim_encode_update", "lion_chain_update_encode", "lion_chain_update_encode_cm")
SCHEDULES = ("linear", "cust")


def _diffusion(sched="linear", T=1000):
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    cfg = released_prior_cfg()
    cfg.ddpm.sched_mode, cfg.ddpm.beta_1, cfg.ddpm.beta_T, cfg.ddpm.num_steps = sched, 1e-4, 0.02, T
    return DiffusionDiscretized(None, None, cfg, device="cpu")


def test_three_symbols_are_declared_bound_and_exported():
    from lion_amd import _lib, chain, diffusion_ops
    abi_check.declared_bound_and_exported(NEW)
    assert "ddim_encode_update" in diffusion_ops.__all__
    assert chain.ENCODE == 4 and {chain.DDIM, chain.DDPM, chain.DPMPP, chain.SDE_DPMPP} == {0, 1, 2, 3}


def test_bad_arguments_are_refused_on_the_host():
    """before any launch (no GPU here: a launch would be a positive HIP error)"""
    from lion_amd import _lib
    l = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, 8 floats behind it
    co, c0 = (0.62, 0.78, 1.0), (0.62, 0.78, 0.0)
    assert l.lion_ddim_encode_update(None, p, 8, *co, p, p, None) == -1       # base
    assert l.lion_ddim_encode_update(p, None, 8, *co, p, p, None) == -1       # eps
    assert l.lion_ddim_encode_update(p, p, 8, *co, None, p, None) == -1       # out
    assert l.lion_ddim_encode_update(p, p, 8, *co, p, None, None) == -1       # a committing row writes base_out
    assert l.lion_ddim_encode_update(p, p, 0, *co, p, p, None) == -1          # numel
    assert l.lion_ddim_encode_update(p, p, 0, *c0, p, None, None) == -1       # base_out may be NULL without commit -- numel may not
    assert l.lion_ddim_encode_update(p + 4, p, 2, *co, p, p, None) == -1      # 16-byte accesses: misaligned base
    assert l.lion_ddim_encode_update(p, p + 4, 2, *co, p, p, None) == -1      # ... eps
    assert l.lion_ddim_encode_update(p, p, 2, *co, p + 8, p, None) == -1      # ... out
    assert l.lion_ddim_encode_update(p, p, 2, *co, p, p + 4, None) == -1      # ... base_out
    assert l.lion_chain_update_encode(None, p, 8, p, p, p, None) == -1
    assert l.lion_chain_update_encode(p, None, 8, p, p, p, None) == -1
    assert l.lion_chain_update_encode(p, p, 8, None, p, p, None) == -1        # cur
    assert l.lion_chain_update_encode(p, p, 8, p, None, p, None) == -1
    assert l.lion_chain_update_encode(p, p, 8, p, p, None, None) == -1        # commit is on the device: base_out is required
    assert l.lion_chain_update_encode(p, p, 0, p, p, p, None) == -1
    assert l.lion_chain_update_encode(p, p + 4, 2, p, p, p, None) == -1
    assert l.lion_chain_update_encode_cm(None, p, 1, 2, p, p, p, None) == -1
    assert l.lion_chain_update_encode_cm(p, None, 1, 2, p, p, p, None) == -1
    assert l.lion_chain_update_encode_cm(p, p, 1, 2, None, p, p, None) == -1
    assert l.lion_chain_update_encode_cm(p, p, 1, 2, p, None, p, None) == -1
    assert l.lion_chain_update_encode_cm(p, p, 1, 2, p, p, None, None) == -1
    assert l.lion_chain_update_encode_cm(p, p, 0, 2, p, p, p, None) == -1
    assert l.lion_chain_update_encode_cm(p, p, 1, 0, p, p, p, None) == -1
    assert l.lion_chain_update_encode_cm(p + 4, p, 1, 2, p, p, p, None) == -1
    assert l.lion_chain_update_encode_cm(p, p, 1, 2, p, p, p + 8, None) == -1


def test_encoder_has_no_cpu_path():
    import torch
    from lion_amd import diffusion_ops
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffusion_ops.ddim_encode_update(x, x, 1.0, 0.0, True)
    d = _diffusion()
    model = torch.nn.Identity()
    for graph in (True, False):
        with pytest.raises(RuntimeError, match="no CPU path"):
            d.run_ddim_forward(model, torch.zeros(2, 128, 1, 1), 5, "logsnr", graph=graph)


# ---- encode_table ------------------------------------------------------------------------------------------------------------
def _table64(ab32, taus, refine):
    """independent float64 restatement, leg by leg from the clean latent (alpha = 1, sigma = 0) upwards"""
    ab = np.asarray(ab32, np.float32).astype(np.float64)
    up = np.asarray(taus)[::-1]                                   # ascending: the targets of the legs
    al = np.concatenate([[1.0], np.sqrt(ab[up])])                 # al[k]: the low end of leg k, al[k + 1] its target
    sg = np.concatenate([[0.0], np.sqrt(1.0 - ab[up])])
    s = al[1:] / al[:-1]
    c = sg[1:] - sg[:-1] * s
    t_pred = np.concatenate([[1], up[:-1] + 1])
    rows = np.zeros((len(up), 1 + refine, 8))
    rows[:, :, 0] = (up + 1)[:, None]
    rows[:, 0, 0] = t_pred
    rows[:, :, 1] = s[:, None]
    rows[:, :, 2] = c[:, None]
    rows[:, -1, 3] = 1.0
    return rows.reshape(-1, 8), al


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("refine", [0, 2])
def test_encode_table_equals_a_float64_restatement(sched, refine):
    d = _diffusion(sched)
    for S, skip in ((1, "logsnr"), (2, "logsnr"), (3, "uniform"), (20, "logsnr"), (20, "uniform"), (50, "quad")):
        taus = d.solver_schedule(S, skip)
        got = d.encode_table(taus, refine)
        want, al = _table64(d._h_alpha_bars.numpy(), taus, refine)
        L, R = len(taus), 1 + refine
        assert got.dtype == np.float32 and got.shape == (L * R, 8)
        assert np.array_equal(got, want.astype(np.float32)), (S, skip)
        g64 = d.encode_table(taus, refine, dtype=np.float64)
        assert np.array_equal(g64, want)
        assert np.all(got[:, 4:] == 0)
        legs = g64.reshape(L, R, 8)
        # commit on the last row of every leg, nowhere else
        assert np.all(legs[:, -1, 3] == 1) and np.all(legs[:, :-1, 3] == 0)
        # t_model: the predictor at the low index + 1 (1 on the first leg), every corrector at the target index + 1
        up = np.asarray(taus)[::-1]
        assert legs[0, 0, 0] == 1 and np.array_equal(legs[1:, 0, 0], up[:-1] + 1)
        assert np.array_equal(legs[:, 1:, 0], np.repeat((up + 1)[:, None], refine, axis=1))
        # one (s, c) per leg, and s carries alpha from the low end to the target
        assert np.all(legs[:, :, 1] == legs[:, :1, 1]) and np.all(legs[:, :, 2] == legs[:, :1, 2])
        assert np.all(np.abs(legs[:, 0, 1] * al[:-1] - al[1:]) <= 1e-12 * al[1:])
        assert np.all(legs[:, 0, 2] > 0) and np.all(legs[:, 0, 1] > 0)
    assert np.array_equal(d.encode_table(taus), d.encode_table(taus, 0))              # refine = 0 is the default
    with pytest.raises(ValueError):
        d.encode_table(taus, -1)


# ---- the encoder is the inverse of the order-1 decoder ---------------------------------------------------------------------------
def encode(d, taus, refine, x, eps):
    """the kernel's expression over encode_table's rows in float64: the model reads the current iterate"""
    base = x = np.asarray(x, np.float64)
    for row in d.encode_table(taus, refine, dtype=np.float64):
        x = row[1] * base + row[2] * eps(x, int(row[0]) - 1)
        if row[3] != 0:
            base = x
    return x


def decode(d, taus, x, eps):
    """the multistep kernel's expressions over dpm_solver_table(order=1) in float64"""
    for row, t in zip(d.dpm_solver_table(taus, 1, dtype=np.float64), taus):
        x0 = row[1] * (x - row[2] * eps(x, t))
        x = row[3] * x + row[4] * (row[5] * x0)
    return x


@pytest.mark.parametrize("sched", SCHEDULES)
def test_refined_encoder_inverts_the_decoder_on_a_nonlinear_toy(sched):
    """eps(x, t) = sigma_t*tanh(x)/2 has Lipschitz constant sigma_t/2 <= 1/2 and 0 < c <= sigma_t <= 1, so every corrector
    contracts the distance to the implicit equation's solution by at least 1/2: 60 of them leave 2^-60 of the predictor's error,
    below float64's rounding, and the decoder then retraces every leg: the input comes back to 1e-10 relative."""
    d = _diffusion(sched)
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    sg = np.sqrt(1.0 - ab)
    eps = lambda x, t: sg[t] * np.tanh(x) / 2.0
    x = np.random.default_rng(7).standard_normal(64) * 1.5
    for S, skip in ((5, "logsnr"), (20, "logsnr"), (20, "uniform")):
        taus = d.solver_schedule(S, skip)
        back = decode(d, taus, encode(d, taus, 60, x, eps), eps)
        err = np.linalg.norm(back - x) / np.linalg.norm(x)
        print(f"{sched} S={S} {skip}: nonlinear toy, refine=60 round trip {err:.3e}")
        assert err <= 1e-10, (S, skip, err)
        # and without refinement it is not the inverse
        assert np.linalg.norm(decode(d, taus, encode(d, taus, 0, x, eps), eps) - x) / np.linalg.norm(x) > 1e-4


@pytest.mark.parametrize("sched", SCHEDULES)
def test_refine_zero_is_textbook_ddim_inversion(sched):
    """x_t = sqrt(ab_t/ab_n)*x_n + (sqrt(1 - ab_t) - sqrt(1 - ab_n)*sqrt(ab_t/ab_n))*eps(x_n, n), the DDIM step read from n up to
    t with eps taken where the state is known; the first leg starts from the clean latent (ab = 1) with the model at index 0"""
    d = _diffusion(sched)
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    sg = np.sqrt(1.0 - ab)
    eps = lambda x, t: sg[t] * np.tanh(x) / 2.0
    x0 = np.random.default_rng(8).standard_normal(64)
    for S, skip in ((5, "logsnr"), (20, "logsnr"), (20, "uniform")):
        taus = d.solver_schedule(S, skip)
        x, ab_n, n = x0.copy(), 1.0, 0
        for t in reversed(taus):
            r = np.sqrt(ab[t] / ab_n)
            x = r * x + (np.sqrt(1.0 - ab[t]) - np.sqrt(1.0 - ab_n) * r) * eps(x, n)
            ab_n, n = ab[t], t
        got = encode(d, taus, 0, x0, eps)
        assert np.linalg.norm(got - x) <= 1e-12 * np.linalg.norm(x), (S, skip)


# ---- the round-trip ladder on the Gaussian toy -----------------------------------------------------------------------------------
# Data ~ N(0, s^2): the exact denoiser is eps(x, t) = sigma_t*x / v_t, v_t = ab_t*s^2 + 1 - ab_t (tests/test_dpm_solver_cpu.py).
def round_trip(d, S, K, s):
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    g = np.sqrt(1.0 - ab) / (ab * s * s + 1.0 - ab)
    eps = lambda x, t: x * g[t]
    taus = d.solver_schedule(S, "logsnr")
    return abs(float(decode(d, taus, encode(d, taus, K, 1.0, eps), eps)) - 1.0)


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("s", [0.25, 0.5, 1.0, 2.0])
def test_each_refinement_halves_the_round_trip_error(s, sched):
    """S = 20, 'logsnr': each of the first three refinements at least halves the relative round-trip error (measured ratios
    2.25 - 4.0, DESIGN.md 4.6.5 lists the ladder), and at equal encoder cost S = 20 with K = 1 beats S = 40 with K = 0."""
    d = _diffusion(sched)
    e = [round_trip(d, 20, K, s) for K in range(5)]
    e40 = [round_trip(d, 40, K, s) for K in range(3)]
    print(f"s={s} {sched}: S=20 " + " ".join(f"K={K} {v:.2e}" for K, v in enumerate(e))
          + "  ratios " + " ".join(f"{a / b:.2f}" for a, b in zip(e, e[1:]))
          + "  |  S=40 " + " ".join(f"K={K} {v:.2e}" for K, v in enumerate(e40)))
    for K in range(3):
        assert e[K + 1] <= e[K] / 2.0, (K, e)
    assert e[1] < e40[0], (e[1], e40[0])
