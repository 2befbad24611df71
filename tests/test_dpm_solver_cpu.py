"""CPU suite of the DPM-Solver++(2M) sampler (DiffusionDiscretized.solver_schedule / dpm_solver_table / run_dpm_solver,
lion_dpmpp_update, lion_chain_update_multistep[_cm]): the C ABI agrees across header, ctypes table and library and refuses bad
arguments on the host; the schedule and the coefficient table against restatements written here; and the solver's integration
error on an ODE with a closed-form solution against DDIM's (float64 numpy, the kernel's four expressions)."""
import ctypes
import os

import numpy as np
import pytest

import abi_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lion_dpmpp_update", "lion_chain_update_multistep", "lion_chain_update_multistep_cm")
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
    assert "dpmpp_update" in diffusion_ops.__all__ and chain.DPMPP == 2 and {chain.DDIM, chain.DDPM} == {0, 1}
    # bad arguments are refused on the host, before any launch (no GPU here: a launch would be a positive HIP error)
    l = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, 8 floats behind it
    co = (156.0, 0.99998, 0.97, 4.1e-4, 1.5, -0.5)
    c1 = co[:4] + (1.0, 0.0)
    assert l.lion_dpmpp_update(None, p, p, 8, *co, p, p, None) == -1        # x
    assert l.lion_dpmpp_update(p, None, p, 8, *co, p, p, None) == -1        # eps
    assert l.lion_dpmpp_update(p, p, p, 8, *co, None, p, None) == -1        # out
    assert l.lion_dpmpp_update(p, p, p, 8, *co, p, None, None) == -1        # hist_out
    assert l.lion_dpmpp_update(p, p, None, 8, *co, p, p, None) == -1        # a5 != 0 reads hist
    assert l.lion_dpmpp_update(p, p, p, 0, *co, p, p, None) == -1           # numel
    assert l.lion_dpmpp_update(p, p, None, 0, *c1, p, p, None) == -1        # hist may be NULL with a5 == 0 -- numel still may not
    assert l.lion_dpmpp_update(p + 4, p, p, 2, *co, p, p, None) == -1       # 16-byte accesses: misaligned x
    assert l.lion_dpmpp_update(p, p, p, 2, *co, p, p + 8, None) == -1       # ... and hist_out
    assert l.lion_chain_update_multistep(None, p, p, 8, p, p, p, None) == -1
    assert l.lion_chain_update_multistep(p, p, None, 8, p, p, p, None) == -1   # coefficients on the device: hist is required
    assert l.lion_chain_update_multistep(p, p, p, 8, None, p, p, None) == -1   # cur
    assert l.lion_chain_update_multistep(p, p, p, 0, p, p, p, None) == -1
    assert l.lion_chain_update_multistep(p, p + 4, p, 2, p, p, p, None) == -1
    assert l.lion_chain_update_multistep_cm(None, p, p, 1, 2, p, p, p, None) == -1
    assert l.lion_chain_update_multistep_cm(p, None, p, 1, 2, p, p, p, None) == -1
    assert l.lion_chain_update_multistep_cm(p, p, None, 1, 2, p, p, p, None) == -1
    assert l.lion_chain_update_multistep_cm(p, p, p, 1, 2, None, p, p, None) == -1
    assert l.lion_chain_update_multistep_cm(p, p, p, 1, 2, p, None, p, None) == -1
    assert l.lion_chain_update_multistep_cm(p, p, p, 0, 2, p, p, p, None) == -1
    assert l.lion_chain_update_multistep_cm(p, p, p, 1, 0, p, p, p, None) == -1
    assert l.lion_chain_update_multistep_cm(p, p, p + 4, 1, 2, p, p, p, None) == -1


def test_dpmpp_update_has_no_cpu_path():
    import torch
    from lion_amd import diffusion_ops
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffusion_ops.dpmpp_update(x, x, None, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0)


# ---- solver_schedule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("skip_type", ["logsnr", "uniform", "quad"])
def test_solver_schedule_is_descending_distinct_and_spans_the_chain(sched, skip_type):
    d = _diffusion(sched)
    T = d._diffusion_steps
    for S in (1, 2, 5, 20, 50):
        tau = d.solver_schedule(S, skip_type)
        assert all(isinstance(t, int) for t in tau)
        assert all(a > b for a, b in zip(tau, tau[1:])), (S, tau)       # strictly descending: distinct
        assert tau[-1] == 0 and 1 <= len(tau) <= S
        if S >= 2:
            assert tau[0] == T - 1
        else:
            assert tau == [0]
    if skip_type == "logsnr":
        assert len(d.solver_schedule(20, skip_type)) == 20


def test_logsnr_schedule_is_the_nearest_index_to_uniform_lambda():
    d = _diffusion("linear")
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    lam = 0.5 * (np.log(ab) - np.log1p(-ab))
    S = 20
    want = []
    for p in np.linspace(lam[-1], lam[0], S):
        i = int(np.abs(lam - p).argmin())
        if i not in want:
            want.append(i)
    assert d.solver_schedule(S) == want == d.solver_schedule(S, "logsnr")
    assert np.all(np.diff(lam[want]) > 0)                       # descending indices: ascending log-SNR


def test_index_spaced_schedules_are_ddim_schedule_without_duplicates():
    d = _diffusion("linear")
    T = d._diffusion_steps
    for S in (2, 5, 20, 50):
        for skip in ("uniform", "quad"):
            ref = sorted(set(d.ddim_schedule(T, S, skip)), reverse=True)
            got = d.solver_schedule(S, skip)
            assert got[1:] == ref[1:] and got[0] == T - 1 >= ref[0]      # only the top entry may move, up to T-1


def test_unknown_skip_type_is_a_value_error():
    d = _diffusion()
    with pytest.raises(ValueError):
        d.solver_schedule(10, "cosine")
    with pytest.raises(ValueError):
        d.solver_schedule(1, "cosine")


# ---- dpm_solver_table --------------------------------------------------------------------------------------------------------
def _table64(ab32, steps, order):
    """independent float64 restatement (vectorised) of the rows {t + 1, a0..a5, 0}"""
    ab = np.asarray(ab32, np.float32).astype(np.float64)
    st = np.asarray(steps)
    t, n = st[:-1], st[1:]
    al, sg = np.sqrt(ab), np.sqrt(1.0 - ab)
    lam = 0.5 * (np.log(ab) - np.log1p(-ab))
    h = lam[n] - lam[t]
    rows = np.zeros((len(st), 8))
    rows[:, 0] = st + 1
    rows[:, 1] = 1.0 / al[st]
    rows[:, 2] = sg[st]
    rows[:-1, 3] = sg[n] / sg[t]
    rows[:-1, 4] = -al[n] * np.expm1(-h)
    rows[:, 5] = 1.0
    if order == 2 and len(st) > 2:
        r = h[:-1] / h[1:]
        rows[1:-1, 5] = 1.0 + 0.5 / r
        rows[1:-1, 6] = -0.5 / r
    rows[-1, 3:7] = (0.0, 1.0, 1.0, 0.0)
    return rows


@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("order", [1, 2])
def test_dpm_solver_table_equals_a_float64_restatement(sched, order):
    d = _diffusion(sched)
    for S, skip in ((1, "logsnr"), (2, "logsnr"), (3, "uniform"), (10, "logsnr"), (20, "logsnr"), (20, "uniform"), (50, "quad")):
        steps = d.solver_schedule(S, skip)
        got = d.dpm_solver_table(steps, order)
        assert got.dtype == np.float32 and got.shape == (len(steps), 8)
        want = _table64(d._h_alpha_bars.numpy(), steps, order)
        assert np.array_equal(got, want.astype(np.float32)), (S, skip)
        assert np.array_equal(d.dpm_solver_table(steps, order, dtype=np.float64), want)
        assert np.all(got[:, 7] == 0) and got[-1, 0] == 1.0 and np.array_equal(got[-1, 3:7], [0, 1, 1, 0])
        assert np.array_equal(got[0, 5:7], [1, 0])
        if order == 2 and len(steps) > 2:
            assert np.all(got[1:-1, 6] < 0) and np.allclose(got[1:-1, 5] + got[1:-1, 6], 1.0, rtol=0, atol=1e-6)
        else:
            assert np.all(got[:, 5] == 1) and np.all(got[:, 6] == 0)
    assert np.array_equal(d.dpm_solver_table(steps), d.dpm_solver_table(steps, 2))    # order 2 is the default


@pytest.mark.parametrize("sched", SCHEDULES)
def test_order_one_is_ddim_with_kappa_zero(sched):
    """x <- a2*x + a3*a0*(x - a1*eps) = (a2 + a3*a0)*x - a3*a0*a1*eps is DDIM's x*sqrt(ab_n/ab_t) + (sqrt(1 - ab_n) -
    sqrt(1 - ab_t)*sqrt(ab_n/ab_t))*eps: both identities to 1e-12 relative, on the float64 values before the cast"""
    d = _diffusion(sched)
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    for S, skip in ((20, "logsnr"), (50, "logsnr"), (20, "uniform"), (1000, "uniform")):
        steps = np.asarray(d.solver_schedule(S, skip))
        tb = d.dpm_solver_table(steps, 1, dtype=np.float64)[:-1]
        t, n = steps[:-1], steps[1:]
        a0, a1, a2, a3 = tb[:, 1], tb[:, 2], tb[:, 3], tb[:, 4]
        s = np.sqrt(ab[n] / ab[t])
        c = np.sqrt(1 - ab[n]) - np.sqrt(1 - ab[t]) * s
        assert np.all(np.abs(a2 + a3 * a0 - s) <= 1e-12 * np.abs(s))
        assert np.all(np.abs(-a3 * a0 * a1 - c) <= 1e-12 * np.abs(c))


def test_order_three_is_a_value_error():
    d = _diffusion()
    for order in (0, 3, 2.5):
        with pytest.raises(ValueError):
            d.dpm_solver_table([999, 500, 0], order)


# ---- accuracy on an ODE with a closed-form solution ------------------------------------------------------------------------------
# Data ~ N(0, s^2): the marginal at index i is N(0, v_i), v_i = ab_i*s^2 + 1 - ab_i, the exact denoiser is
# eps(x, t) = sigma_t*x / v_t, and the probability-flow ODE keeps x / sqrt(v) constant.
def closed_form(ab, s):
    v = ab * s * s + 1.0 - ab
    x0 = np.sqrt(v[0] / v[-1])                                   # from x_{T-1} = 1 down to index 0
    return (x0 - np.sqrt(1 - ab[0]) * (np.sqrt(1 - ab[0]) * x0 / v[0])) / np.sqrt(ab[0])   # ... and its data prediction


def run_solver(table, steps, ab, s, dtype=np.float64):
    """the kernel's four expressions over the table's rows, in `dtype`"""
    f = dtype
    v = ab * s * s + 1.0 - ab
    g = (np.sqrt(1.0 - ab) / v).astype(f)
    x, hist = f(1.0), f(0.0)
    for row, t in zip(table.astype(f), steps):
        a0, a1, a2, a3, a4, a5 = row[1:7]
        eps = x * g[t]
        x0 = a0 * (x - a1 * eps)
        D = a4 * x0 if a5 == 0 else a4 * x0 + a5 * hist
        x, hist = a2 * x + a3 * D, x0
    return float(x)


def run_ddim(d, steps, ab, s):
    v = ab * s * s + 1.0 - ab
    x = 1.0
    for i, t in enumerate(steps):
        sc, c, sigma = d.ddim_coefficients(t, None if i == len(steps) - 1 else steps[i + 1], 0.0)
        assert sigma == 0.0
        x = x * sc + c * (np.sqrt(1.0 - ab[t]) * x / v[t])
    return x


@pytest.mark.parametrize("S", [10, 20])
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("s", [0.2, 0.5, 1.0])
def test_second_order_error_is_a_third_of_ddims(s, sched, S):
    """'logsnr' spacing, the same index list for both: relative error of DPM-Solver++(2M) <= 1/3 of DDIM's (kappa = 0).
    Measured: the ratio DDIM / 2M lies between 5.5 and 21 over these twelve cases (DESIGN.md 4.6.3 lists the pairs)."""
    d = _diffusion(sched)
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    steps = d.solver_schedule(S, "logsnr")
    exact = closed_form(ab, s)
    e2 = abs(run_solver(d.dpm_solver_table(steps, 2, dtype=np.float64), steps, ab, s) - exact) / abs(exact)
    e1 = abs(run_ddim(d, steps, ab, s) - exact) / abs(exact)
    print(f"s={s} {sched} S={S} (visited {len(steps)}): DDIM {e1:.3e}  2M {e2:.3e}  ratio {e1 / e2:.2f}")
    assert e2 <= e1 / 3.0, (e1, e2)
    # order 1 of the table IS that DDIM chain, up to the float32 rounding of ddim_coefficients: per step two coefficients of
    # at most four float32 roundings each (2^-24 relative, on terms of size <= 1) applied to |x|, |eps| of order 1
    # (x / sqrt(v) is constant and v falls from 1 to v_0: |x| <= 1), summed over the steps, relative to the exact value
    e1t = abs(run_solver(d.dpm_solver_table(steps, 1, dtype=np.float64), steps, ab, s) - exact) / abs(exact)
    assert abs(e1t - e1) <= len(steps) * 8 * 2.0 ** -24 / abs(exact)
