"""CPU suite of the stochastic few-step solver SDE-DPM-Solver++(2M) (dpm_solver_table(stochastic=True),
solver_schedule(t_start=...), lion_sde_dpmpp_update, lion_chain_update_multistep_noise[_cm]): the coefficient identities and the
tail schedule in float64, the C ABI's argument checks on the host, and the solver's error on a linear-Gaussian toy by exact
covariance propagation -- nothing is sampled, so nothing here has statistical noise."""
import ctypes
import os

import numpy as np
import pytest

import abi_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lion_sde_dpmpp_update", "lion_chain_update_multistep_noise", "lion_chain_update_multistep_noise_cm")
SCHEDULES = ("linear", "cust")
STARTS = (None, 400, 200, 100)          # None: the whole chain from T-1
SCALES = (0.2, 0.5, 1.0)


def _diffusion(sched="linear", T=1000):
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    cfg = released_prior_cfg()
    cfg.ddpm.sched_mode, cfg.ddpm.beta_1, cfg.ddpm.beta_T, cfg.ddpm.num_steps = sched, 1e-4, 0.02, T
    return DiffusionDiscretized(None, None, cfg, device="cpu")


def _index_lists(d):
    for S in (2, 10, 20):
        for skip in ("logsnr", "uniform", "quad"):
            for t_start in (None, 400, 100, 1):
                yield d.solver_schedule(S, skip, t_start)


# ---- coefficients --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDULES)
def test_order_one_is_ddim_with_kappa_one_and_the_variance_closes(sched):
    """x <- a2*x + a3*a0*(x - a1*eps) + a6*z against DDIM's x*s + c*eps + sigma*z at kappa = 1 (the expressions of
    ddim_coefficients in float64), and (a2*sigma_t)^2 + a6^2 = sigma_n^2: 1e-12 relative on the values before the cast"""
    d = _diffusion(sched)
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    for steps in _index_lists(d):
        steps = np.asarray(steps)
        for order in (1, 2):
            tb = d.dpm_solver_table(steps, order, dtype=np.float64, stochastic=True)
            assert np.array_equal(tb[-1, 3:8], [0, 1, 1, 0, 0])                  # the last row draws nothing
            tb = tb[:-1]
            t, n = steps[:-1], steps[1:]
            a0, a1, a2, a3, a6 = tb[:, 1], tb[:, 2], tb[:, 3], tb[:, 4], tb[:, 7]
            assert np.all(a6 > 0)
            var_n = 1.0 - ab[n]
            assert np.all(np.abs((a2 * np.sqrt(1.0 - ab[t])) ** 2 + a6 ** 2 - var_n) <= 1e-12 * var_n)
            if order == 1:
                s = np.sqrt(ab[n] / ab[t])
                sigma = np.sqrt((1 - ab[n]) / (1 - ab[t]) * (1 - ab[t] / ab[n]))
                c = np.sqrt(1 - ab[n] - sigma ** 2) - np.sqrt(1 - ab[t]) * s
                assert np.all(np.abs(a2 + a3 * a0 - s) <= 1e-12 * np.abs(s))
                assert np.all(np.abs(-a3 * a0 * a1 - c) <= 1e-12 * np.abs(c))
                assert np.all(np.abs(a6 - sigma) <= 1e-12 * sigma)
                assert np.all(tb[:, 5] == 1) and np.all(tb[:, 6] == 0)
    # ... and ddim_coefficients itself, float32 arithmetic: a handful of roundings of 2^-24 on terms of size <= 1
    steps = d.solver_schedule(10)
    tb = d.dpm_solver_table(steps, 1, dtype=np.float64, stochastic=True)
    for i in range(len(steps) - 1):
        s, c, sigma = d.ddim_coefficients(steps[i], steps[i + 1], 1.0)
        assert abs(tb[i, 3] + tb[i, 4] * tb[i, 1] - s) <= 1e-6 and abs(-tb[i, 4] * tb[i, 1] * tb[i, 2] - c) <= 1e-6
        assert abs(tb[i, 7] - sigma) <= 1e-6


@pytest.mark.parametrize("sched", SCHEDULES)
def test_stochastic_table_shares_every_other_column_and_defaults_do_not_move(sched):
    d = _diffusion(sched)
    for steps in _index_lists(d):
        for order in (1, 2):
            det = d.dpm_solver_table(steps, order)
            assert np.array_equal(det, d.dpm_solver_table(steps, order, stochastic=False))
            assert np.array_equal(det, d.dpm_solver_table(steps, order, np.float32, False)) and np.all(det[:, 7] == 0)
            sde = d.dpm_solver_table(steps, order, stochastic=True)
            assert sde.dtype == np.float32 and sde.shape == det.shape
            assert np.array_equal(sde[:, [0, 1, 2, 5, 6]], det[:, [0, 1, 2, 5, 6]])       # t, a0, a1, a4, a5
            assert np.array_equal(sde[-1], det[-1])
            if len(steps) > 1:
                assert np.all(sde[:-1, 3] < det[:-1, 3]) and np.all(sde[:-1, 4] > det[:-1, 4]) and np.all(sde[:-1, 7] > 0)
    for S in (1, 2, 10, 20):
        for skip in ("logsnr", "uniform", "quad"):
            assert d.solver_schedule(S, skip, None) == d.solver_schedule(S, skip) == d.solver_schedule(S, skip, t_start=None)


# ---- the tail schedule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("skip_type", ["logsnr", "uniform", "quad"])
def test_tail_schedule(sched, skip_type):
    d = _diffusion(sched)
    T = d._diffusion_steps
    for S in (2, 3, 8, 10, 20, 50):
        for t_start in (1, 2, 7, 100, 200, 400, 998, T - 1, np.int64(300)):
            tau = d.solver_schedule(S, skip_type, t_start)
            assert all(isinstance(t, int) for t in tau)
            assert all(a > b for a, b in zip(tau, tau[1:])), (S, t_start, tau)       # descending and distinct
            assert tau[0] == t_start and tau[-1] == 0 and 2 <= len(tau) <= S
        assert d.solver_schedule(S, skip_type, T - 1) == d.solver_schedule(S, skip_type)
    for bad in (0, -1, T, T + 5, 2.0, True, "3"):
        with pytest.raises(ValueError):
            d.solver_schedule(10, skip_type, bad)
    with pytest.raises(ValueError):
        d.solver_schedule(1, skip_type, 100)          # a tail visits t_start and 0


def test_logsnr_tail_is_the_nearest_index_to_uniform_lambda_below_the_start():
    d = _diffusion("linear")
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    lam = 0.5 * (np.log(ab) - np.log1p(-ab))
    for S, t_start in ((10, 200), (20, 400), (8, 37)):
        want = []
        for p in np.linspace(lam[t_start], lam[0], S):
            i = int(np.abs(lam[:t_start + 1] - p).argmin())
            if i not in want:
                want.append(i)
        assert d.solver_schedule(S, "logsnr", t_start) == want


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_three_symbols_are_declared_bound_exported_and_refuse_bad_arguments():
    from lion_amd import _lib, chain, diffusion_ops
    abi_check.declared_bound_and_exported(NEW)
    for name in NEW:
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "sde_dpmpp_update" in diffusion_ops.__all__
    assert chain.SDE_DPMPP == 3 and (chain.DDIM, chain.DDPM, chain.DPMPP) == (0, 1, 2)
    # bad arguments are refused on the host, before any launch (no GPU here: a launch would be a positive HIP error)
    l = _lib.load()
    buf = (ctypes.c_float * 16)()
    p = (ctypes.addressof(buf) + 15) & ~15          # 16-byte aligned, 8 floats behind it: never dereferenced here
    co = (156.0, 0.99998, 0.97, 4.1e-4, 1.5, -0.5, 0.02)
    c1 = co[:4] + (1.0, 0.0, 0.02)                   # a5 == 0
    c0 = co[:6] + (0.0,)                             # a6 == 0
    f = l.lion_sde_dpmpp_update                      # (x, eps, hist, z_in, numel, a0..a6, seed, word, stream, out, hist_out, z_out)
    assert f(None, p, p, p, 8, *co, p, 0, 0, p, p, p, None) == -1          # x
    assert f(p, None, p, p, 8, *co, p, 0, 0, p, p, p, None) == -1          # eps
    assert f(p, p, p, p, 8, *co, p, 0, 0, None, p, p, None) == -1          # out
    assert f(p, p, p, p, 8, *co, p, 0, 0, p, None, p, None) == -1          # hist_out
    assert f(p, p, None, p, 8, *co, p, 0, 0, p, p, p, None) == -1          # a5 != 0 reads hist
    assert f(p, p, p, None, 8, *co, None, 0, 0, p, p, p, None) == -1       # a6 != 0 needs z_in or seed
    assert f(p, p, p, p, 0, *co, p, 0, 0, p, p, p, None) == -1             # numel
    assert f(p, p, None, None, 0, *c1[:6], 0.0, None, 0, 0, p, p, None, None) == -1   # every optional absent: numel still counts
    assert f(p + 4, p, p, p, 2, *co, p, 0, 0, p, p, p, None) == -1         # 16-byte accesses: misaligned x
    assert f(p, p, p, p + 4, 2, *co, p, 0, 0, p, p, p, None) == -1         # ... z_in
    assert f(p, p, p, p, 2, *co, p, 0, 0, p, p + 8, p, None) == -1         # ... hist_out
    assert f(p, p, p, p, 2, *c0, p, 0, 0, p, p, p + 4, None) == -1         # ... z_out
    g = l.lion_chain_update_multistep_noise          # (x, eps, hist, numel, cur, table, seed, stream, out, hist_out, z_out)
    good = [p, p, p, 8, p, p, p, 0, p, p, None]
    for k in (0, 1, 2, 4, 5, 6, 8, 9):               # every required pointer
        a = list(good)
        a[k] = None
        assert g(*a, None) == -1, k
    assert g(p, p, p, 0, p, p, p, 0, p, p, None, None) == -1
    assert g(p, p + 4, p, 2, p, p, p, 0, p, p, None, None) == -1
    assert g(p, p, p, 2, p, p, p, 0, p, p, p + 4, None) == -1
    h = l.lion_chain_update_multistep_noise_cm       # (x, eps_cm, hist, B, N, cur, table, seed, stream, out, hist_out, z_out)
    good = [p, p, p, 1, 2, p, p, p, 0, p, p, None]
    for k in (0, 1, 2, 5, 6, 7, 9, 10):
        a = list(good)
        a[k] = None
        assert h(*a, None) == -1, k
    assert h(p, p, p, 0, 2, p, p, p, 0, p, p, None, None) == -1
    assert h(p, p, p, 1, 0, p, p, p, 0, p, p, None, None) == -1
    assert h(p, p, p + 4, 1, 2, p, p, p, 0, p, p, None, None) == -1
    assert h(p, p, p, 1, 2, p, p, p, 0, p + 8, p, None, None) == -1


def test_sde_update_has_no_cpu_path_and_checks_its_arguments():
    import torch
    from lion_amd import diffusion_ops
    x = torch.zeros(8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        diffusion_ops.sde_dpmpp_update(x, x, None, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0)


def test_new_keyword_arguments_exist_with_their_defaults():
    import inspect
    from lion_amd import editing, sampling
    from lion_amd.diffusion import DiffusionDiscretized
    from lion_amd.models.lion import LION
    par = inspect.signature(DiffusionDiscretized.run_dpm_solver).parameters
    assert (par["stochastic"].default, par["t_start"].default, par["seed"].default) == (False, None, None)
    par = inspect.signature(editing.diffuse_denoise).parameters
    assert (par["solver_steps"].default, par["stochastic"].default) == (None, True)
    assert inspect.signature(sampling.generate_samples_vada_2prior).parameters["dpm_stochastic"].default is False
    assert inspect.signature(LION.sample).parameters["dpm_stochastic"].default is False


# ---- exact covariance propagation on a linear-Gaussian toy ---------------------------------------------------------------------
# Data ~ N(0, s^2): the marginal at index t is N(0, v_t), v_t = ab_t*s^2 + 1 - ab_t, and the exact denoiser is
# eps = sigma_t*x / v_t, so x0 = c_t*x with c_t = alpha_t*s^2 / v_t.  One solver step is linear in (x, hist) plus independent
# noise: M = [[a2 + a3*a4*c_t, a3*a5], [c_t, 0]],  P <- M P M^T + diag(a6^2, 0),  from P = diag(v_start, 0).
# Error: |P_xx / v_0 - 1| on arrival at index 0 (before the last row, which returns the data prediction).
def variance_error(d, steps, order, s, stochastic=True):
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    v = ab * s * s + 1.0 - ab
    table = d.dpm_solver_table(steps, order, dtype=np.float64, stochastic=stochastic)
    P = np.diag([v[steps[0]], 0.0])
    for row, t in zip(table[:-1], steps[:-1]):
        a2, a3, a4, a5, a6 = row[3], row[4], row[5], row[6], row[7]
        c = np.sqrt(ab[t]) * s * s / v[t]
        M = np.array([[a2 + a3 * a4 * c, a3 * a5], [c, 0.0]])
        P = M @ P @ M.T + np.diag([a6 * a6, 0.0])
    return abs(P[0, 0] / v[0] - 1.0), P[0, 0]


def error_table(sched, S_list=(5, 10, 20, 50)):
    """{(start, s, S): (order-1 error, order-2 error, deterministic order-2 error)}: what DESIGN.md 4.6.4 prints"""
    d = _diffusion(sched)
    out = {}
    for start in STARTS:
        for s in SCALES:
            for S in S_list:
                steps = d.solver_schedule(S, "logsnr", start)
                out[(start, s, S)] = (variance_error(d, steps, 1, s)[0], variance_error(d, steps, 2, s)[0],
                                      variance_error(d, steps, 2, s, stochastic=False)[0])
    return out


@pytest.fixture(scope="module")
def linear_errors():
    return error_table("linear", (10, 20))


@pytest.mark.parametrize("S", [10, 20])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("start", STARTS)
def test_second_order_variance_error_is_a_third_of_first_orders(linear_errors, start, s, S):
    """'linear' schedule, 'logsnr' spacing: the error of order 2 in the variance on arrival at index 0 is at most a third
    of order 1's (= DDIM, kappa = 1).  Measured ratios over these 24 cells: 4.8 ... 52, the smallest 4.83 at start 100,
    s = 1.0, S = 10 (DESIGN.md 4.6.4 prints the table, with the 'cust' schedule's cells, which are not asserted)."""
    e1, e2, _ = linear_errors[(start, s, S)]
    print(f"start={start} s={s} S={S}: order 1 {e1:.3e}  order 2 {e2:.3e}  ratio {e1 / e2:.2f}")
    assert e2 <= e1 / 3.0, (e1, e2)


def test_deterministic_rows_keep_the_variance_on_this_toy_only_up_to_their_order():
    """the recursion itself: with a6 = 0 and the probability-flow rows it reproduces the deterministic chain, whose state is
    x_start times a scalar -- P_xx is that scalar squared times v_start (run in float64 beside it)"""
    d = _diffusion("linear")
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    s = 0.5
    v = ab * s * s + 1.0 - ab
    steps = d.solver_schedule(10, "logsnr", 400)
    table = d.dpm_solver_table(steps, 2, dtype=np.float64)
    x, hist = 1.0, 0.0
    for row, t in zip(table[:-1], steps[:-1]):
        x0 = row[1] * (x - row[2] * (np.sqrt(1 - ab[t]) * x / v[t]))
        D = row[5] * x0 + row[6] * hist
        x, hist = row[3] * x + row[4] * D, x0
    _, pxx = variance_error(d, steps, 2, s, stochastic=False)
    assert abs(pxx - x * x * v[400]) <= 1e-12 * pxx


if __name__ == "__main__":      # the tables of DESIGN.md 4.6.4
    for sched in SCHEDULES:
        tab = error_table(sched)
        print(f"\n{sched}: ratio order 1 / order 2 of |P_xx/v_0 - 1|   (in brackets: SDE order 2 / deterministic order 2)")
        print("start  s     " + "".join(f"S={S:<18d}" for S in (5, 10, 20, 50)))
        for start in STARTS:
            for s in SCALES:
                cells = []
                for S in (5, 10, 20, 50):
                    e1, e2, ed = tab[(start, s, S)]
                    cells.append(f"{e1 / e2:7.2f} [{e2 / ed:6.2f}]    ")
                print(f"{'T-1' if start is None else start:<6} {s:<5} " + "".join(cells))
