"""Float64 restatement of scipy's RK45 (scipy/integrate/_ivp/rk.py RK45 + RungeKutta._step_impl, common.py
select_initial_step / norm, base.py OdeSolver.step): the oracle of the device solver (lion_amd/csrc/ode.hip).

Stage sums run in ascending stage order with one rounding per operation, as the device does; scipy's np.dot may order
or fuse them differently, which moves results by ulps (tests/test_ode_cpu.py bounds that against solve_ivp itself)."""
import math

import numpy as np

C = [0.0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0]
A = [[], [1 / 5], [3 / 40, 9 / 40], [44 / 45, -56 / 15, 32 / 9],
     [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
     [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656]]
BW = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]
E = [-71 / 57600, 0, 71 / 16695, -71 / 1920, 17253 / 339200, -22 / 525, 1 / 40]
SAFETY, MIN_FACTOR, MAX_FACTOR, ERR_EXP = 0.9, 0.2, 10, -1 / 5


def rms(x):
    return np.linalg.norm(x) / x.size ** 0.5


def combo(K, w):
    """sum_j K[j] * w[j], ascending j"""
    acc = K[0] * w[0]
    for j in range(1, len(w)):
        acc = acc + K[j] * w[j]
    return acc


def stage_state(y, K, h, s):
    """the argument of evaluation s (1..5) of a step, and y_new for s == 6"""
    if s == 6:
        return y + h * combo(K, BW)
    return y + combo(K, A[s]) * h


def error_norm(y, y_new, K, h, rtol, atol):
    scale = atol + np.maximum(np.abs(y), np.abs(y_new)) * rtol
    return rms((combo(K, E) * h) / scale)


def step_factor(en, rejected_before):
    """(accepted, factor) of one attempt with error norm en"""
    if en < 1:
        factor = MAX_FACTOR if en == 0 else min(MAX_FACTOR, SAFETY * en ** ERR_EXP)
        if rejected_before:
            factor = min(1, factor)
        return True, factor
    return False, max(MIN_FACTOR, SAFETY * en ** ERR_EXP)


def min_step(t, direction):
    return 10 * np.abs(np.nextafter(t, direction * np.inf) - t)


def initial_step(fun, t0, y0, t_bound, f0, direction, rtol, atol, order=4):
    interval = abs(t_bound - t0)
    if interval == 0.0:
        return 0.0
    scale = atol + np.abs(y0) * rtol
    d0, d1 = rms(y0 / scale), rms(f0 / scale)
    h0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    h0 = min(h0, interval)
    y1 = y0 + h0 * direction * f0
    f1 = fun(t0 + h0 * direction, y1)
    d2 = rms((f1 - f0) / scale) / h0
    if d1 <= 1e-15 and d2 <= 1e-15:
        h1 = max(1e-6, h0 * 1e-3)
    else:
        h1 = (0.01 / max(d1, d2)) ** (1 / (order + 1))
    return min(100 * h0, h1, interval)


def rk45(fun, t0, t_bound, y0, rtol, atol, max_attempts=100000):
    """solve_ivp(fun, (t0, t_bound), y0, method='RK45', rtol=rtol, atol=atol) to the end of the span.
    Returns dict(y, t, nfe, n_accepted, n_rejected, ts (accepted times, t0 first), status: 'finished' | 'failed')."""
    count = [0]

    def f(t, y):
        count[0] += 1
        return np.asarray(fun(t, y), dtype=np.float64)

    t = float(t0)
    y = np.asarray(y0, dtype=np.float64).copy()
    direction = np.sign(t_bound - t0) if t_bound != t0 else 1
    fc = f(t, y)
    h_abs = initial_step(f, t, y, t_bound, fc, direction, rtol, atol)
    ts, acc, rej, attempts = [t], 0, 0, 0
    out = lambda status: dict(y=y, t=t, nfe=count[0], n_accepted=acc, n_rejected=rej, ts=ts, status=status)
    while t != t_bound:
        ms = min_step(t, direction)
        h_abs = max(h_abs, ms)
        rejected = False
        while True:
            if h_abs < ms:
                return out('failed')
            attempts += 1
            assert attempts < max_attempts
            h = h_abs * direction
            t_new = t + h
            if direction * (t_new - t_bound) > 0:
                t_new = t_bound
            h = t_new - t
            h_abs = abs(h)
            K = [fc]
            for s in range(1, 6):
                K.append(f(t + C[s] * h, stage_state(y, K, h, s)))
            y_new = stage_state(y, K, h, 6)
            f_new = f(t + h, y_new)
            K.append(f_new)
            ok, factor = step_factor(error_norm(y, y_new, K, h, rtol, atol), rejected)
            h_abs *= factor
            if ok:
                break
            rejected = True
            rej += 1
        t, y, fc = t_new, y_new, f_new
        acc += 1
        ts.append(t)
        if direction * (t - t_bound) >= 0:
            break
    return out('finished')


# ---- the VPSDE PF-ODE of Gaussian data N(0, s^2 I), in closed form -------------------------------------------------

def vp_log_mean(t, b0=0.1, b1=20.0):
    """log m(t) = -(b0 t + (b1 - b0) t^2 / 2) / 2"""
    return -0.5 * (b0 * t + 0.5 * (b1 - b0) * t * t)


def vp_var(t, b0=0.1, b1=20.0, sigma2_0=0.0):
    return 1.0 - (1.0 - sigma2_0) * math.exp(2 * vp_log_mean(t, b0, b1))


def gaussian_drift(t, y, s2, b0=0.1, b1=20.0):
    """dx/dt = f x + g2/2 * eps*(x, t) / sigma_t with the exact eps* = sigma_t x / (m^2 s^2 + sigma_t^2)"""
    g2 = b0 + (b1 - b0) * t
    m2 = math.exp(2 * vp_log_mean(t, b0, b1))
    return -0.5 * g2 * y + 0.5 * g2 * y / (m2 * s2 + vp_var(t, b0, b1))


def gaussian_flow(x0, t0, t1, s2, b0=0.1, b1=20.0):
    """x(t1) of the PF-ODE started at x(t0) = x0"""
    tot = lambda t: math.exp(2 * vp_log_mean(t, b0, b1)) * s2 + vp_var(t, b0, b1)
    return x0 * math.sqrt(tot(t1) / tot(t0))
