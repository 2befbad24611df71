"""The arithmetic of the single-product convolution (csrc/conv3d_half.hip) restated in numpy and held to its contract on
the CPU: with the split kernels' exact power-of-two block scaling the ONE fp16 piece kept per operand is the operand
rounded to an 11-bit significand (round to nearest even) at any magnitude -- operands more than 2^27 below their block's
maximum go subnormal -- so the GEMM is rne11(W) rne11(X) accumulated in fp32:
  sharp:        |D - rne11(W) rne11(X)| < 5e-6 of the column maximum   (the fp32-class bound the GPU tests use),
  elementwise:  |D - W X| <= 2^-10 sum |w||x|                          (two roundings of 2^-11 each).
K = 1728 = 64 channels x 27 taps, the production layer's reduction length.  (The kernel itself: test_conv_half_gpu.py.)"""
import numpy as np
import pytest

from test_split_numerics_cpu import CASES, cut, scale_exp, split_gemm

BOUND = 5e-6
M, K, N = 48, 1728, 64


def half_gemm(W, X, headroom=0):
    """split_gemm of test_split_numerics_cpu.py with one piece: main += W_h X_h, no low pieces, no corr"""
    ew = scale_exp(np.abs(W).max())
    Wh = cut(W * np.float32(2.0 ** ew))[0].astype(np.float32)
    main = np.zeros((W.shape[0], X.shape[1]), np.float32)
    E = np.full(X.shape[1], 127)
    for k0 in range(0, W.shape[1], 16):
        xc = X[k0:k0 + 16]
        m = np.abs(xc).max(0)
        for n in np.nonzero(m > 0)[0]:
            e = scale_exp(m[n])
            if e < E[n]:
                if E[n] != 127:
                    main[:, n] *= np.float32(2.0 ** (e - headroom - E[n]))
                E[n] = e - headroom
        xs = np.where(E == 127, 1.0, 2.0 ** E.astype(np.float64)).astype(np.float32)
        main += Wh[:, k0:k0 + 16] @ cut(xc * xs[None, :])[0].astype(np.float32)
    us = np.where(E == 127, 1.0, 2.0 ** (-E.astype(np.float64))).astype(np.float32)
    return (main * us[None, :]) * np.float32(2.0 ** -ew)


def rne11(a):
    m, e = np.frexp(a.astype(np.float64))
    return np.ldexp(np.round(m * 2048.0) / 2048.0, e)


def operands(case, rng):
    W = rng.standard_normal((M, K)).astype(np.float32)
    X = rng.standard_normal((K, N)).astype(np.float32)
    if case == "nine-decades":
        X = (np.exp(rng.uniform(np.log(1e-6), np.log(1e4), X.shape)) * rng.choice([-1.0, 1.0], X.shape)).astype(np.float32)
    elif case == "beyond-fp16-max":
        X *= np.float32(3.0e6)
    elif case == "tiny":
        X *= np.float32(1e-30)
    elif case == "per-column-scales":
        X *= np.exp(rng.uniform(np.log(1e-6), np.log(1e7), (1, N))).astype(np.float32)
    elif case == "huge-one-chunk":
        X[32:48] *= np.float32(1e4)
        X[:16] *= np.float32(1e-3)
    elif case == "tiny-weights":
        W *= np.float32(1e-9)
    elif case == "huge-weights":
        W *= np.float32(1e6)
    elif case == "residual-bits":
        k = rng.integers(-2048, 2048, X.shape).astype(np.float32)
        X = ((1.0 + k * 2.0 ** -22) * rng.choice([-1.0, 1.0], X.shape)).astype(np.float32)
    return W, X


def col_err(got, ref):
    """largest |got - ref| as a fraction of the column's maximum |ref|"""
    return (np.abs(got.astype(np.float64) - ref).max(0) / np.maximum(np.abs(ref).max(0), 1e-300)).max()


@pytest.mark.parametrize("headroom", [0, 4])
@pytest.mark.parametrize("case", CASES)
def test_one_piece_product_meets_both_bounds(case, headroom):
    assert len(CASES) == 9
    W, X = operands(case, np.random.default_rng(7))
    W64, X64 = W.astype(np.float64), X.astype(np.float64)
    got = half_gemm(W, X, headroom)
    assert np.isfinite(got).all()
    emul = rne11(W) @ rne11(X)
    exact = W64 @ X64
    e_emul = col_err(got, emul)
    ratio = (np.abs(got.astype(np.float64) - exact) / (2.0 ** -10 * (np.abs(W64) @ np.abs(X64)))).max()
    print(f"{case} H={headroom}: vs rounded operands {e_emul:.2e} of the column maximum; "
          f"|err| / (2^-10 sum|w||x|) <= {ratio:.3f}")
    assert e_emul < BOUND, (case, e_emul)
    assert ratio <= 1.0, (case, ratio)


def test_power_of_two_scaling_is_exact():
    rng = np.random.default_rng(3)
    W = rng.standard_normal((32, 48)).astype(np.float32)
    X = rng.standard_normal((48, 16)).astype(np.float32)
    for headroom in (0, 4):
        base = half_gemm(W, X, headroom)
        for k in (-80, -17, 9, 40, 80):
            f = np.float32(2.0 ** k)
            assert np.array_equal(half_gemm(W, X * f, headroom), base * f), k
            assert np.array_equal(half_gemm(W * f, X, headroom), base * f), k


def test_the_two_yardsticks_tell_the_modes_apart():
    """the control: one piece is MORE than 5e-6 max away from the exact product (the precision is reduced), and the
    three-product model is MORE than 5e-6 max away from the rounded-operand emulation (it is not what one piece computes)"""
    W, X = operands("normal", np.random.default_rng(7))
    exact = W.astype(np.float64) @ X.astype(np.float64)
    emul = rne11(W) @ rne11(X)
    mx = np.abs(exact).max()
    assert np.abs(half_gemm(W, X) - exact).max() > BOUND * mx
    assert np.abs(split_gemm(W, X) - emul).max() > BOUND * mx
    assert np.abs(split_gemm(W, X) - exact).max() < BOUND * mx and np.abs(half_gemm(W, X) - emul).max() < BOUND * mx
