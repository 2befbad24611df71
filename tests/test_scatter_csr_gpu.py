"""-m gpu: the atomics-free backward scatters (csrc/scatter_csr.hip) behind grouping / 3-NN interpolation / devoxelize
backward: against the sum carried out in float64, against the legacy LDS-atomic entry points of the C ABI (which stay the
fallback), bit-for-bit reproducible, on ragged shapes (bins not a multiple of 8, E not a multiple of the workgroup, empty
bins, one bin holding most entries).  Reference: grouping.cu:58-80, neighbor_interpolate.cu:145-170, trilinear_devox.cu:119-162."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref(gy, idx, w, S, bins):
    B, C = gy.shape[:2]
    g = gy.reshape(B, C, -1).double().cpu().numpy()
    ix = idx.reshape(B, -1).cpu().numpy()
    ww = None if w is None else w.reshape(B, -1).double().cpu().numpy()
    out = np.zeros((B, C, bins))
    E = ix.shape[1]
    src = np.arange(E) % S
    for b in range(B):
        contrib = g[b][:, src] * (1.0 if ww is None else ww[b][None, :])
        for c in range(C):
            np.add.at(out[b, c], np.clip(ix[b], 0, bins - 1), contrib[c])
    return out


@pytest.mark.parametrize("B,C,N,M,U", [(2, 35, 2048, 1024, 32), (3, 7, 203, 51, 5), (1, 67, 16, 16, 4)])
def test_grouping_backward_csr(B, C, N, M, U):
    from lion_amd import _lib
    from lion_amd.functional.backend import _backend as bk
    g = torch.Generator(device="cuda").manual_seed(N + M)
    idx = torch.randint(0, N, (B, M, U), device="cuda", dtype=torch.int32, generator=g)
    idx[:, : M // 2] = 3 % N                       # one bin holds half of all entries
    gy = torch.randn(B, C, M, U, device="cuda", generator=g)
    got = bk.grouping_backward(gy, idx, N)
    again = bk.grouping_backward(gy, idx, N)
    assert torch.equal(got, again), "not reproducible"
    ref = _ref(gy, idx, None, M * U, N)
    assert np.abs(got.double().cpu().numpy() - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1.0)
    legacy = torch.empty(B, C, N, device="cuda")
    _lib.check(_lib.load().lion_grouping_backward(_lib.ptr(gy), _lib.ptr(idx), B, C, N, M, U, _lib.ptr(legacy),
                                                  _lib.stream_ptr(gy.device)), "grouping_backward")
    assert (legacy - got).abs().max().item() <= 1e-4 * max(got.abs().max().item(), 1.0)


@pytest.mark.parametrize("B,C,N,M", [(2, 192, 2048, 1024), (3, 5, 333, 77), (1, 16, 64, 16)])
def test_three_nn_interpolate_backward_csr(B, C, N, M):
    from lion_amd import _lib
    from lion_amd.functional.backend import _backend as bk
    g = torch.Generator(device="cuda").manual_seed(N * 7 + M)
    idx = torch.randint(0, M, (B, 3, N), device="cuda", dtype=torch.int32, generator=g)
    w = torch.rand(B, 3, N, device="cuda", generator=g)
    gy = torch.randn(B, C, N, device="cuda", generator=g)
    got = bk.three_nearest_neighbors_interpolate_backward(gy, idx, w, M)
    assert torch.equal(got, bk.three_nearest_neighbors_interpolate_backward(gy, idx, w, M))
    ref = _ref(gy, idx, w, N, M)
    assert np.abs(got.double().cpu().numpy() - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1.0)
    legacy = torch.empty(B, C, M, device="cuda")
    _lib.check(_lib.load().lion_three_nn_interpolate_backward(_lib.ptr(gy), _lib.ptr(idx), _lib.ptr(w), B, C, N, M,
                                                              _lib.ptr(legacy), _lib.stream_ptr(gy.device)), "legacy")
    assert (legacy - got).abs().max().item() <= 1e-4 * max(got.abs().max().item(), 1.0)


@pytest.mark.parametrize("B,C,N,r", [(2, 64, 2048, 32), (2, 16, 500, 16), (1, 8, 64, 8)])
def test_trilinear_devoxelize_backward_csr(B, C, N, r):
    from lion_amd import _lib
    from lion_amd.functional.backend import _backend as bk
    g = torch.Generator(device="cuda").manual_seed(N + r)
    r3 = r ** 3
    inds = torch.randint(0, r3, (B, 8, N), device="cuda", dtype=torch.int32, generator=g)
    wg = torch.rand(B, 8, N, device="cuda", generator=g)
    gy = torch.randn(B, C, N, device="cuda", generator=g)
    # the product op keeps the LDS-atomic kernel here (faster for 32768 mostly empty bins); the atomics-free path itself:
    got = bk._scatter_csr(gy, inds, wg, N, 8 * N, r3, "devoxelize_backward (csr)")
    assert got is not None and torch.equal(got, bk._scatter_csr(gy, inds, wg, N, 8 * N, r3, "devoxelize_backward (csr)"))
    ref = _ref(gy, inds, wg, N, r3)
    assert np.abs(got.double().cpu().numpy() - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1.0)
    legacy = torch.empty(B, C, r3, device="cuda")
    _lib.check(_lib.load().lion_trilinear_devoxelize_backward(_lib.ptr(gy), _lib.ptr(inds), _lib.ptr(wg), B, C, N, r3,
                                                              _lib.ptr(legacy), _lib.stream_ptr(gy.device)), "legacy")
    assert (legacy - got).abs().max().item() <= 1e-4 * max(got.abs().max().item(), 1.0)


# ---- the ORDER of the sums: bit-for-bit against the ascending-entry-order fp32 sum of tests/train_norm_ref.py --------------
# (tests/test_train_norm_reference_cpu.py shows that reversing one long bin changes bits, so an order or membership bug in
# csr_build_kernel cannot pass these.)

import train_norm_ref as tr  # noqa: E402

CSR_EPT_NT = 32 * 1024          # CSR_EPT * CSR_NT: up to here the long bins are ranked by their entries
CSR_SHORT = 32


def host_ct(B, C, S):
    """channels per workgroup of the apply, by the same lines as lion_scatter_csr"""
    ct = (128 * 1024) // (S * 4)
    assert ct >= 1
    ct = min(ct, 16, C)
    while ct > 1 and B * ((C + ct - 1) // ct) < 256:
        ct >>= 1
    return ct


def csr_direct(gy, idx, w, S, bins):
    """lion_scatter_csr itself on host-made inputs -> numpy [B, C, bins]"""
    from lion_amd import _lib
    B, C = gy.shape[:2]
    E = idx.shape[1]
    wsb = _lib.load().lion_scatter_csr_workspace_bytes(B, E, bins)
    assert wsb > 0
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    gx = torch.full((B, C, bins), float("nan"), device="cuda")
    dw = None if w is None else torch.from_numpy(w).cuda()
    _lib.call("lion_scatter_csr", torch.from_numpy(gy).cuda(), torch.from_numpy(idx).cuda(), dw, B, C, S, E, bins, ws, wsb, gx)
    return gx.cpu().numpy()


def check_order(gy, idx, w, S, bins, what):
    for ww in (None, w):
        got = csr_direct(gy, idx, ww, S, bins)
        want = tr.scatter_in_order32(gy, idx, ww, S, bins)
        bad = np.flatnonzero((got != want).any(axis=(0, 1)))
        assert np.array_equal(got, want), f"{what} weights={ww is not None}: bins {bad[:8]} differ from the ordered sum"
        assert np.array_equal(got, csr_direct(gy, idx, ww, S, bins)), f"{what}: not reproducible"


def entries_with_bin_lengths(rng, E, lengths, bins):
    """idx int32 [E]: bin k holds exactly lengths[k] entries for k < len(lengths), the rest fall at random into the bins
    behind them; the entries of every bin are spread over the whole entry range"""
    fixed = np.repeat(np.arange(len(lengths)), lengths)
    rest = rng.integers(len(lengths), bins, E - fixed.size)
    return rng.permutation(np.concatenate([fixed, rest])).astype(np.int32)


def values(rng, B, C, S, E):
    return rng.standard_normal((B, C, S)).astype(np.float32), rng.uniform(0.1, 1.0, (B, E)).astype(np.float32)


def test_csr_order_at_every_bin_length_of_the_ranking_path():
    """E = 32768 = CSR_EPT * CSR_NT, the largest entry set whose long bins are ranked: bins of 0, 1, 3, 4, 5 (the apply's
    4-at-a-time list reads and their tail), 31, 32 (insertion sort), 33 (the first ranked length: the rank loop's 8-at-a-time
    body and a tail of 1), 64, 1025 and one of 16384 entries, in one call"""
    rng = np.random.default_rng(0)
    B, C, E, bins = 2, 3, CSR_EPT_NT, 300
    lengths = [0, 1, 3, 4, 5, 31, 32, 33, 64, 1025, 16384]
    idx = np.stack([entries_with_bin_lengths(rng, E, lengths, bins) for _ in range(B)])
    assert np.bincount(idx[1], minlength=bins)[:len(lengths)].tolist() == lengths
    gy, w = values(rng, B, C, E, E)
    check_order(gy, idx, w, E, bins, "ranking path")


def test_csr_order_beyond_the_ranked_entry_count():
    """E = 32768 + 40: the long bins keep the thread-per-bin insertion sort, O(c^2) dependent global steps in ONE thread for a
    bin of c entries.  No bin here holds more than 300 entries, and none may: a bin of thousands of entries would run for
    minutes in this regime and look like a hang (the limit stands in the header of csrc/scatter_csr.hip)."""
    rng = np.random.default_rng(1)
    B, C, E, bins = 1, 3, CSR_EPT_NT + 40, 600
    S = E // 8                                     # 8 entries per source, as devoxelize has: S = E rows would not fit the LDS
    idx = entries_with_bin_lengths(rng, E, [300, 33, 32, 0, 64], bins)[None]
    assert np.bincount(idx[0]).max() <= 300 and E > CSR_EPT_NT and S * 8 == E
    gy, w = values(rng, B, C, S, E)
    check_order(gy, idx, w, S, bins, "insertion-sort regime")


@pytest.mark.parametrize("bins", [1, 7, 8, 9, 1000])
def test_csr_order_over_bin_counts_and_clamped_indices(bins):
    """fewer bins than the 8 ranges of the build, exactly 8, 9 (span 2: ranges 5-7 are empty and the last non-empty range holds
    one bin), many; indices below 0 and at or above `bins` land in bins 0 and bins - 1"""
    rng = np.random.default_rng(bins)
    B, C, E = 2, 5, 2000
    idx = rng.integers(-3, bins + 3, (B, E)).astype(np.int32)
    assert (idx < 0).any() and (idx >= bins).any()
    gy, w = values(rng, B, C, E, E)
    check_order(gy, idx, w, E, bins, f"bins={bins}")
    got = csr_direct(gy[:, :1], np.full((B, E), -5, np.int32), None, E, bins)
    assert np.all(got[:, :, 1:] == 0) and np.all(got[:, :, 0] != 0)
    got = csr_direct(gy[:, :1], np.full((B, E), bins + 5, np.int32), None, E, bins)
    assert np.all(got[:, :, :-1] == 0) and np.all(got[:, :, -1] != 0)


@pytest.mark.parametrize("S,mult", [(100, 3), (101, 3), (100, 8), (101, 8)])
def test_csr_order_of_a_weighted_scatter_with_more_entries_than_sources(S, mult):
    """S != E (entry e reads element e mod S: 3-NN interpolation and devoxelize), S % 4 in {0, 1}: the float4 and the scalar
    staging of the gy rows"""
    rng = np.random.default_rng(S + mult)
    B, C, E, bins = 2, 7, S * mult, 37
    idx = rng.integers(0, bins, (B, E)).astype(np.int32)
    gy, w = values(rng, B, C, S, E)
    check_order(gy, idx, w, S, bins, f"S={S} E={E}")


@pytest.mark.parametrize("B,C,S,bins,ct,last", [(8, 500, 64, 40, 16, 4), (8, 100, 10000, 777, 3, 1), (1, 2, 32768, 2048, 1, 1)])
def test_csr_order_over_channel_tilings(B, C, S, bins, ct, last):
    """CT = 16 with a last group of 4 channels; CT = 3 (not a power of two) with a last group of 1; CT = 1 with 128 KiB of LDS.
    The asserted CT is computed as lion_scatter_csr does: a retune fails here instead of emptying the test."""
    assert host_ct(B, C, S) == ct and C - (C - 1) // ct * ct == last
    assert S * 4 * ct <= 128 * 1024
    rng = np.random.default_rng(C)
    idx = rng.integers(0, bins, (B, S)).astype(np.int32)
    gy, w = values(rng, B, C, S, S)
    check_order(gy, idx, w, S, bins, f"CT={ct}")


def test_csr_rejections_are_taken_on_the_host():
    """more bins per range than 60 KiB of LDS counters hold; a workspace one byte short -- both before any launch"""
    from lion_amd import _lib
    lib = _lib.load()
    B, C, S, E = 1, 1, 4, 4
    st = _lib.stream_ptr()
    gy, idx = torch.ones(B, C, S, device="cuda"), torch.zeros(B, E, device="cuda", dtype=torch.int32)
    for bins, short, want in ((8 * 15361, 0, -2), (8 * 15360, 1, -3), (16, 1, -3)):
        wsb = lib.lion_scatter_csr_workspace_bytes(B, E, bins)
        ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
        gx = torch.full((B, C, bins), float("nan"), device="cuda")
        got = lib.lion_scatter_csr(_lib.ptr(gy), _lib.ptr(idx), None, B, C, S, E, bins, _lib.ptr(ws), wsb - short, _lib.ptr(gx), st)
        assert got == want, (bins, short, got)
        torch.cuda.synchronize()
        assert torch.isnan(gx).all()
