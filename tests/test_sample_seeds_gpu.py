"""-m gpu: per-shape seeds.  The keyed draw (lion_philox_normal_keyed) against the single-seed kernels, sample by sample and bit for
bit; the keyed update kernels against a float32 numpy restatement on the noise they report; the captured keyed step against the
eager step on the real priors; graph against eager through the samplers; and what the feature is for: a sample's noise, start
and result do not depend on its position in the batch or on its batchmates, and a job's shapes not on how it is sharded."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KA, KB, KC, KD, KE = 0x1234567890ABCDEF, 0x0FEDCBA987654321, 0xDEADBEEF00000001, 5, 2 ** 64 - 7
KEYS = (KA, KB, KC)
STEP = 5
START, DIFFUSE = 0xFFFFFFFE, 0xFFFFFFFF
#             a0       a1       a2    a3      a4   a5    a6       the multistep-noise rows of tests/test_sde_solver_gpu.py
MS_ROWS = {"first": (156.0, 0.99998, 0.93, 8.1e-4, 1.0, 0.0, 0.31),
           "second": (156.0, 0.99998, 0.93, 8.1e-4, 1.5, -0.5, 0.31),
           "final": (1.00005, 0.01, 0.0, 1.0, 1.0, 0.0, 0.0),
           "identity": (1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)}
#              mode  a0     a1     a2    a3    a4   a5
UN_ROWS = {"ddim": (0, 1.002, -0.03, 0.05, 0.0, 0.0, 0.0),            # out = x*s + (c*eps + sigma*z)
           "ddpm": (1, 1.01, 0.02, 0.7, 0.14, 0.9, 0.0),              # t > 0: a0*(x - a1*eps/a2) + (a3*z)*a4
           "ddpm_t0": (1, 1.01, 0.02, 1.0, 0.14, 0.9, 1.0)}           # t == 0 (a5 != 0): a0*(x - a1*eps)
LAYOUTS = [("flat", 3, 128), ("cm", 2, 5), ("cm", 2, 257)]            # flat: (B, n); channel-major: (B, N), n = 4*N


def _words(keys):
    from lion_amd.chain import key_words
    return key_words(list(keys), "cuda")


def _cur(row, step):
    """cur as lion_chain_begin_step leaves it for table row `step` holding `row` = a0..a5"""
    cur = torch.zeros(8, device="cuda")
    cur[1:1 + len(row)] = torch.tensor([float(v) for v in row], device="cuda")
    cur.view(torch.int32)[7] = step - 2 ** 32 if step >= 2 ** 31 else step      # the word's bits
    return cur


@functools.lru_cache(maxsize=None)
def _single(n, step, stream_id, seed):
    """the z today's single-seed lion_chain_update_noise reports for an n-element tensor under `seed` (computed once, never
    written afterwards)"""
    from lion_amd import _lib
    x = torch.zeros(n, device="cuda")
    out, z = torch.empty_like(x), torch.empty_like(x)
    _lib.call("lion_chain_update_noise", 0, x, x, n, _cur((1.0,), step), _words([seed])[0], stream_id, out, z)
    return z


def _keyed(keys, n, step, stream_id=0):
    from lion_amd.diffusion_ops import philox_normal_keyed
    return philox_normal_keyed(list(keys), len(keys), [n], step, stream_id=stream_id)


# ---- 1. the keyed draw is the single-seed kernel's, per sample ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 128, 1020, 1028, 8192])
def test_keyed_draw_equals_single_seed_kernel_per_sample(n):
    z = _keyed(KEYS, n, STEP)
    assert tuple(z.shape) == (3, n) and torch.isfinite(z).all()
    for b, key in enumerate(KEYS):
        assert torch.equal(z[b], _single(n, STEP, 0, key)), (n, b)
        assert z[b].any()
    assert not torch.equal(z[0], z[1]) and not torch.equal(z[1], z[2])
    assert not torch.equal(z, _keyed(KEYS, n, STEP + 1)) and not torch.equal(z, _keyed(KEYS, n, STEP, 1))
    for b, key in enumerate(KEYS):                          # ... sample by sample
        assert not torch.equal(z[b], _single(n, STEP + 1, 0, key)) and not torch.equal(z[b], _single(n, STEP, 1, key))
    # the two reserved words: each the single-seed kernel's draw at that word, and apart from each other
    zs, zd = _keyed(KEYS, n, START), _keyed(KEYS, n, DIFFUSE)
    for b, key in enumerate(KEYS):
        assert torch.equal(zs[b], _single(n, START, 0, key)) and torch.equal(zd[b], _single(n, DIFFUSE, 0, key))
        assert not torch.equal(zs[b], zd[b]) and not torch.equal(zs[b], z[b])
    # equal keys give equal rows; neither the batch size nor the position nor the batchmates matter
    same = _keyed((KB, KB, KA, KB), n, STEP)
    assert torch.equal(same[0], same[1]) and torch.equal(same[1], same[3]) and torch.equal(same[0], z[1])
    assert torch.equal(same[2], z[0])
    assert torch.equal(_keyed((KC,), n, STEP)[0], z[2])


def test_keyed_draw_wrapper_refusals():
    from lion_amd.diffusion_ops import philox_normal_keyed
    for shape in ([6], [0], [3, 1]):
        with pytest.raises(ValueError):
            philox_normal_keyed([1, 2], 2, shape, 0)
    with pytest.raises(ValueError):
        philox_normal_keyed([1, 2, 3], 2, [8], 0)


# ---- 2. the keyed update kernels -------------------------------------------------------------------------------------------------
def _layout(layout, B, n_or_N, seed):
    """x, eps as the kernel takes it, eps in x's layout (numpy), the per-sample element count, the entry-point suffix + sizes"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if layout == "flat":
        x = torch.randn(B, n_or_N, device="cuda", generator=g)
        eps = torch.randn(B, n_or_N, device="cuda", generator=g)
        return x, eps, eps.cpu().numpy(), n_or_N, "", (B, n_or_N)
    x = torch.randn(B, n_or_N, 4, device="cuda", generator=g)
    eps_cm = torch.randn(B, 4, n_or_N, device="cuda", generator=g)
    return x, eps_cm, eps_cm.permute(0, 2, 1).contiguous().cpu().numpy(), 4 * n_or_N, "_cm", (B, n_or_N)


def _restate_update(x, e, z, row):
    mode, a0, a1, a2, a3, a4, a5 = [row[0]] + [np.float32(v) for v in row[1:]]
    if mode == 0:
        return x * a0 + (a1 * e + a2 * z)
    if a5 != 0:
        return a0 * (x - a1 * e)
    return a0 * (x - a1 * e / a2) + (a3 * z) * a4


@pytest.mark.parametrize("layout,B,size", LAYOUTS)
@pytest.mark.parametrize("kind", list(UN_ROWS))
def test_keyed_update_noise_equals_float32_numpy(kind, layout, B, size):
    from lion_amd import _lib
    row = UN_ROWS[kind]
    keys = KEYS[:B]
    x, eps, e_np, n, suffix, sizes = _layout(layout, B, size, 11)
    x_keep, eps_keep = x.clone(), eps.clone()
    out, z = torch.empty_like(x), torch.full_like(x, float("nan"))
    _lib.call("lion_chain_update_noise%s_keyed" % suffix, row[0], x, eps, *sizes, _cur(row[1:], STEP), _words(keys), 0, out, z)
    want = _restate_update(x.cpu().numpy(), e_np.reshape(x.shape), z.cpu().numpy(), row)
    assert np.isfinite(want).all() and torch.equal(out, torch.from_numpy(want).cuda())
    for b, key in enumerate(keys):                          # the reported z is the keyed draw of test 1 for the cur step word
        assert torch.equal(z[b].reshape(-1), _single(n, STEP, 0, key)), (kind, layout, b)
    assert torch.equal(x, x_keep) and torch.equal(eps, eps_keep)            # inputs untouched
    x2 = x.clone()                                          # in place and without z_out, as the captured step runs it
    _lib.call("lion_chain_update_noise%s_keyed" % suffix, row[0], x2, eps, *sizes, _cur(row[1:], STEP), _words(keys), 0, x2, None)
    assert torch.equal(x2, out)


def _restate_multistep(x, e, h, z, row):
    a0, a1, a2, a3, a4, a5, a6 = (np.float32(v) for v in row)
    x0 = a0 * (x - a1 * e)
    D = a4 * x0 if a5 == 0 else a4 * x0 + a5 * h
    out = a2 * x + a3 * D
    return (out + a6 * z if a6 != 0 else out), x0


@pytest.mark.parametrize("layout,B,size", LAYOUTS)
@pytest.mark.parametrize("kind", list(MS_ROWS))
def test_keyed_multistep_noise_equals_float32_numpy(kind, layout, B, size):
    from lion_amd import _lib
    row = MS_ROWS[kind]
    keys = KEYS[:B]
    x, eps, e_np, n, suffix, sizes = _layout(layout, B, size, 13)
    hist = torch.randn(x.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(17))
    if row[5] == 0:
        hist.fill_(float("nan"))                           # a5 == 0: hist is not read
    keep = [t.clone() for t in (x, eps, hist)]
    table = torch.zeros(STEP + 2, 8, device="cuda")
    table[STEP, 7] = row[6]
    name = "lion_chain_update_multistep_noise%s_keyed" % suffix
    out, h_out, z = torch.empty_like(x), torch.empty_like(x), torch.full_like(x, float("nan"))
    _lib.call(name, x, eps, hist, *sizes, _cur(row[:6], STEP), table, _words(keys), 0, out, h_out, z)
    want, want_h = _restate_multistep(x.cpu().numpy(), e_np.reshape(x.shape), hist.cpu().numpy(), z.cpu().numpy(), row)
    assert np.isfinite(want).all() and np.isfinite(want_h).all()
    assert torch.equal(out, torch.from_numpy(want).cuda()) and torch.equal(h_out, torch.from_numpy(want_h).cuda())
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((x, eps, hist), keep))   # inputs untouched
    if row[6] != 0:
        for b, key in enumerate(keys):
            assert torch.equal(z[b].reshape(-1), _single(n, STEP, 0, key)), (kind, layout, b)
    else:
        # nothing is drawn: zeros are reported, and the result is the same whatever the key buffer holds (two poisoned buffers)
        assert not z.any()
        for poison in (-1, 0x5A5A5A5A):
            o2, h2, z2 = torch.empty_like(x), torch.empty_like(x), torch.full_like(x, float("nan"))
            _lib.call(name, x, eps, hist, *sizes, _cur(row[:6], STEP), table, torch.full((B, 2), poison, dtype=torch.int32,
                                                                                         device="cuda"), 0, o2, h2, z2)
            assert torch.equal(o2, out) and torch.equal(h2, h_out) and not z2.any()
    x3, h3 = x.clone(), hist.clone()                        # in place, as the captured step runs it
    _lib.call(name, x3, eps, h3, *sizes, _cur(row[:6], STEP), table, _words(keys), 0, x3, h3, None)
    assert torch.equal(x3, out) and torch.equal(h3, h_out)


@pytest.mark.parametrize("B,n", [(3, 128), (2, 4), (2, 1028)])
def test_keyed_diffuse_equals_float32_numpy(B, n):
    from lion_amd import _lib, diffusion_ops
    keys = KEYS[:B]
    x0 = torch.randn(B, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(19))
    keep = x0.clone()
    m, s = 0.8125, 0.58203125
    out, z = diffusion_ops.diffuse(x0, m, s, seeds=list(keys), return_noise=True)
    want = np.float32(m) * x0.cpu().numpy() + np.float32(s) * z.cpu().numpy()
    assert torch.equal(out, torch.from_numpy(want).cuda()) and torch.equal(x0, keep)
    for b, key in enumerate(keys):
        # today's lion_chain_diffuse on that one sample under seed = keys[b]: the same reserved word, the same stream
        o1, z1 = diffusion_ops.diffuse(x0[b].contiguous(), m, s, seed=key, return_noise=True)
        assert torch.equal(z[b], z1) and torch.equal(out[b], o1)
        assert torch.equal(z[b], _single(n, DIFFUSE, 1, key))
    o2 = torch.empty_like(x0)                               # without z_out; the words given directly
    _lib.call("lion_chain_diffuse_keyed", x0, B, n, m, s, _words(keys), 1, o2, None)
    assert torch.equal(o2, out)
    with pytest.raises(ValueError):
        diffusion_ops.diffuse(x0, m, s, seeds=list(keys), seed=3)
    with pytest.raises(ValueError):
        diffusion_ops.diffuse(x0, m, s, seeds=[1] * (B + 1))


# ---- the real priors --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_lion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.lion import LION
    torch.manual_seed(3)
    lion = LION(released_prior_cfg())
    lion.priors.eval()
    lion.vae.eval()
    return lion


def _priors(lion, B):
    sh = lion.vae.latent_shape()
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda", generator=g))
    return (lion.priors[0], sh[0], None), (lion.priors[1], sh[1], style)


def _tables(d):
    """mode -> the 4-5 rows a captured keyed step is checked on"""
    from lion_amd import chain
    return {chain.DDPM: d.ddpm_table(4),
            chain.DDIM: d.ddim_table(d.ddim_schedule(d._diffusion_steps, 4), 1.0),
            chain.SDE_DPMPP: d.dpm_solver_table(d.solver_schedule(5, "logsnr", 300), stochastic=True)}


# ---- 3. the captured keyed step equals the eager step -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 0, 3], ids=["ddpm", "ddim", "sde_dpmpp"])
def test_captured_keyed_step_equals_eager_step_on_the_priors(small_lion, mode):
    """after every replay ch.x == the by-value update of the eagerly evaluated prior on the keyed draw for that row: the flat
    keyed update behind the global prior, the channel-major one behind the local"""
    from lion_amd import chain, diffusion_ops
    lion, d = small_lion, small_lion.diffusion
    lion.priors.eval()
    B, keys = 2, [KA, KB]
    table = _tables(d)[mode]
    S = len(table)
    assert 4 <= S <= 5
    with torch.no_grad():
        for k, (prior, shape, cond) in enumerate(_priors(lion, B)):
            ch = chain.GraphedChain(prior, B, shape, cond, None, "cuda", mode, 16, record_noise=True, keyed=True)
            assert ch.keyed and ch.cm_out == (k == 1) and tuple(ch.seed.shape) == (B, 2)
            assert torch.isfinite(ch.x).all() and torch.isfinite(ch.z).all()       # the warm-up drew nothing harmful
            x0 = diffusion_ops.philox_normal_keyed(keys, B, shape, chain.START_STEP_WORD)
            ch.prepare(x0, table, keys, cond, None)
            assert torch.equal(ch.x, x0) and torch.equal(ch.seed, _words(keys))
            for i in range(S):
                x_i = ch.x.clone()
                h_i = None if ch.hist is None else ch.hist.clone()
                ch.replay()
                tt = torch.full((B,), float(table[i, 0]), device="cuda")
                eps = prior(x=x_i, t=tt, condition_input=cond, clip_feat=None).float().contiguous()
                z = diffusion_ops.philox_normal_keyed(keys, B, shape, i)
                r = [float(v) for v in table[i]]
                if mode == chain.DDPM:
                    want = diffusion_ops.ddpm_update(x_i, eps, z, r[6] != 0, r[1], r[2], r[3], r[4], r[5])
                elif mode == chain.DDIM:
                    want = diffusion_ops.ddim_update(x_i, eps, z, r[1], r[2], r[3])
                else:
                    noisy = r[7] != 0
                    want, want_h = diffusion_ops.sde_dpmpp_update(x_i, eps, h_i, *r[1:8], noise=z if noisy else None)
                    assert torch.equal(ch.hist, want_h), (k, i)
                    if not noisy:
                        z = torch.zeros_like(z)
                assert torch.equal(ch.x, want), (mode, k, i, (ch.x - want).abs().max().item())
                assert torch.equal(ch.z, z), (mode, k, i)
            assert torch.isfinite(ch.x).all()


# ---- 4. graph against eager through the samplers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "from_t", "dpm"])
def test_sampler_graph_equals_eager_under_seeds(small_lion, sampler):
    lion, d = small_lion, small_lion.diffusion
    B, seeds = 2, [KA, KB]
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    for prior, shape, cond in _priors(lion, B):
        start = d._keyed_start(seeds, B, shape)

        def run(graph):
            if sampler == "ddim":
                return d.run_ddim(prior, B, shape, ddim_step=4, kappa=1.0, condition_input=cond, seeds=seeds, graph=graph)[0]
            if sampler == "from_t":
                return d.run_denoising_diffusion_from_t(prior, B, shape, 4, start, condition_input=cond, seeds=seeds,
                                                        graph=graph)[0]
            return d.run_dpm_solver(prior, B, shape, steps=4, stochastic=True, condition_input=cond, seeds=seeds, graph=graph)[0]
        a, b, a2 = run(True), run(False), run(True)
        assert torch.isfinite(a).all() and torch.equal(a, b), (sampler, (a - b).abs().max().item())
        assert torch.equal(a, a2)
        other = seeds[::-1]
        if sampler == "from_t":
            c = d.run_denoising_diffusion_from_t(prior, B, shape, 4, start, condition_input=cond, seeds=other)[0]
        elif sampler == "ddim":
            c = d.run_ddim(prior, B, shape, ddim_step=4, kappa=1.0, condition_input=cond, seeds=other)[0]
        else:
            c = d.run_dpm_solver(prior, B, shape, steps=4, stochastic=True, condition_input=cond, seeds=other)[0]
        assert not torch.equal(a, c)
    assert any(ch.keyed for ch in d._chains._entries.values())
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])


# ---- 5. / 6. position and batchmates ----------------------------------------------------------------------------------------------
def _recorded(d, prior, shape, cond, seeds):
    """(start latent, [per-step noise], final latent) of a 4-step stochastic solver run under `seeds`, through chain.RECORD"""
    from lion_amd import chain
    chain.RECORD = rec = []
    try:
        out, _ = d.run_dpm_solver(prior, len(seeds), shape, steps=4, stochastic=True, condition_input=cond, seeds=list(seeds),
                                  keep_trajectory=False)
    finally:
        chain.RECORD = None
    assert len(rec) == 1 and len(rec[0][1]) == len(d.solver_schedule(4)) == 4
    return rec[0][0], rec[0][1], out


def test_noise_start_and_result_follow_the_sample_not_its_position(small_lion):
    """seeds (a, b, c) against (c, a, b) with the conditioning rows permuted alike: everything is the same rows, permuted.  Every
    operator of the denoisers works per cloud or per column, so the final latents are bit-equal too."""
    lion, d = small_lion, small_lion.diffusion
    perm = [2, 0, 1]
    for prior, shape, cond in _priors(lion, 3):
        s1, z1, o1 = _recorded(d, prior, shape, cond, (KA, KB, KC))
        s2, z2, o2 = _recorded(d, prior, shape, None if cond is None else cond[perm].contiguous(), (KC, KA, KB))
        assert torch.equal(s2, s1[perm]) and not torch.equal(s1[0], s1[1])
        for za, zb in zip(z1, z2):
            assert torch.equal(zb, za[perm])
        assert z1[0].any() and not z1[-1].any()             # the last row draws nothing
        assert torch.isfinite(o1).all() and torch.equal(o2, o1[perm]), (o2 - o1[perm]).abs().max().item()


def test_a_sample_does_not_depend_on_its_batchmates(small_lion):
    lion, d = small_lion, small_lion.diffusion
    for prior, shape, cond in _priors(lion, 2):
        s1, z1, o1 = _recorded(d, prior, shape, cond, (KA, KB))
        s2, z2, o2 = _recorded(d, prior, shape, cond, (KA, KC))
        assert torch.equal(s1[0], s2[0]) and not torch.equal(s1[1], s2[1])
        for za, zb in zip(z1[:-1], z2[:-1]):
            assert torch.equal(za[0], zb[0]) and not torch.equal(za[1], zb[1])
        assert torch.equal(o1[0], o2[0]), (o1[0] - o2[0]).abs().max().item()
        assert not torch.equal(o1[1], o2[1])


# ---- 7. applications ---------------------------------------------------------------------------------------------------------------
def test_generate_samples_and_lion_sample_take_seeds(small_lion):
    from lion_amd.chain import split_seed
    from lion_amd.sampling import SAMPLE_SUBKEYS, generate_samples_vada_2prior
    lion, d = small_lion, small_lion.diffusion
    sh = lion.vae.latent_shape()
    seeds = [KA, KB]
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    p1, i1 = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, 2, dpm_step=4, dpm_stochastic=True, seeds=seeds)
    p2, i2 = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, 2, dpm_step=4, dpm_stochastic=True,
                                          seeds=torch.tensor([KA - 2 ** 64 if KA >= 2 ** 63 else KA, KB]))
    p3, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, 2, dpm_step=4, dpm_stochastic=True, seeds=[KA, KC])
    assert tuple(p1.shape) == (2, 2048, 3) and torch.isfinite(p1).all() and torch.equal(p1, p2)
    assert torch.equal(p1[0], p3[0]) and not torch.equal(p1[1], p3[1])
    assert i1["seeds"] == i2["seeds"] and i1["seeds"]["seeds"] == seeds
    for j, name in enumerate(SAMPLE_SUBKEYS):
        assert i1["seeds"][name] == [split_seed(s, 4)[j] for s in seeds]
    o1 = lion.sample(num_samples=2, dpm_step=4, seeds=seeds)
    o2 = lion.sample(num_samples=2, dpm_step=4, seeds=seeds)
    assert torch.isfinite(o1["points"]).all() and torch.equal(o1["points"], o2["points"])
    assert torch.equal(o1["z_global"], o2["z_global"]) and torch.equal(o1["z_local"], o2["z_local"])
    assert o1["seeds"] == i1["seeds"]
    assert not torch.equal(o1["points"], p1)                # the deterministic solver from the same starts
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    with pytest.raises(ValueError):
        lion.sample(num_samples=2, dpm_step=4, seeds=[1])


def test_diffuse_denoise_variations_are_addressed_by_seed(small_lion):
    from lion_amd.chain import split_seed
    from lion_amd.editing import SUBKEYS, diffuse_denoise
    lion = small_lion
    g = torch.Generator(device="cuda").manual_seed(17)
    x0 = (torch.randn(1, 2048, 3, device="cuda", generator=g) * 0.5).expand(3, 2048, 3).contiguous()
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, ia = diffuse_denoise(lion.vae, lion.priors, lion.diffusion, x0, 200, solver_steps=3, seeds=(KA, KB, KC))
    b, ib = diffuse_denoise(lion.vae, lion.priors, lion.diffusion, x0, 200, solver_steps=3, seeds=(KD, KB, KE))
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    assert tuple(a.shape) == (3, 2048, 3) and torch.isfinite(a).all()
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]) and not torch.equal(a[0], a[2])
    assert torch.equal(a[1], b[1]), (a[1] - b[1]).abs().max().item()        # variation KB again, among other batchmates
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])
    for key in ("global_original", "global_edited", "local_original", "local_edited"):
        assert torch.equal(ia[key][1], ib[key][1]) and not torch.equal(ia[key][0], ib[key][0]), key
    assert ia["seeds"]["seeds"] == [KA, KB, KC]
    for j, name in enumerate(SUBKEYS):
        assert ia["seeds"][name] == [split_seed(s, 5)[j] for s in (KA, KB, KC)]


# ---- 8. world-size invariance at equal batch ---------------------------------------------------------------------------------------
def test_a_job_gives_the_same_shapes_however_it_is_sharded(small_lion):
    from lion_amd.sampling import generate_samples_vada_2prior, shape_seeds, shard_batch
    lion, d = small_lion, small_lion.diffusion
    sh = lion.vae.latent_shape()
    base, total = 20240229, 4

    def gen(seeds):
        return generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, len(seeds), dpm_step=3, seeds=seeds)[0]
    job = shape_seeds(base, 0, total)
    one = torch.cat([gen(job[0:2]), gen(job[2:4])])                         # one process, two calls of B = 2
    counts = [shard_batch(total, r, 2) for r in range(2)]
    assert counts == [2, 2]
    ranks = torch.cat([gen(shape_seeds(base, sum(counts[:r]), counts[r])) for r in range(2)])      # "two ranks"
    late, early = gen(shape_seeds(base, 2, 2)), gen(shape_seeds(base, 0, 2))                       # ... in reverse order
    assert torch.isfinite(one).all() and torch.equal(one, ranks) and torch.equal(one, torch.cat([early, late]))
    assert len({tuple(c.flatten()[:8].tolist()) for c in one}) == 4         # four different clouds
