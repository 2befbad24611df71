"""-m gpu: diffuse-denoise.  lion_chain_diffuse against float64 and its generator's properties; the tail of the ancestral
chain (run_denoising_diffusion_from_t) against the full chain, graphed against eager, on the capture the full chain made;
the two-latent recipe (lion_amd/editing.py) on the released configuration with a 12-step schedule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 12
B = 2
SEED = 0x1234567890ABCDEF
STEP_WORD = 0xFFFFFFFF


def _seed_words(seed):
    return torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32).view(np.int32)).cuda()


def _draw(numel, seed=SEED, stream_id=1, m=0.0, s=1.0, x0=None):
    """(out, z) of lion_chain_diffuse drawing its own noise"""
    from lion_amd import _lib
    x0 = torch.zeros(numel, device="cuda") if x0 is None else x0
    out, z = torch.empty_like(x0), torch.empty_like(x0)
    _lib.call("lion_chain_diffuse", x0, None, numel, m, s, _seed_words(seed), stream_id, out, z)
    return out, z


# ---- 1. kernel arithmetic -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numel", [1, 3, 4, 5, 255, 1027, 4 * 64 * 4 + 2])
def test_diffuse_kernel_against_float64(numel):
    """out vs float64 m*x0 + s*z on the z the kernel reported.  Bound: the kernel rounds each product and the sum once
    (or one product and the fused sum): |error| <= 2^-24 (|m x0| + |s z|) + 2^-24 |result| -- asserted with the looser
    2^-23 (|m x0| + |s z|) + ulp(result), every operand form: noise given / drawn, in place / out of place, pointers
    16-byte aligned / offset by 4 bytes."""
    from lion_amd import _lib
    m, s = np.float32(0.94371), np.float32(0.33079)
    g = torch.Generator(device="cuda").manual_seed(numel)
    sd = _seed_words(SEED)
    for given in (True, False):
        for in_place in (False, True):
            for off in (0, 1):
                x0 = torch.randn(numel + off, device="cuda", generator=g)[off:]
                z_in = torch.randn(numel + off, device="cuda", generator=g)[off:] if given else None
                z_out = torch.full((numel + off + 4,), 7.0, device="cuda")
                x0_before = x0.clone()
                out_buf = None if in_place else torch.full((numel + off + 4,), 7.0, device="cuda")
                out = x0 if in_place else out_buf[off:off + numel]
                _lib.call("lion_chain_diffuse", x0, z_in, numel, float(m), float(s), None if given else sd, 1, out,
                          z_out[off:off + numel])
                z = z_out[off:off + numel]
                assert torch.isfinite(z).all()
                if given:
                    assert torch.equal(z, z_in)
                a, b = float(m) * x0_before.double().cpu().numpy(), float(s) * z.double().cpu().numpy()
                want = a + b
                got = out.double().cpu().numpy()
                bound = 2.0 ** -23 * (np.abs(a) + np.abs(b)) + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
                err = np.abs(got - want)
                assert (err <= bound).all(), (given, in_place, off, float((err / bound).max()))
                # nothing outside [off, off + numel) was written
                assert (z_out[:off] == 7.0).all() and (z_out[off + numel:] == 7.0).all()
                if not in_place:
                    assert torch.equal(x0, x0_before)
                    assert (out_buf[:off] == 7.0).all() and (out_buf[off + numel:] == 7.0).all()


def test_diffuse_kernel_without_z_out():
    out, z = _draw(1027, m=0.5, s=0.25, x0=torch.ones(1027, device="cuda"))
    from lion_amd import _lib
    out2 = torch.empty_like(out)
    _lib.call("lion_chain_diffuse", torch.ones(1027, device="cuda"), None, 1027, 0.5, 0.25, _seed_words(SEED), 1, out2, None)
    assert torch.equal(out, out2)


# ---- 2. generator ---------------------------------------------------------------------------------------------------------
def test_draw_is_the_philox_stream_of_its_counter():
    """same seed and stream: same bits; the counter goes by element, so n draws are the prefix of 2n + 3; another seed or
    stream: other bits; and the values are the chain generator's at counter (element/4, the step word, stream)"""
    from test_chain_gpu import normals
    n = 1027
    _, z = _draw(n)
    assert torch.equal(z, _draw(n)[1])
    assert torch.equal(z, _draw(2 * n + 3)[1][:n])
    assert not torch.equal(z, _draw(n, seed=SEED + 1)[1])
    assert not torch.equal(z, _draw(n, stream_id=0)[1])
    ref = normals(n, STEP_WORD, 1, SEED)    # device logf / sincospif vs float64 libm, as for the chain's update
    np.testing.assert_allclose(z.cpu().numpy().astype(np.float64), ref, rtol=0, atol=2e-6)


def test_draw_differs_from_a_chain_steps_noise_under_the_same_seed():
    """the noise step 0 of a chain reports (z_out of lion_chain_update_noise, stream 0) against the forward draw under the
    same seed, on the stream the package uses (1) and on the chain's own (0: only the step word differs)"""
    from test_chain_gpu import _call_update
    n = 1 << 16
    x = torch.zeros(n, device="cuda")
    _, z_step = _call_update(0, x, x, (1.0, 1.0, 0.0, 1.0, 0, 0, 0), 0, SEED)
    for stream_id in (1, 0):
        _, z = _draw(n, stream_id=stream_id)
        same = int((z == z_step).sum())
        assert same < n / 1e4, (stream_id, same)


def test_draw_moments():
    n = 1 << 20
    _, z = _draw(n)
    z = z.double()
    mean, var = z.mean().item(), z.var(unbiased=False).item()
    assert abs(mean) < 5 / np.sqrt(n), mean
    assert abs(var - 1.0) < 5 * np.sqrt(2.0 / n), var


@pytest.fixture(scope="module")
def lion():
    """the released configuration on a 12-step schedule"""
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.lion import LION
    cfg = released_prior_cfg()
    cfg.ddpm.num_steps = T
    torch.manual_seed(3)
    model = LION(cfg)
    model.priors.eval()
    model.vae.eval()
    return model


def test_diffuse_of_a_constant(lion):
    d = lion.diffusion
    n, c, t = 1 << 20, 0.75, T - 1
    ab = d._h_alpha_bars[t]
    m, s = float(torch.sqrt(ab)), float(torch.sqrt(1.0 - ab))
    x0 = torch.full((n,), c, device="cuda")
    torch.manual_seed(1)
    a = d.diffuse(x0, t)
    assert abs(a.double().mean().item() - m * c) < s * 5 / np.sqrt(n)
    torch.manual_seed(1)                         # seed=None: torch.manual_seed governs the draw
    assert torch.equal(a, d.diffuse(x0, t))
    assert not torch.equal(a, d.diffuse(x0, t))
    b, z = d.diffuse(x0, t, seed=9, return_noise=True)
    assert torch.equal(b, d.diffuse(x0, t, noise=z))     # the given-noise path: the same arithmetic
    # the coefficients are those of iw_quantities_t + sample_q.  On the host's copy of the float32 schedule, where sqrt and
    # every product and sum are IEEE (one rounding each, no contraction between torch's separate operations): bit for bit
    x4 = torch.randn(2, 8, 1, 1, device="cuda")
    z4 = torch.randn(2, 8, 1, 1, device="cuda")
    got = d.diffuse(x4, t, noise=z4)
    ab4 = ab.expand(2)
    host = d.sample_q(x4.cpu(), z4.cpu(), (1.0 - ab4)[:, None, None, None], torch.sqrt(ab4)[:, None, None, None])
    assert torch.equal(got.cpu(), host)
    # and on the device's quantities, whose sqrt is the device library's (accurate to 1 ulp, not necessarily correctly rounded:
    # a relative 2^-23 per coefficient), with 2^-23 (|m x0| + |s z|) of rounding in each of the two evaluations: 3 * 2^-23 < 2^-21
    _, var_t, m_t, _, _, _ = d.iw_quantities_t(2, torch.full((2,), t, device="cuda"))
    dev = d.sample_q(x4, z4, var_t, m_t)
    bound = 2.0 ** -21 * ((m * x4.double()).abs() + (s * z4.double()).abs())
    assert ((got.double() - dev.double()).abs() <= bound).all(), float(((got.double() - dev.double()).abs() / bound).max())


# ---- 3-6. the tail of the chain -------------------------------------------------------------------------------------------
def _prior(lion, i):
    """(model, latent shape, condition_input) of prior i"""
    sh = lion.vae.latent_shape()
    if i == 0:
        return lion.priors[0], sh[0], None
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda", generator=g))
    return lion.priors[1], sh[1], style


@pytest.mark.parametrize("which", [0, 1])
def test_tail_equals_the_full_chain(lion, which):
    d = lion.diffusion
    model, shape, cond = _prior(lion, which)
    g = torch.Generator(device="cuda").manual_seed(5 + which)
    noise = (torch.randn([B] + shape, device="cuda", generator=g),
             [torch.randn([B] + shape, device="cuda", generator=g) for _ in range(T)])
    full, traj = d.run_denoising_diffusion(model, B, shape, condition_input=cond, given_noise=noise, graph=False)
    traj = traj['pred_x']
    assert len(traj) == T
    for k in (1, 2, T - 1, T):
        start = noise[0] if k == T else traj[T - 1 - k]          # the state after the step at t = k
        x, states = d.run_denoising_diffusion_from_t(model, B, shape, k, start.clone(), condition_input=cond,
                                                     given_noise=noise, graph=False)
        assert torch.equal(x, full), k
        assert len(states) == k and all(torch.equal(a, b) for a, b in zip(states, traj[T - k:])), k


@pytest.mark.parametrize("which", [0, 1])
def test_graphed_tail_equals_the_eager_tail_on_its_recorded_noise(lion, which):
    from lion_amd import chain
    d = lion.diffusion
    model, shape, cond = _prior(lion, which)
    k = 5
    start = torch.randn([B] + shape, device="cuda")
    chain.RECORD = []
    try:
        xg, sg = d.run_denoising_diffusion_from_t(model, B, shape, k, start, condition_input=cond)
        rec = list(chain.RECORD)
    finally:
        chain.RECORD = None
    assert len(rec) == 1 and len(rec[0][1]) == k and torch.equal(rec[0][0], start)
    by_t = [rec[0][1][k - 1 - t] for t in range(k)]               # step i of the tail is t = k - 1 - i
    xe, se = d.run_denoising_diffusion_from_t(model, B, shape, k, rec[0][0], condition_input=cond,
                                              given_noise=(None, by_t), graph=False)
    assert torch.equal(xg, xe), float((xg - xe).abs().max())
    assert len(sg) == len(se) == k and all(torch.equal(a, b) for a, b in zip(sg, se))
    assert torch.equal(sg[-1], sg[-2])        # the reference's quirk: the last entry repeats the state before the last update


@pytest.mark.parametrize("which", [0, 1])
def test_tail_replays_the_capture_of_the_full_chain(lion, which):
    d = lion.diffusion
    model, shape, cond = _prior(lion, which)
    d.run_denoising_diffusion(model, B, shape, condition_input=cond, keep_trajectory=False)     # captures, if nothing has
    entries = dict(d._chains._entries)
    graphs = {key: ch.graph for key, ch in entries.items()}
    x, _ = d.run_denoising_diffusion_from_t(model, B, shape, 3, torch.randn([B] + shape, device="cuda"),
                                            condition_input=cond)
    assert torch.isfinite(x).all()
    after = d._chains._entries
    assert set(after) == set(entries)
    assert all(after[key] is entries[key] and after[key].graph is graphs[key] for key in entries)
    # time_start = T from the full chain's start, under its seed: the full chain
    torch.manual_seed(7)
    full, traj = d.run_denoising_diffusion(model, B, shape, condition_input=cond)
    torch.manual_seed(7)
    start = torch.randn([B] + shape, device="cuda")
    x, states = d.run_denoising_diffusion_from_t(model, B, shape, T, start, condition_input=cond)
    assert torch.equal(x, full)
    assert len(states) == T and all(torch.equal(a, b) for a, b in zip(states, traj['pred_x']))
    assert set(d._chains._entries) == set(entries)


def test_time_start_zero_returns_its_input(lion):
    d = lion.diffusion
    model, shape, cond = _prior(lion, 0)
    start = torch.randn([B] + shape, device="cuda")
    keep = start.clone()
    x, states = d.run_denoising_diffusion_from_t(model, B, shape, 0, start)
    assert x is start and torch.equal(x, keep) and states == []


# ---- 7. the recipe --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    g = torch.Generator(device="cuda").manual_seed(17)
    return torch.randn(B, 2048, 3, device="cuda", generator=g) * 0.5


def _edit(lion, cloud, time_start, **kw):
    from lion_amd.editing import diffuse_denoise
    return diffuse_denoise(lion.vae, lion.priors, lion.diffusion, cloud, time_start, **kw)


def test_recipe_without_diffusion_is_the_vaes_reconstruction(lion, cloud):
    vae = lion.vae
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    points, info = _edit(lion, cloud, 0, seed=5)
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    gen = torch.Generator(device="cuda").manual_seed(info["seeds"]["vae"] & 0x7FFFFFFFFFFFFFFF)
    with torch.no_grad():
        dist = vae.encode_global(cloud)
        zg = dist.sample_given_rho(torch.randn(dist.mu.shape, device="cuda", generator=gen))
        style = vae.global2style(zg)
        dist = vae.encode_local(cloud, style)
        zl = dist.sample_given_rho(torch.randn(dist.mu.shape, device="cuda", generator=gen))
        want = vae.decoder(None, beta=None, context=zl, style=style)
    assert torch.equal(points, want)
    sh = vae.latent_shape()
    assert torch.equal(info["global_edited"], zg.view([B] + sh[0])) and torch.equal(info["local_edited"], zl.view([B] + sh[1]))
    assert torch.equal(info["global_edited"], info["global_original"])
    assert torch.equal(info["local_edited"], info["local_original"])


def test_recipe_is_governed_by_its_seed(lion, cloud):
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, ia = _edit(lion, cloud, (2, 3), seed=5)
    b, ib = _edit(lion, cloud, (2, 3), seed=5)
    c, ic = _edit(lion, cloud, (2, 3), seed=6)
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    assert a.shape == cloud.shape and torch.isfinite(a).all()
    assert torch.equal(a, b) and ia["seeds"] == ib["seeds"] and ia["time_start"] == (2, 3)
    assert not torch.equal(a, c) and ia["seeds"] != ic["seeds"]
    for key in ("global", "local"):
        assert not torch.equal(ia[key + "_edited"], ia[key + "_original"])
        assert ia[key + "_edited"].shape == ia[key + "_original"].shape
    # the local prior was conditioned on the EDITED global latent (style_mlp is '': global2style is the identity)
    assert torch.equal(ia["condition_input"], lion.vae.global2style(ia["global_edited"]))
    assert torch.equal(ia["condition_input"], ia["global_edited"])
    assert not torch.equal(ia["condition_input"], ia["global_original"])
    # seed=None: torch.manual_seed governs the call
    torch.manual_seed(3)
    e, _ = _edit(lion, cloud, (2, 3))
    torch.manual_seed(3)
    f, _ = _edit(lion, cloud, (2, 3))
    assert torch.equal(e, f) and not torch.equal(e, a)


def test_recipe_keep_first(lion, cloud):
    _, info = _edit(lion, cloud, (2, 3), seed=5, keep_first=True)
    for key in ("global", "local"):
        new, old = info[key + "_edited"], info[key + "_original"]
        assert torch.equal(new[0], old[0]) and not torch.equal(new[1], old[1])
