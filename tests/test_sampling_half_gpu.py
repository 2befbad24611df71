"""-m gpu: conv_precision="half" through the samplers -- the reduced-precision mode runs INSIDE the captured chain, on the
library's own kernels (LION_STRICT for the whole module: no vendor-library fallback is taken), a chain captured under one
precision is never replayed under the other, and the VAE decode stays fp32-accurate."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 2, 4


@pytest.fixture(scope="module", autouse=True)
def strict_module():
    from lion_amd import _fallback
    was = _fallback.strict()
    _fallback.reset()
    _fallback.strict(True)
    yield
    _fallback.strict(was)
    assert _fallback.counts() == {}, _fallback.counts()


@pytest.fixture(scope="module")
def setup():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.lion import LION
    torch.manual_seed(3)
    lion = LION(released_prior_cfg())
    lion.priors.eval()
    lion.vae.eval()
    sh = lion.vae.latent_shape()
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda"))
    x0 = torch.randn([B] + sh[1], device="cuda")
    return lion, sh, style, x0


def _ddim(d, lion, sh, style, x0, **kw):
    return d.run_ddim(lion.priors[1], B, sh[1], ddim_step=S, condition_input=style, x_noisy=x0.clone(), is_image=False,
                      keep_trajectory=False, **kw)[0]


def test_half_graphed_chain_equals_the_eager_loop_on_recorded_noise(setup):
    from lion_amd import chain
    lion, sh, style, x0 = setup
    chain.RECORD = []
    try:
        torch.manual_seed(5)
        g = _ddim(lion.diffusion, lion, sh, style, x0, conv_precision="half")
        rec = list(chain.RECORD)
    finally:
        chain.RECORD = None
    assert len(rec) == 1 and len(rec[0][1]) == S
    e = _ddim(lion.diffusion, lion, sh, style, x0, graph=False, given_noise=rec[0], conv_precision="half")
    assert torch.equal(g, e), float((g - e).abs().max())


def test_precision_change_recaptures_and_fp32_is_untouched(setup):
    """half, then fp32 on the same sampler object: the fp32 result is bit-identical to a sampler that never saw half mode;
    the half latent is finite and differs (the mode is on).  Its drift after the 4 steps is printed, not asserted: no bound
    for a free-running chain can be derived."""
    from lion_amd import chain, conv_ops
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    lion, sh, style, x0 = setup
    fresh = DiffusionDiscretized(None, None, released_prior_cfg(), device="cuda")
    ref = _ddim(fresh, lion, sh, style, x0, kappa=0.0)

    captured = []
    real_init = chain.GraphedChain.__init__

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        captured.append(self.policy[-1])
    chain.GraphedChain.__init__ = spy
    try:
        d = lion.diffusion
        h = _ddim(d, lion, sh, style, x0, kappa=0.0, conv_precision="half")
        h2 = _ddim(d, lion, sh, style, x0, kappa=0.0, conv_precision="half")
        f = _ddim(d, lion, sh, style, x0, kappa=0.0)
    finally:
        chain.GraphedChain.__init__ = real_init
    assert conv_ops.PRECISION == "fp32"
    assert captured[-1] == "fp32" and "half" in captured and len(captured) <= 2, captured
    assert torch.equal(f, ref)
    assert torch.equal(h, h2)
    assert torch.isfinite(h).all() and not torch.equal(h, ref)
    drift = (h - ref).abs().max().item() / ref.abs().max().item()
    rms = ((h - ref).square().mean().sqrt() / ref.square().mean().sqrt()).item()
    print(f"half vs fp32 latent after {S} DDIM steps (B={B}): max |d| / max = {drift:.3e}, rms(d) / rms = {rms:.3e}")


def test_decode_stays_fp32(setup):
    """generate_samples_vada_2prior(conv_precision="half"): the decode runs under the fp32 setting and equals an fp32
    decode of the same latent bit for bit"""
    from lion_amd import conv_ops
    from lion_amd.sampling import generate_samples_vada_2prior
    lion, sh, _, _ = setup
    seen = {}
    real = lion.vae.sample

    def spy(num_samples=10, decomposed_eps=(), **k):
        seen["precision"] = conv_ops.PRECISION
        seen["eps"] = [e.clone() for e in decomposed_eps]
        return real(num_samples=num_samples, decomposed_eps=decomposed_eps, **k)
    lion.vae.sample = spy
    try:
        torch.manual_seed(9)
        pts, _ = generate_samples_vada_2prior(sh, lion.priors, lion.diffusion, lion.vae, B, ddim_step=S, conv_precision="half")
    finally:
        del lion.vae.sample
    assert seen["precision"] == "fp32"
    with torch.no_grad():
        again = lion.vae.sample(num_samples=B, decomposed_eps=seen["eps"])
    assert torch.equal(pts, again) and torch.isfinite(pts).all()
    torch.manual_seed(9)
    pts32, _ = generate_samples_vada_2prior(sh, lion.priors, lion.diffusion, lion.vae, B, ddim_step=S)
    assert not torch.equal(pts, pts32)
