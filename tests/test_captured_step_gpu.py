"""-m gpu: lion_amd/chain.py::CapturedStep on its own (a toy step, no denoiser and no schedule), and the two drivers that
moved onto it: graph.GraphedDenoiser captures again when its weights changed, ode.OdeGraph owns its buffers."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(0.5, 1.5, 8))


def _toy():
    from lion_amd import chain
    m = Toy().cuda()
    x = torch.zeros(2, 8, device="cuda")

    def step():
        x.mul_(m.w).add_(1)
    return m, x, chain.CapturedStep(m, step, x)


def test_toy_step_replays_equal_eager_applications():
    m, x, cs = _toy()
    assert cs.graph_b is None and cs.geo_graphs is None
    start = torch.randn(2, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    x.copy_(start)
    for _ in range(3):
        cs.replay()
    want = start.clone()
    with torch.no_grad():
        for _ in range(3):
            want.mul_(m.w).add_(1)
    assert torch.equal(x, want)


def test_toy_step_validity():
    from lion_amd import _wcache, conv_ops
    m, x, cs = _toy()
    assert cs.valid()
    with conv_ops.conv_precision("half"):      # a kernel-selecting switch: the policy the graph was captured under is gone
        assert not cs.valid()
    assert cs.valid()
    with torch.no_grad():
        m.w.mul_(2)
    assert not cs.valid()
    m, x, cs = _toy()
    assert cs.valid()
    _wcache.invalidate_all()
    assert not cs.valid()


def _lion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.lion import LION
    torch.manual_seed(5)
    lion = LION(released_prior_cfg())
    lion.priors.eval()
    return lion


def test_graphed_denoiser_recaptures_after_a_weight_change():
    """a graph captured before the weights changed is never replayed: the next call captures again and matches the eager
    forward of the NEW weights (the bound of test_models_gpu.py::test_graph_replay_equals_eager_denoisers)"""
    from lion_amd.graph import GraphedDenoiser
    lion = _lion()
    sh = lion.vae.latent_shape()
    B = 2
    zg = [torch.randn([B] + sh[0], device="cuda") for _ in range(2)]
    zl = [torch.randn([B] + sh[1], device="cuda") for _ in range(2)]
    ts = [torch.full((B,), v, device="cuda") for v in (999.0, 500.0)]
    with torch.no_grad():
        style = lion.vae.global2style(zg[0])
        for prior, zs, cond in ((lion.priors[0], zg, None), (lion.priors[1], zl, style)):
            graphed = GraphedDenoiser(prior, zs[0], ts[0], condition_input=cond)
            first = graphed.step
            assert first.geo_graphs is None and first.graph_b is None    # one graph on one stream, as before
            if prior is lion.priors[1]:
                assert first.pinned, "the graph holds no reference to the packed weights it points at"
            for p in prior.parameters():
                p.mul_(1.01)
            assert not first.valid()
            want = prior(x=zs[1], t=ts[1], condition_input=cond, clip_feat=None).float()
            got = graphed(x=zs[1], t=ts[1], condition_input=cond, clip_feat=None).float()
            assert graphed.step is not first and graphed.step.valid()
            err = (got - want).abs().max().item() / want.abs().max().item()
            assert err <= 1e-6, err


def test_ode_graph_owns_its_buffers():
    from lion_amd import ode
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion_continuous import make_diffusion
    lion = _lion()
    diff = make_diffusion(released_prior_cfg().sde, device="cuda")
    shape = lion.vae.latent_shape()[0]
    try:
        g = ode.graph_for(lion.priors[0], 2, shape, None, None, torch.device("cuda"), diff.ode_scalars())
        assert g.state.x32.data_ptr() == g.x.data_ptr() and g.state.t_model is g.t
        assert tuple(g.x.shape) == (2,) + tuple(shape) and g.cond is None and g.clip is None
        assert not hasattr(g, "chain")
        assert not any(hasattr(g, name) for name in ("table", "counter", "seed"))
        assert g.step.valid() and g.matches(None, None, diff.ode_scalars())
    finally:
        ode.clear_graphs()
