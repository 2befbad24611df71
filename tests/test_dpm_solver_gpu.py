"""-m gpu: the DPM-Solver++(2M) sampler.  The update kernel (lion_dpmpp_update, lion_chain_update_multistep[_cm]) against a
float32 numpy restatement, bit for bit; the whole chain on a toy denoiser whose ODE has a closed-form solution; the captured
step against the eager step on the real priors; and the existing samplers beside it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SECOND = (156.0, 0.99998, 0.97, 4.1e-4, 1.5, -0.5)      # a second-order row at a late step
FIRST = (156.0, 0.99998, 0.97, 4.1e-4, 1.0, 0.0)        # the first step / order 1
FINAL = (1.00005, 0.01, 0.0, 1.0, 1.0, 0.0)             # the last row: the data prediction
ROWS = {"second": SECOND, "first": FIRST, "final": FINAL}


def restate(x, eps, hist, row):
    """the kernel's four expressions on float32 numpy arrays: every operation rounds once"""
    a0, a1, a2, a3, a4, a5 = (np.float32(v) for v in row)
    x0 = a0 * (x - a1 * eps)
    D = a4 * x0 if a5 == 0 else a4 * x0 + a5 * hist
    return a2 * x + a3 * D, x0


def _inputs(numel, seed=0):
    rng = np.random.default_rng(1000 * seed + numel)
    return tuple(rng.standard_normal(numel).astype(np.float32) for _ in range(3))


def _cur(row):
    return torch.tensor([418.0] + list(row) + [0.0], dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("numel", [1, 3, 4, 5, 255, 1027, 32 * 128])
@pytest.mark.parametrize("kind", list(ROWS))
def test_update_kernel_equals_float32_numpy(kind, numel):
    from lion_amd import _lib
    from lion_amd.diffusion_ops import dpmpp_update
    row = ROWS[kind]
    x, e, h = _inputs(numel)
    if row[5] == 0:
        h = np.full(numel, np.nan, np.float32)             # a5 == 0: hist is not read
    want_out, want_hist = restate(x, e, h, row)
    assert np.isfinite(want_out).all() and np.isfinite(want_hist).all()
    dx, de, dh = (torch.from_numpy(a).cuda() for a in (x, e, h))
    want_out, want_hist = torch.from_numpy(want_out).cuda(), torch.from_numpy(want_hist).cuda()
    out, hist_out = dpmpp_update(dx, de, dh, *row)
    assert torch.isfinite(out).all() and torch.isfinite(hist_out).all()
    assert torch.equal(out, want_out) and torch.equal(hist_out, want_hist)
    assert torch.equal(dx, torch.from_numpy(x).cuda()) and torch.equal(de, torch.from_numpy(e).cuda())   # inputs untouched
    if row[5] == 0:                                         # ... and hist may then be absent altogether
        o2, h2 = dpmpp_update(dx, de, None, *row)
        assert torch.equal(o2, want_out) and torch.equal(h2, want_hist)
    else:
        with pytest.raises(ValueError):
            dpmpp_update(dx, de, None, *row)
    # in place: out is x and hist_out is hist
    x2, h2 = dx.clone(), dh.clone()
    r = dpmpp_update(x2, de, h2, *row, out=x2, hist_out=h2)
    assert r[0] is x2 and r[1] is h2
    assert torch.equal(x2, want_out) and torch.equal(h2, want_hist)
    # the captured step's form: the same coefficients read from cur[1..6], out of place and in place
    o3, h3 = torch.empty_like(dx), torch.empty_like(dx)
    _lib.call("lion_chain_update_multistep", dx, de, dh, numel, _cur(row), o3, h3)
    assert torch.equal(o3, out) and torch.equal(h3, hist_out)
    x4, h4 = dx.clone(), dh.clone()
    _lib.call("lion_chain_update_multistep", x4, de, h4, numel, _cur(row), x4, h4)
    assert torch.equal(x4, out) and torch.equal(h4, hist_out)


@pytest.mark.parametrize("B,N", [(1, 1), (2, 3), (3, 64), (2, 257)])
@pytest.mark.parametrize("kind", list(ROWS))
def test_channel_major_form_equals_the_flat_form(kind, B, N):
    from lion_amd import _lib
    row = ROWS[kind]
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + N)
    x = torch.randn(B, N, 4, device="cuda", generator=g)
    hist = torch.randn(B, N, 4, device="cuda", generator=g)
    if row[5] == 0:
        hist.fill_(float("nan"))
    eps_cm = torch.randn(B, 4, N, device="cuda", generator=g)
    cur = _cur(row)
    o1, h1 = torch.empty_like(x), torch.empty_like(x)
    _lib.call("lion_chain_update_multistep", x, eps_cm.permute(0, 2, 1).contiguous(), hist, x.numel(), cur, o1, h1)
    o2, h2 = torch.empty_like(x), torch.empty_like(x)
    _lib.call("lion_chain_update_multistep_cm", x, eps_cm, hist, B, N, cur, o2, h2)
    assert torch.isfinite(o1).all() and torch.equal(o1, o2) and torch.equal(h1, h2)
    x3, h3 = x.clone(), hist.clone()                       # in place, as the captured step runs it
    _lib.call("lion_chain_update_multistep_cm", x3, eps_cm, h3, B, N, cur, x3, h3)
    assert torch.equal(x3, o1) and torch.equal(h3, h1)


# ---- whole chain on a toy denoiser -------------------------------------------------------------------------------------------
def _diffusion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.diffusion import DiffusionDiscretized
    return DiffusionDiscretized(None, None, released_prior_cfg(), device="cuda")


class ToyDenoiser(torch.nn.Module):
    """the exact denoiser of data ~ N(0, s^2): eps = x * sigma_t / v_t, one float32 product per element"""

    def __init__(self, g):
        super().__init__()
        self.register_buffer("g", g)

    def forward(self, x, t, condition_input=None, clip_feat=None, **kwargs):
        return x * self.g[t.long() - 1].view(-1, *([1] * (x.dim() - 1)))


def test_whole_chain_on_a_toy_denoiser():
    """graph == float32 numpy loop over the same table == eager loop, bit for bit; the error against the closed form is at
    most a third of DDIM's on the same indices (the CPU suite's condition, here on float32 chains); a second call captures
    nothing."""
    d = _diffusion()
    s, B, S = 0.5, 2, 20
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    v = ab * s * s + 1.0 - ab
    g = (np.sqrt(1.0 - ab) / v).astype(np.float32)
    toy = ToyDenoiser(torch.from_numpy(g)).cuda()
    x_start = np.random.default_rng(5).standard_normal((B, 128, 1, 1)).astype(np.float32)
    xs = torch.from_numpy(x_start).cuda()
    a, traj = d.run_dpm_solver(toy, B, [128, 1, 1], steps=S, x_noisy=xs, graph=True)
    n_entries = len(d._chains._entries)
    entry = list(d._chains._entries.values())[-1]
    assert n_entries == 1 and entry.mode == 2 and entry.hist is not None
    steps = d.solver_schedule(S)
    table = d.dpm_solver_table(steps)
    assert len(traj) == len(steps) == S and torch.equal(traj[-1], a)
    x, hist = x_start.copy(), np.zeros_like(x_start)
    for i, t in enumerate(steps):
        x, hist = restate(x, x * g[t], hist, table[i, 1:7])
        assert np.array_equal(traj[i].cpu().numpy(), x), i
    b, _ = d.run_dpm_solver(toy, B, [128, 1, 1], steps=S, x_noisy=xs, graph=False)
    assert torch.equal(a, b)
    assert torch.equal(xs, torch.from_numpy(x_start).cuda())        # the caller's start is not written
    a2, _ = d.run_dpm_solver(toy, B, [128, 1, 1], steps=S, x_noisy=xs, graph=True, keep_trajectory=False)
    assert torch.equal(a2, a)
    assert len(d._chains._entries) == n_entries and list(d._chains._entries.values())[-1] is entry
    # accuracy: the ODE is linear, x / sqrt(v) constant along it, then the data prediction at index 0
    x0 = np.sqrt(v[0] / v[-1])
    exact = (x0 - np.sqrt(1 - ab[0]) * (np.sqrt(1 - ab[0]) * x0 / v[0])) / np.sqrt(ab[0]) * x_start.astype(np.float64)
    xd = x_start.copy()
    for i, t in enumerate(steps):                                     # DDIM, kappa = 0, float32, the same indices
        sc, c, sigma = d.ddim_coefficients(t, None if i == len(steps) - 1 else steps[i + 1], 0.0)
        xd = xd * np.float32(sc) + np.float32(c) * (xd * g[t])
    err = lambda y: np.linalg.norm(y.astype(np.float64) - exact) / np.linalg.norm(exact)
    e2, e1 = err(a.cpu().numpy()), err(xd)
    print(f"toy s={s} S={S}: DDIM {e1:.3e}  2M {e2:.3e}  ratio {e1 / e2:.2f}")
    assert e2 <= e1 / 3.0, (e1, e2)


# ---- the real priors ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_lion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.lion import LION
    torch.manual_seed(3)
    lion = LION(released_prior_cfg())
    lion.priors.eval()
    lion.vae.eval()
    return lion


def test_captured_step_equals_eager_step_on_the_priors(small_lion):
    """Every replay of the captured step leaves x and hist == lion_dpmpp_update(x_i, prior(x_i, t_i), hist_i, row_i) evaluated
    eagerly on the graph's own previous state: the flat update behind the global prior, the channel-major one behind the local."""
    from lion_amd import chain, diffusion_ops
    lion, d = small_lion, small_lion.diffusion
    lion.priors.eval()
    B, S = 2, 5
    sh = lion.vae.latent_shape()
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda"))
        for k, (prior, shape, cond) in enumerate(((lion.priors[0], sh[0], None), (lion.priors[1], sh[1], style))):
            steps = d.solver_schedule(S)
            table = d.dpm_solver_table(steps)
            assert len(steps) == S and np.all(table[1:-1, 6] != 0)
            ch = chain.GraphedChain(prior, B, shape, cond, None, "cuda", chain.DPMPP, 16)
            assert ch.cm_out == (k == 1)
            x0 = torch.randn([B] + shape, device="cuda")
            ch.prepare(x0, table, 0, cond, None)
            assert torch.equal(ch.x, x0) and not ch.hist.any()
            for i in range(S):
                x_i, h_i = ch.x.clone(), ch.hist.clone()
                ch.replay()
                tt = torch.full((B,), float(table[i, 0]), device="cuda")
                eps = prior(x=x_i, t=tt, condition_input=cond, clip_feat=None).float().contiguous()
                want_x, want_h = diffusion_ops.dpmpp_update(x_i, eps, h_i, *[float(v) for v in table[i, 1:7]])
                assert torch.equal(ch.x, want_x), (k, i, (ch.x - want_x).abs().max().item() / want_x.abs().max().item())
                assert torch.equal(ch.hist, want_h), (k, i)
            assert torch.isfinite(ch.x).all()


def test_sampler_graph_equals_eager_on_the_priors(small_lion):
    lion, d = small_lion, small_lion.diffusion
    B, S = 2, 5
    sh = lion.vae.latent_shape()
    style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda"))
    for prior, shape, cond in ((lion.priors[0], sh[0], None), (lion.priors[1], sh[1], style)):
        x0 = torch.randn([B] + shape, device="cuda")
        a, tr = d.run_dpm_solver(prior, B, shape, steps=S, x_noisy=x0, condition_input=cond, graph=True)
        b, tr_b = d.run_dpm_solver(prior, B, shape, steps=S, x_noisy=x0, condition_input=cond, graph=False)
        assert len(tr) == len(tr_b) == S and torch.equal(tr[-1], a)
        assert torch.equal(a, b), (a - b).abs().max().item() / b.abs().max().item()
        assert torch.isfinite(a).all() and not torch.equal(a, x0)
        assert prior.training                               # as run_ddim leaves it
        # order 1 through the same kernel is another chain
        c, _ = d.run_dpm_solver(prior, B, shape, steps=S, order=1, x_noisy=x0, condition_input=cond, keep_trajectory=False)
        assert torch.isfinite(c).all() and not torch.equal(a, c)


def test_state_hook_graph_equals_eager(small_lion):
    """a hook that overwrites half of the latent before every evaluation: the same result in both paths, called once per step"""
    lion, d = small_lion, small_lion.diffusion
    B, S = 2, 4
    sh = lion.vae.latent_shape()
    style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda"))
    x0 = torch.randn([B] + sh[1], device="cuda")
    n = x0[0].numel()
    forced = [torch.randn(B, n // 2, device="cuda") for _ in range(S)]
    outs = {}
    for graph in (True, False):
        seen = []

        def hook(i, x):
            seen.append(i)
            x.view(B, -1)[:, :n // 2].copy_(forced[i])
        outs[graph], _ = d.run_dpm_solver(lion.priors[1], B, sh[1], steps=S, x_noisy=x0, condition_input=style, graph=graph,
                                          state_hook=hook, keep_trajectory=False)
        assert seen == list(range(S))
    plain, _ = d.run_dpm_solver(lion.priors[1], B, sh[1], steps=S, x_noisy=x0, condition_input=style, keep_trajectory=False)
    assert torch.equal(outs[True], outs[False])
    assert not torch.equal(outs[True], plain)


def test_nothing_existing_moves(small_lion):
    """DDIM before and after a solver run on the same DiffusionDiscretized and model: the same bits, its capture kept; the
    two-prior driver and LION.sample with dpm_step; dpm_step = 0 is the call without the argument."""
    from lion_amd import chain
    from lion_amd.sampling import generate_samples_vada_2prior
    lion, d = small_lion, _diffusion()
    B = 2
    sh = lion.vae.latent_shape()
    prior = lion.priors[0]
    x0 = torch.randn([B] + sh[0], device="cuda")
    ddim = lambda: d.run_ddim(prior, B, sh[0], ddim_step=4, kappa=0.0, x_noisy=x0, is_image=False)[0]
    before = ddim()
    entries = dict(d._chains._entries)
    assert len(entries) == 1
    s1, _ = d.run_dpm_solver(prior, B, sh[0], steps=6, x_noisy=x0)
    after = dict(d._chains._entries)
    assert len(after) == 2 and all(after[k] is v for k, v in entries.items())       # one entry added, none replaced
    new = [v for k, v in after.items() if k not in entries]
    assert len(new) == 1 and new[0].mode == chain.DPMPP
    assert torch.equal(ddim(), before)
    assert dict(d._chains._entries) == after
    assert torch.isfinite(s1).all() and not torch.equal(s1, before)
    # the two-prior driver
    torch.manual_seed(11)
    p1, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, dpm_step=6)
    torch.manual_seed(11)
    p2, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, dpm_step=6)
    assert tuple(p1.shape) == (B, 2048, 3) and torch.isfinite(p1).all() and torch.equal(p1, p2)
    torch.manual_seed(11)
    q0, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, ddim_step=3)
    torch.manual_seed(11)
    q1, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, ddim_step=3, dpm_step=0)
    torch.manual_seed(11)
    q2, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, ddim_step=3, dpm_step=6)    # the solver goes first
    assert torch.equal(q0, q1) and torch.equal(q2, p1) and not torch.equal(q0, p1)
    out = lion.sample(num_samples=2, dpm_step=6)
    assert tuple(out['points'].shape) == (2, 2048, 3) and torch.isfinite(out['points']).all()
    assert tuple(out['z_global'].shape)[0] == 2 and torch.isfinite(out['z_local']).all()
