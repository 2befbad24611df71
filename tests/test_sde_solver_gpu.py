"""-m gpu: the stochastic few-step solver SDE-DPM-Solver++(2M).  The update kernel (lion_sde_dpmpp_update,
lion_chain_update_multistep_noise[_cm]) against a float32 numpy restatement on the noise it reports, bit for bit, and that noise
against lion_chain_update_noise's; the whole chain on a toy denoiser against the float64 covariance recursion; the captured
step against the eager step on the real priors; tails from an intermediate index; diffuse_denoise and the samplers on it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
#        a0       a1       a2    a3      a4   a5    a6
ROWS = {"first": (156.0, 0.99998, 0.93, 8.1e-4, 1.0, 0.0, 0.31),       # the first step / order 1: hist is not read
        "second": (156.0, 0.99998, 0.93, 8.1e-4, 1.5, -0.5, 0.31),     # a second-order row at a late step
        "final": (1.00005, 0.01, 0.0, 1.0, 1.0, 0.0, 0.0),             # the last row: the data prediction, nothing drawn
        "identity": (1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)}               # the chain's warm-up row: out = x
STEP = 5                                                                # the row's index in the table = its counter word


def restate(x, eps, hist, z, row):
    """the kernel's expressions on float32 numpy arrays: every operation rounds once"""
    a0, a1, a2, a3, a4, a5, a6 = (np.float32(v) for v in row)
    x0 = a0 * (x - a1 * eps)
    D = a4 * x0 if a5 == 0 else a4 * x0 + a5 * hist
    out = a2 * x + a3 * D
    return (out + a6 * z if a6 != 0 else out), x0


def _inputs(numel, seed=0):
    rng = np.random.default_rng(1000 * seed + numel)
    return tuple(rng.standard_normal(numel).astype(np.float32) for _ in range(3))


def _seed_words(seed=SEED):
    return torch.from_numpy(np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32).view(np.int32)).cuda()


def _cur_table(row, step=STEP):
    """cur as lion_chain_begin_step leaves it for row `step` of a table whose column 7 holds a6"""
    table = torch.zeros(step + 2, 8, device="cuda")
    table[step] = torch.tensor([418.0] + list(row), device="cuda")
    cur = table[step].clone()
    cur.view(torch.int32)[7] = step
    return cur, table


def _chain_noise(numel, step, stream_id, seed=SEED):
    """the z lion_chain_update_noise draws for (seed, step, stream_id)"""
    from lion_amd import _lib
    x = torch.zeros(numel, device="cuda")
    cur = torch.zeros(8, device="cuda")
    cur[1] = 1.0
    cur.view(torch.int32)[7] = step
    out, z = torch.empty_like(x), torch.empty_like(x)
    _lib.call("lion_chain_update_noise", 0, x, x, numel, cur, _seed_words(seed), stream_id, out, z)
    return z


@pytest.mark.parametrize("numel", [1, 3, 4, 5, 255, 1027, 32 * 128])
@pytest.mark.parametrize("kind", list(ROWS))
def test_update_kernel_equals_float32_numpy(kind, numel):
    from lion_amd import _lib
    from lion_amd.diffusion_ops import sde_dpmpp_update
    row = ROWS[kind]
    noisy = row[6] != 0
    x, e, h = _inputs(numel)
    if row[5] == 0:
        h = np.full(numel, np.nan, np.float32)             # a5 == 0: hist is not read
    dx, de, dh = (torch.from_numpy(a).cuda() for a in (x, e, h))
    words = _seed_words()
    # the by-value entry point, noise drawn in the kernel: the restatement runs on the z it reports
    out, hist_out, z = sde_dpmpp_update(dx, de, dh, *row, seed=words, step=STEP, stream_id=0, return_noise=True)
    want_out, want_hist = restate(x, e, h, z.cpu().numpy(), row)
    assert np.isfinite(want_out).all() and np.isfinite(want_hist).all()
    want_out, want_hist = torch.from_numpy(want_out).cuda(), torch.from_numpy(want_hist).cuda()
    assert torch.equal(out, want_out) and torch.equal(hist_out, want_hist)
    assert torch.equal(dx, torch.from_numpy(x).cuda()) and torch.equal(de, torch.from_numpy(e).cuda())   # inputs untouched
    # that z is the chain generator's for (seed, step, stream 0); a row that draws nothing reports zeros
    if noisy:
        assert torch.equal(z, _chain_noise(numel, STEP, 0)) and torch.isfinite(z).all() and z.any()
        assert not torch.equal(z, _chain_noise(numel, STEP + 1, 0)) and not torch.equal(z, _chain_noise(numel, STEP, 1))
    else:
        assert not z.any()
        o2, h2 = sde_dpmpp_update(dx, de, dh, *row)        # ... and needs neither noise nor seed
        assert torch.equal(o2, want_out) and torch.equal(h2, want_hist)
    assert torch.equal(sde_dpmpp_update(dx, de, dh, *row, seed=SEED, step=STEP)[0], want_out)      # the seed as an int
    # given noise: the same function of that z
    o3, h3, z3 = sde_dpmpp_update(dx, de, dh, *row, noise=z, return_noise=True)
    assert torch.equal(o3, want_out) and torch.equal(h3, want_hist) and torch.equal(z3, z)
    zn = torch.from_numpy(_inputs(numel, 7)[0]).cuda()
    o4, _, z4 = sde_dpmpp_update(dx, de, dh, *row, noise=zn, return_noise=True)
    assert torch.equal(o4, torch.from_numpy(restate(x, e, h, zn.cpu().numpy(), row)[0]).cuda())
    assert torch.equal(z4, zn if noisy else torch.zeros_like(zn))
    if row[5] == 0:                                         # hist may then be absent altogether
        assert torch.equal(sde_dpmpp_update(dx, de, None, *row, seed=words, step=STEP)[0], want_out)
    else:
        with pytest.raises(ValueError):
            sde_dpmpp_update(dx, de, None, *row, seed=words, step=STEP)
    if noisy:
        with pytest.raises(ValueError):
            sde_dpmpp_update(dx, de, dh, *row)
    # in place: out is x and hist_out is hist
    x2, h2 = dx.clone(), dh.clone()
    r = sde_dpmpp_update(x2, de, h2, *row, seed=words, step=STEP, out=x2, hist_out=h2)
    assert r[0] is x2 and r[1] is h2 and torch.equal(x2, want_out) and torch.equal(h2, want_hist)
    # the captured step's form: a0..a5 and the step index from cur, a6 from the table, out of place and in place
    cur, table = _cur_table(row)
    o5, h5, z5 = torch.empty_like(dx), torch.empty_like(dx), torch.full_like(dx, float("nan"))
    _lib.call("lion_chain_update_multistep_noise", dx, de, dh, numel, cur, table, words, 0, o5, h5, z5)
    assert torch.equal(o5, want_out) and torch.equal(h5, want_hist) and torch.equal(z5, z)
    x6, h6 = dx.clone(), dh.clone()
    _lib.call("lion_chain_update_multistep_noise", x6, de, h6, numel, cur, table, words, 0, x6, h6, None)
    assert torch.equal(x6, want_out) and torch.equal(h6, want_hist)


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
    cur, table = _cur_table(row)
    words = _seed_words()
    o1, h1, z1 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    _lib.call("lion_chain_update_multistep_noise", x, eps_cm.permute(0, 2, 1).contiguous(), hist, x.numel(), cur, table, words,
              0, o1, h1, z1)
    o2, h2, z2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    _lib.call("lion_chain_update_multistep_noise_cm", x, eps_cm, hist, B, N, cur, table, words, 0, o2, h2, z2)
    assert torch.isfinite(o1).all() and torch.equal(o1, o2) and torch.equal(h1, h2) and torch.equal(z1, z2)
    assert z1.any() == (row[6] != 0)
    x3, h3 = x.clone(), hist.clone()                       # in place, as the captured step runs it
    _lib.call("lion_chain_update_multistep_noise_cm", x3, eps_cm, h3, B, N, cur, table, words, 0, x3, h3, None)
    assert torch.equal(x3, o1) and torch.equal(h3, h1)


def test_bad_arguments_are_refused_before_any_launch():
    """argument checks only: every pointer handed over is a live buffer of 64 floats (or NULL), nothing is dereferenced"""
    from lion_amd import _lib
    a = [torch.full((64,), 2.0, device="cuda") for _ in range(6)]
    x, e, h, o, ho, z = a
    cur, table = _cur_table(ROWS["second"])
    words = _seed_words()
    co = ROWS["second"]

    def refused(name, *args):
        with pytest.raises(RuntimeError, match="LION_EINVAL"):
            _lib.call(name, *args)
    refused("lion_sde_dpmpp_update", None, e, h, None, 64, *co, words, 0, 0, o, ho, None)
    refused("lion_sde_dpmpp_update", x, e, None, None, 64, *co, words, 0, 0, o, ho, None)        # a5 != 0
    refused("lion_sde_dpmpp_update", x, e, h, None, 64, *co, None, 0, 0, o, ho, None)            # a6 != 0: z_in or seed
    refused("lion_sde_dpmpp_update", x, e, h, None, 0, *co, words, 0, 0, o, ho, None)
    refused("lion_sde_dpmpp_update", x[1:], e, h, None, 8, *co, words, 0, 0, o, ho, None)        # misaligned x
    refused("lion_sde_dpmpp_update", x, e, h, z[2:], 8, *co, None, 0, 0, o, ho, None)            # ... z_in
    refused("lion_sde_dpmpp_update", x, e, h, None, 8, *co, words, 0, 0, o, ho, z[1:])           # ... z_out
    refused("lion_chain_update_multistep_noise", x, e, h, 64, cur, None, words, 0, o, ho, None)  # table
    refused("lion_chain_update_multistep_noise", x, e, h, 64, cur, table, None, 0, o, ho, None)  # seed
    refused("lion_chain_update_multistep_noise", x, e, None, 64, cur, table, words, 0, o, ho, None)
    refused("lion_chain_update_multistep_noise", x, e, h, 0, cur, table, words, 0, o, ho, None)
    refused("lion_chain_update_multistep_noise", x, e[1:], h, 8, cur, table, words, 0, o, ho, None)
    refused("lion_chain_update_multistep_noise_cm", x, e, h, 0, 4, cur, table, words, 0, o, ho, None)
    refused("lion_chain_update_multistep_noise_cm", x, e, h, 2, 0, cur, table, words, 0, o, ho, None)
    refused("lion_chain_update_multistep_noise_cm", x, e, h, 2, 4, None, table, words, 0, o, ho, None)
    refused("lion_chain_update_multistep_noise_cm", x, e, h[1:], 2, 4, cur, table, words, 0, o, ho, None)
    torch.cuda.synchronize()
    assert all(bool((t == 2.0).all()) for t in a)           # nothing ran


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


def _variance_recursion(table, steps, ab, s):
    """P_xx on arrival at the last index, in float64 on the (float32) table the chain ran: the pair (x, hist) evolves by
    M = [[a2 + a3*a4*c_t, a3*a5], [c_t, 0]], c_t = alpha_t*s^2/v_t, plus the fresh noise: P <- M P M^T + diag(a6^2, 0)"""
    v = ab * s * s + 1.0 - ab
    tb = np.asarray(table, np.float64)
    P = np.diag([v[steps[0]], 0.0])
    for row, t in zip(tb[:-1], steps[:-1]):
        c = np.sqrt(ab[t]) * s * s / v[t]
        M = np.array([[row[3] + row[4] * row[5] * c, row[4] * row[6]], [c, 0.0]])
        P = M @ P @ M.T + np.diag([row[7] ** 2, 0.0])
    return P[0, 0]


def test_whole_chain_on_a_toy_denoiser():
    """graph == eager from one seed, bit for bit; the seed governs the result; a second call captures nothing; and the sample
    variance on arrival at index 0 is the float64 recursion's P_xx within 5 standard deviations of a variance estimate from
    n = 262144 independent Gaussians (5*sqrt(2/n) = 1.4 % relative) plus 1e-4 for the float32 chain: a test of the noise
    scale the kernel applies, not of the solver's order."""
    from lion_amd import chain
    d = _diffusion()
    s, B, S, numel = 0.5, 32, 10, 8192
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    v = ab * s * s + 1.0 - ab
    toy = ToyDenoiser(torch.from_numpy((np.sqrt(1.0 - ab) / v).astype(np.float32))).cuda()
    g = torch.Generator(device="cuda").manual_seed(5)
    xs = torch.randn(B, numel, 1, 1, device="cuda", generator=g) * float(np.sqrt(v[-1]))
    keep = xs.clone()
    steps = d.solver_schedule(S)
    table = d.dpm_solver_table(steps, stochastic=True)
    assert len(steps) == S
    a, traj = d.run_dpm_solver(toy, B, [numel, 1, 1], steps=S, x_noisy=xs, stochastic=True, seed=SEED, graph=True)
    entries = dict(d._chains._entries)
    entry = list(entries.values())[-1]
    assert len(entries) == 1 and entry.mode == chain.SDE_DPMPP == 3 and entry.hist is not None and entry.z is None
    assert len(traj) == S and torch.equal(traj[-1], a) and torch.isfinite(a).all()
    b, traj_b = d.run_dpm_solver(toy, B, [numel, 1, 1], steps=S, x_noisy=xs, stochastic=True, seed=SEED, graph=False)
    assert all(torch.equal(p, q) for p, q in zip(traj, traj_b)) and torch.equal(a, b)
    assert torch.equal(xs, keep)                                       # the caller's start is not written
    a2, _ = d.run_dpm_solver(toy, B, [numel, 1, 1], steps=S, x_noisy=xs, stochastic=True, seed=SEED, keep_trajectory=False)
    c, _ = d.run_dpm_solver(toy, B, [numel, 1, 1], steps=S, x_noisy=xs, stochastic=True, seed=SEED + 1, keep_trajectory=False)
    assert torch.equal(a2, a) and not torch.equal(c, a)
    assert dict(d._chains._entries) == entries                         # one capture served all of it
    torch.manual_seed(9)                                               # seed=None: torch's generator governs the key
    e1, _ = d.run_dpm_solver(toy, B, [numel, 1, 1], steps=S, x_noisy=xs, stochastic=True, keep_trajectory=False)
    torch.manual_seed(9)
    e2, _ = d.run_dpm_solver(toy, B, [numel, 1, 1], steps=S, x_noisy=xs, stochastic=True, keep_trajectory=False, graph=False)
    assert torch.equal(e1, e2) and not torch.equal(e1, a)
    # the first step is the by-value kernel on the chain generator's noise for (seed, step 0, stream 0)
    from lion_amd.diffusion_ops import sde_dpmpp_update
    eps0 = toy(xs, torch.full((B,), float(table[0, 0]), device="cuda"))
    want0, _, z0 = sde_dpmpp_update(xs, eps0, None, *[float(t) for t in table[0, 1:8]], seed=SEED, step=0, return_noise=True)
    assert torch.equal(traj[0], want0) and torch.equal(z0.flatten(), _chain_noise(xs.numel(), 0, 0))
    # the variance on arrival at index 0: the state before the last row
    n = B * numel
    pxx = _variance_recursion(table, steps, ab, s)
    got = float(traj[-2].double().pow(2).mean())
    bound = 5.0 * np.sqrt(2.0 / n) + 1e-4
    print(f"toy s={s} S={S}: sample variance {got:.6f}  recursion {pxx:.6f}  v_0 {v[0]:.6f}  "
          f"relative {got / pxx - 1:+.2e} (bound {bound:.2e})")
    assert abs(got / pxx - 1.0) <= bound
    # the deterministic solver beside it: its own cache entry, its own result, and the stochastic capture is kept
    dd, _ = d.run_dpm_solver(toy, B, [numel, 1, 1], steps=S, x_noisy=xs, keep_trajectory=False)
    after = d._chains._entries
    assert len(after) == 2 and all(after[k] is w for k, w in entries.items()) and not torch.equal(dd, a)


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


def _priors(lion, B):
    sh = lion.vae.latent_shape()
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda", generator=g))
    return (lion.priors[0], sh[0], None), (lion.priors[1], sh[1], style)


def test_captured_step_equals_eager_step_on_the_priors(small_lion):
    """Every replay of the captured step leaves x and hist == lion_sde_dpmpp_update(x_i, prior(x_i, t_i), hist_i, row_i) on the
    seed's noise for step i, evaluated eagerly on the graph's own previous state: the flat update behind the global prior, the
    channel-major one behind the local.  With record_noise the chain reports that noise; the warm-up drew none."""
    from lion_amd import chain, diffusion_ops
    lion, d = small_lion, small_lion.diffusion
    lion.priors.eval()
    B, S = 2, 5
    with torch.no_grad():
        for k, (prior, shape, cond) in enumerate(_priors(lion, B)):
            steps = d.solver_schedule(S, "logsnr", 300)
            table = d.dpm_solver_table(steps, stochastic=True)
            assert len(steps) == S and np.all(table[1:-1, 6] != 0) and np.all(table[:-1, 7] != 0) and table[-1, 7] == 0
            ch = chain.GraphedChain(prior, B, shape, cond, None, "cuda", chain.SDE_DPMPP, 16, record_noise=True)
            assert ch.cm_out == (k == 1) and ch.hist is not None
            assert not ch.z.any() and torch.isfinite(ch.x).all()          # identity rows: finite and draw-free
            x0 = torch.randn([B] + shape, device="cuda")
            ch.prepare(x0, table, SEED, cond, None)
            assert torch.equal(ch.x, x0) and not ch.hist.any()
            words = diffusion_ops.seed_words(SEED, "cuda")
            for i in range(S):
                x_i, h_i = ch.x.clone(), ch.hist.clone()
                ch.replay()
                tt = torch.full((B,), float(table[i, 0]), device="cuda")
                eps = prior(x=x_i, t=tt, condition_input=cond, clip_feat=None).float().contiguous()
                want_x, want_h, z = diffusion_ops.sde_dpmpp_update(x_i, eps, h_i, *[float(v) for v in table[i, 1:8]], seed=words,
                                                                   step=i, return_noise=True)
                assert torch.equal(ch.x, want_x), (k, i, (ch.x - want_x).abs().max().item() / want_x.abs().max().item())
                assert torch.equal(ch.hist, want_h) and torch.equal(ch.z, z), (k, i)
                assert z.any() == (i < S - 1)
            assert torch.isfinite(ch.x).all()


def test_sampler_graph_equals_eager_on_the_priors(small_lion):
    lion, d = small_lion, small_lion.diffusion
    B, S = 2, 5
    for prior, shape, cond in _priors(lion, B):
        x0 = torch.randn([B] + shape, device="cuda")
        kw = dict(steps=S, x_noisy=x0, condition_input=cond, stochastic=True)
        a, tr = d.run_dpm_solver(prior, B, shape, seed=SEED, graph=True, **kw)
        b, tr_b = d.run_dpm_solver(prior, B, shape, seed=SEED, graph=False, **kw)
        assert len(tr) == len(tr_b) == S and torch.equal(tr[-1], a)
        assert torch.equal(a, b), (a - b).abs().max().item() / b.abs().max().item()
        assert torch.isfinite(a).all() and not torch.equal(a, x0)
        assert prior.training                               # as run_ddim leaves it
        c, _ = d.run_dpm_solver(prior, B, shape, seed=SEED + 1, keep_trajectory=False, **kw)
        assert torch.isfinite(c).all() and not torch.equal(a, c)


def test_state_hook_graph_equals_eager(small_lion):
    """a hook that overwrites half of the latent before every evaluation: the same result in both paths, called once per step"""
    lion, d = small_lion, small_lion.diffusion
    B, S = 2, 4
    prior, shape, cond = _priors(lion, B)[1]
    x0 = torch.randn([B] + shape, device="cuda")
    n = x0[0].numel()
    forced = [torch.randn(B, n // 2, device="cuda") for _ in range(S)]
    outs = {}
    for graph in (True, False):
        seen = []

        def hook(i, x):
            seen.append(i)
            x.view(B, -1)[:, :n // 2].copy_(forced[i])
        outs[graph], _ = d.run_dpm_solver(prior, B, shape, steps=S, x_noisy=x0, condition_input=cond, graph=graph,
                                          state_hook=hook, keep_trajectory=False, stochastic=True, seed=SEED)
        assert seen == list(range(S))
    plain, _ = d.run_dpm_solver(prior, B, shape, steps=S, x_noisy=x0, condition_input=cond, keep_trajectory=False,
                                stochastic=True, seed=SEED)
    assert torch.equal(outs[True], outs[False])
    assert not torch.equal(outs[True], plain)


def _count_calls(model, fn):
    """the timesteps `model` is evaluated at while fn() runs (eager paths: a replayed graph calls no module)"""
    seen = []
    handle = model.register_forward_pre_hook(lambda mod, args, kwargs: seen.append(float(kwargs["t"][0])), with_kwargs=True)
    try:
        out = fn()
    finally:
        handle.remove()
    return out, seen


@pytest.mark.parametrize("stochastic", [True, False])
def test_tail_from_t_start_visits_its_schedule(small_lion, stochastic):
    lion, d = small_lion, small_lion.diffusion
    B, S, t_start = 2, 6, 200
    prior, shape, cond = _priors(lion, B)[0]
    x0 = torch.randn([B] + shape, device="cuda")
    want = d.solver_schedule(S, "logsnr", t_start)
    assert want[0] == t_start and want[-1] == 0 and len(want) == S
    kw = dict(steps=S, x_noisy=x0, condition_input=cond, stochastic=stochastic, t_start=t_start, seed=SEED)
    (b, tr_b), seen = _count_calls(prior, lambda: d.run_dpm_solver(prior, B, shape, graph=False, **kw))
    assert seen == [float(t + 1) for t in want]                        # the model's timestep is the index + 1
    a, tr = d.run_dpm_solver(prior, B, shape, graph=True, **kw)
    assert len(tr) == len(want) and torch.equal(a, b) and torch.isfinite(a).all()
    full, _ = d.run_dpm_solver(prior, B, shape, steps=S, x_noisy=x0, condition_input=cond, stochastic=stochastic, seed=SEED,
                               keep_trajectory=False)
    assert not torch.equal(full, a)
    with pytest.raises(ValueError):
        d.run_dpm_solver(prior, B, shape, steps=S, t_start=t_start)     # a tail needs its start
    with pytest.raises(ValueError):
        d.run_dpm_solver(prior, B, shape, steps=S, x_noisy=x0, t_start=1000)


# ---- diffuse_denoise and the samplers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    g = torch.Generator(device="cuda").manual_seed(17)
    return torch.randn(2, 2048, 3, device="cuda", generator=g) * 0.5


def _edit(lion, cloud, time_start, **kw):
    from lion_amd.editing import diffuse_denoise
    return diffuse_denoise(lion.vae, lion.priors, lion.diffusion, cloud, time_start, **kw)


def test_diffuse_denoise_default_is_the_ancestral_tail(small_lion, cloud):
    a, ia = _edit(small_lion, cloud, (2, 3), seed=5)
    b, ib = _edit(small_lion, cloud, (2, 3), seed=5, solver_steps=None)
    assert torch.equal(a, b) and torch.isfinite(a).all() and ia["seeds"] == ib["seeds"]
    for key in ("global_edited", "local_edited"):
        assert torch.equal(ia[key], ib[key])
    assert ia["tail_steps"] == ([1, 0], [2, 1, 0])
    for bad in (1, 0, 2.0, True):
        with pytest.raises(ValueError):
            _edit(small_lion, cloud, (2, 3), seed=5, solver_steps=bad)


def test_diffuse_denoise_solver_tail(small_lion, cloud):
    lion, d = small_lion, small_lion.diffusion
    ts, S = (150, 200), 8
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    a, ia = _edit(lion, cloud, ts, seed=5, solver_steps=S)
    b, ib = _edit(lion, cloud, ts, seed=5, solver_steps=S)
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    assert a.shape == cloud.shape and torch.isfinite(a).all() and torch.equal(a, b) and ia["seeds"] == ib["seeds"]
    want = tuple(d.solver_schedule(S, "logsnr", t) for t in ts)
    assert ia["tail_steps"] == want and all(w[0] == t and len(w) <= S for w, t in zip(want, ts))
    for key in ("global", "local"):
        assert not torch.equal(ia[key + "_edited"], ia[key + "_original"])
    c, _ = _edit(lion, cloud, ts, seed=6, solver_steps=S)
    det, _ = _edit(lion, cloud, ts, seed=5, solver_steps=S, stochastic=False)
    assert not torch.equal(c, a) and not torch.equal(det, a) and torch.isfinite(det).all()
    # the eager loop: the same points, and len(schedule) evaluations of each prior
    seen = [[], []]
    handles = [p.register_forward_pre_hook(lambda mod, args, kwargs, k=k: seen[k].append(float(kwargs["t"][0])), with_kwargs=True)
               for k, p in enumerate(lion.priors)]
    try:
        e, _ = _edit(lion, cloud, ts, seed=5, solver_steps=S, graph=False)
    finally:
        for h in handles:
            h.remove()
    assert seen[0] == [float(t + 1) for t in want[0]] and seen[1] == [float(t + 1) for t in want[1]]
    assert torch.equal(e, a)


def test_diffuse_denoise_solver_tail_honours_zero_and_keep_first(small_lion, cloud):
    lion, d = small_lion, small_lion.diffusion
    _, info = _edit(lion, cloud, (0, 200), seed=5, solver_steps=8, keep_first=True)
    assert torch.equal(info["global_edited"], info["global_original"])
    assert info["tail_steps"] == ([], d.solver_schedule(8, "logsnr", 200))
    new, old = info["local_edited"], info["local_original"]
    assert torch.equal(new[0], old[0]) and not torch.equal(new[1], old[1]) and torch.isfinite(new).all()
    p0, i0 = _edit(lion, cloud, 0, seed=5, solver_steps=8)
    q0, _ = _edit(lion, cloud, 0, seed=5)
    assert torch.equal(p0, q0) and i0["tail_steps"] == ([], [])


def test_samplers_take_dpm_stochastic(small_lion):
    from lion_amd.sampling import generate_samples_vada_2prior
    lion, d = small_lion, _diffusion()
    B = 2
    sh = lion.vae.latent_shape()
    torch.manual_seed(11)
    p1, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, dpm_step=8, dpm_stochastic=True)
    torch.manual_seed(11)
    p2, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, dpm_step=8, dpm_stochastic=True)
    torch.manual_seed(11)
    p3, _ = generate_samples_vada_2prior(sh, lion.priors, d, lion.vae, B, dpm_step=8)
    assert tuple(p1.shape) == (B, 2048, 3) and torch.isfinite(p1).all() and torch.equal(p1, p2) and not torch.equal(p1, p3)
    modes = sorted(ch.mode for ch in d._chains._entries.values())
    assert modes == [2, 2, 3, 3]
    out = lion.sample(num_samples=2, dpm_step=8, dpm_stochastic=True)
    assert tuple(out['points'].shape) == (2, 2048, 3) and torch.isfinite(out['points']).all()
