"""-m gpu: the deterministic few-step encoder (refined DDIM inversion).  The update kernel (lion_ddim_encode_update,
lion_chain_update_encode[_cm]) against a float32 numpy restatement, bit for bit; the whole chain on the toy denoiser of the
DPM-Solver tests and its round trip through the order-1 decoder; the captured step against the eager step on the real priors;
encode_interpolate on the discrete diffusion; and the existing samplers beside it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S_C = (0.62390161, 0.77528828)        # a middle leg of a 3-leg schedule: s = alpha_t/alpha_n, c = sigma_t - sigma_n*s
SENTINEL = -777.0


def restate(base, eps, s, c):
    """the kernel's expression on float32 numpy arrays: every operation rounds once"""
    return np.float32(s) * base + np.float32(c) * eps


def _cur(s, c, commit):
    return torch.tensor([303.0, s, c, float(commit), 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("numel", [1, 3, 4, 5, 255, 1027, 4096])
@pytest.mark.parametrize("commit", [0, 1])
def test_update_kernel_equals_float32_numpy(commit, numel):
    from lion_amd import _lib
    from lion_amd.diffusion_ops import ddim_encode_update
    rng = np.random.default_rng(numel)
    b, e = (rng.standard_normal(numel).astype(np.float32) for _ in range(2))
    want = torch.from_numpy(restate(b, e, *S_C)).cuda()
    assert torch.isfinite(want).all()
    db, de = torch.from_numpy(b).cuda(), torch.from_numpy(e).cuda()
    sentinel = torch.full_like(db, SENTINEL)
    # by value, out of place
    bo = sentinel.clone()
    out, r_bo = ddim_encode_update(db, de, *S_C, commit, base_out=bo)
    assert r_bo is bo and torch.equal(out, want)
    assert torch.equal(bo, want if commit else sentinel)            # commit = 0: base_out is not written
    assert torch.equal(db, torch.from_numpy(b).cuda()) and torch.equal(de, torch.from_numpy(e).cuda())   # inputs untouched
    out2, bo2 = ddim_encode_update(db, de, *S_C, commit)            # no base_out given: NULL without commit, a fresh one with
    assert torch.equal(out2, want) and ((bo2 is None) if not commit else torch.equal(bo2, want))
    # in place: base_out is base, out is the buffer the model read
    b3, x3 = db.clone(), torch.full_like(db, 5.0)
    r = ddim_encode_update(b3, de, *S_C, commit, out=x3, base_out=b3)
    assert r[0] is x3 and r[1] is b3 and torch.equal(x3, want) and torch.equal(b3, want if commit else db)
    # fully in place: out and base_out are both base
    b4 = db.clone()
    ddim_encode_update(b4, de, *S_C, commit, out=b4, base_out=b4)
    assert torch.equal(b4, want)
    # the captured step's form: the same coefficients read from cur[1..3], out of place and in place
    cur = _cur(*S_C, commit)
    o5, bo5 = torch.empty_like(db), sentinel.clone()
    _lib.call("lion_chain_update_encode", db, de, numel, cur, o5, bo5)
    assert torch.equal(o5, want) and torch.equal(bo5, want if commit else sentinel)
    b6, x6 = db.clone(), torch.full_like(db, 5.0)
    _lib.call("lion_chain_update_encode", b6, de, numel, cur, x6, b6)
    assert torch.equal(x6, want) and torch.equal(b6, want if commit else db)
    b7 = db.clone()
    _lib.call("lion_chain_update_encode", b7, de, numel, cur, b7, b7)
    assert torch.equal(b7, want)


@pytest.mark.parametrize("B,N", [(1, 1), (2, 3), (3, 64), (2, 257)])
@pytest.mark.parametrize("commit", [0, 1])
def test_channel_major_form_equals_the_flat_form(commit, B, N):
    from lion_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + N)
    base = torch.randn(B, N, 4, device="cuda", generator=g)
    eps_cm = torch.randn(B, 4, N, device="cuda", generator=g)
    cur = _cur(*S_C, commit)
    sentinel = torch.full_like(base, SENTINEL)
    o1, b1 = torch.empty_like(base), sentinel.clone()
    _lib.call("lion_chain_update_encode", base, eps_cm.permute(0, 2, 1).contiguous(), base.numel(), cur, o1, b1)
    o2, b2 = torch.empty_like(base), sentinel.clone()
    _lib.call("lion_chain_update_encode_cm", base, eps_cm, B, N, cur, o2, b2)
    assert torch.isfinite(o1).all() and torch.equal(o1, o2) and torch.equal(b1, b2)
    assert torch.equal(b2, o1 if commit else sentinel)
    b3, x3 = base.clone(), torch.zeros_like(base)            # in place, as the captured step runs it
    _lib.call("lion_chain_update_encode_cm", b3, eps_cm, B, N, cur, x3, b3)
    assert torch.equal(x3, o1) and torch.equal(b3, o1 if commit else base)


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
    """K = 0, 1, 2: graph == float32 numpy loop over encode_table == eager loop, bit for bit, on one capture that a second call
    reuses; the caller's latent is not written; and the round trip through run_dpm_solver(order=1) shows the CPU suite's ladder
    on float32 chains: every refinement at least halves the error."""
    from lion_amd import chain
    d = _diffusion()
    s, B, S = 0.5, 2, 20
    ab = d._h_alpha_bars.numpy().astype(np.float64)
    g = (np.sqrt(1.0 - ab) / (ab * s * s + 1.0 - ab)).astype(np.float32)
    toy = ToyDenoiser(torch.from_numpy(g)).cuda()
    start = (np.random.default_rng(5).standard_normal((B, 128, 1, 1)) * s).astype(np.float32)
    xs = torch.from_numpy(start).cuda()
    taus = d.solver_schedule(S)
    assert len(taus) == S
    errs, entry = [], None
    for K in (0, 1, 2):
        a, traj = d.run_ddim_forward(toy, xs, S, "logsnr", refine=K, graph=True, keep_trajectory=True)
        assert sum(e.mode == chain.ENCODE for e in d._chains._entries.values()) == 1
        if entry is None:
            entry = list(d._chains._entries.values())[-1]
            assert entry.mode == chain.ENCODE == 4 and entry.base is not None and entry.hist is None
        assert list(d._chains._entries.values())[-1] is entry          # one capture serves every K
        table = d.encode_table(taus, K)
        assert len(traj) == S and torch.equal(traj[-1], a)
        x = base = start.copy()
        leg = 0
        for row in table:
            x = restate(base, x * g[int(row[0]) - 1], row[1], row[2])
            if row[3] != 0:
                base = x
                assert np.array_equal(traj[leg].cpu().numpy(), x), (K, leg)
                leg += 1
        assert leg == S and np.isfinite(x).all()
        b, traj_b = d.run_ddim_forward(toy, xs, S, "logsnr", refine=K, graph=False, keep_trajectory=True)
        assert torch.equal(a, b) and len(traj_b) == S and all(torch.equal(p, q) for p, q in zip(traj, traj_b))
        a2, t2 = d.run_ddim_forward(toy, xs, S, "logsnr", refine=K)    # a second call captures nothing
        assert torch.equal(a2, a) and t2 == [] and list(d._chains._entries.values())[-1] is entry
        assert torch.equal(xs, torch.from_numpy(start).cuda())          # the caller's latent is not written
        back, _ = d.run_dpm_solver(toy, B, [128, 1, 1], steps=S, order=1, x_noisy=a, keep_trajectory=False)
        errs.append(float(np.linalg.norm(back.cpu().numpy().astype(np.float64) - start) / np.linalg.norm(start)))
    print("toy s=0.5 S=20 float32 round trip: " + " ".join(f"K={K} {e:.3e}" for K, e in enumerate(errs))
          + "  ratios " + " ".join(f"{p / q:.2f}" for p, q in zip(errs, errs[1:])))
    for K in range(2):
        assert errs[K + 1] <= errs[K] / 2.0, errs


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
    """Every replay of the captured step leaves x == lion_ddim_encode_update(base_i, prior(x_i, t_i), row_i) evaluated eagerly on
    the graph's own previous state, and base == x after a committing row, untouched otherwise: the flat update behind the
    global prior, the channel-major one behind the local."""
    from lion_amd import chain, diffusion_ops
    lion, d = small_lion, small_lion.diffusion
    lion.priors.eval()
    B, S, K = 2, 3, 1
    sh = lion.vae.latent_shape()
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda"))
        for k, (prior, shape, cond) in enumerate(((lion.priors[0], sh[0], None), (lion.priors[1], sh[1], style))):
            taus = d.solver_schedule(S)
            table = d.encode_table(taus, K)
            assert len(taus) == S and len(table) == S * (1 + K)
            ch = chain.GraphedChain(prior, B, shape, cond, None, "cuda", chain.ENCODE, 16)
            assert ch.cm_out == (k == 1)
            x0 = torch.randn([B] + shape, device="cuda")
            ch.prepare(x0, table, 0, cond, None)
            assert torch.equal(ch.x, x0) and torch.equal(ch.base, x0)
            for i in range(len(table)):
                x_i, b_i = ch.x.clone(), ch.base.clone()
                ch.replay()
                tt = torch.full((B,), float(table[i, 0]), device="cuda")
                eps = prior(x=x_i, t=tt, condition_input=cond, clip_feat=None).float().contiguous()
                want, _ = diffusion_ops.ddim_encode_update(b_i, eps, float(table[i, 1]), float(table[i, 2]), False)
                assert torch.equal(ch.x, want), (k, i, (ch.x - want).abs().max().item() / want.abs().max().item())
                assert torch.equal(ch.base, want if table[i, 3] != 0 else b_i), (k, i)
            assert torch.isfinite(ch.x).all() and not torch.equal(ch.x, x0)


def test_encoder_graph_equals_eager_on_the_priors(small_lion):
    lion, d = small_lion, small_lion.diffusion
    B, S, K = 2, 3, 1
    sh = lion.vae.latent_shape()
    style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda"))
    for prior, shape, cond in ((lion.priors[0], sh[0], None), (lion.priors[1], sh[1], style)):
        x0 = torch.randn([B] + shape, device="cuda")
        keep = x0.clone()
        a, tr = d.run_ddim_forward(prior, x0, S, "logsnr", condition_input=cond, refine=K, graph=True, keep_trajectory=True)
        b, tr_b = d.run_ddim_forward(prior, x0, S, "logsnr", condition_input=cond, refine=K, graph=False, keep_trajectory=True)
        assert len(tr) == len(tr_b) == S and torch.equal(tr[-1], a)
        assert torch.equal(a, b), (a - b).abs().max().item() / b.abs().max().item()
        assert all(torch.equal(p, q) for p, q in zip(tr, tr_b))
        assert torch.isfinite(a).all() and not torch.equal(a, x0) and torch.equal(x0, keep)
        assert prior.training                               # as run_ddim leaves it


def test_encode_interpolate_on_the_discrete_diffusion(small_lion):
    from lion_amd.interpolation import decode_noise, encode_interpolate, encode_noise
    lion, d = small_lion, small_lion.diffusion
    B, S, K = 4, 3, 1
    clouds = torch.randn(B, 2048, 3, device="cuda") * 0.3
    with torch.no_grad():
        latents = [t.clone() for t in lion.vae.decompose_eps(lion.vae.encode(clouds)[0])]
    kw = dict(latents=latents, steps=S, refine=K)
    out, info = encode_interpolate(lion.vae, lion.priors, d, clouds, graph=True, **kw)
    assert tuple(out.shape) == (B, 2048, 3) and torch.isfinite(out).all()
    legs = len(d.solver_schedule(S))
    assert info["nfe"] == [legs * (1 + K), legs, legs * (1 + K), legs]
    assert set(info) >= {"latents", "nfe", "interpolated"}
    # the end rows' noise is what the encoder gave: the mixing replaces rows 1 .. B-2 only
    noise = encode_noise(lion.vae, lion.priors, d, **kw)
    for z_mixed, z in zip(info["noise"], noise):
        assert torch.isfinite(z_mixed).all()
        assert torch.equal(z_mixed[0], z[0]) and torch.equal(z_mixed[-1], z[-1])
        assert not torch.equal(z_mixed[1], z[1]) and not torch.equal(z_mixed[2], z[2])
    # decode_noise is the decoder encode_interpolate ran
    g, l = decode_noise(lion.vae, lion.priors, d, info["noise"], steps=S)
    assert torch.equal(g, info["interpolated"][0]) and torch.equal(l, info["interpolated"][1])
    out_e, info_e = encode_interpolate(lion.vae, lion.priors, d, clouds, graph=False, **kw)
    assert torch.equal(out, out_e)
    assert all(torch.equal(p, q) for p, q in zip(info["noise"] + info["interpolated"], info_e["noise"] + info_e["interpolated"]))


def test_nothing_existing_moves(small_lion):
    """a run_dpm_solver result and a run_ddim result on one DiffusionDiscretized: the same bits before and after an encode call on
    it, their captures kept beside the encoder's"""
    from lion_amd import chain
    lion, d = small_lion, _diffusion()
    B = 2
    sh = lion.vae.latent_shape()
    prior = lion.priors[0]
    x0 = torch.randn([B] + sh[0], device="cuda")
    ddim = lambda: d.run_ddim(prior, B, sh[0], ddim_step=4, kappa=0.0, x_noisy=x0, is_image=False)[0]
    dpm = lambda: d.run_dpm_solver(prior, B, sh[0], steps=4, x_noisy=x0, keep_trajectory=False)[0]
    before = ddim(), dpm()
    entries = dict(d._chains._entries)
    assert len(entries) == 2
    z, _ = d.run_ddim_forward(prior, x0, 4, "logsnr", refine=1)
    after = dict(d._chains._entries)
    assert len(after) == 3 and all(after[k] is v for k, v in entries.items())       # one entry added, none replaced
    new = [v for k, v in after.items() if k not in entries]
    assert len(new) == 1 and new[0].mode == chain.ENCODE
    assert torch.equal(ddim(), before[0]) and torch.equal(dpm(), before[1])
    assert dict(d._chains._entries) == after
    assert torch.isfinite(z).all() and not torch.equal(z, x0)
