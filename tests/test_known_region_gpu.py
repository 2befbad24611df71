"""-m gpu: region-preserving diffuse-denoise.  The "_known" update kernels against a composition of existing
kernels -- the "_from" update where a quad is not kept, lion_philox_normal_keyed on stream 2 into lion_chain_diffuse where it is
-- quad by quad and bit for bit, on both sides of a workgroup's 256 quads; then the contract on the real priors: graph equals
eager (A), an all-False mask is the call without `known` (B), an all-True mask returns x0 (C), the kept groups are x0 and the
forward draw at every level on the way (D), per-sample starts (E), batchmates' masks do not matter (F), one capture serves
every mask, x0 and first_row (G); then editing.diffuse_denoise(keep=)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KA, KB, KC = 0x1234567890ABCDEF, 0x0FEDCBA987654321, 0xDEADBEEF00000001
KEYS = (KA, KB, KC)
FIRST_ROW = (0, 2, 5)
ROWS = (0, 1, 2, 4, 5, 6)
#            mode  a0     a1     a2    a3    a4   a5       the rows of tests/test_start_steps_gpu.py
UN_ROWS = {"ddim": (0, 1.002, -0.03, 0.05, 0.0, 0.0, 0.0),            # out = x*s + (c*eps + sigma*z)
           "ddpm": (1, 1.01, 0.02, 0.7, 0.14, 0.9, 0.0),              # t > 0: a0*(x - a1*eps/a2) + (a3*z)*a4
           "ddpm_t0": (1, 1.01, 0.02, 1.0, 0.14, 0.9, 1.0)}           # t == 0 (a5 != 0): a0*(x - a1*eps)
LAYOUTS = [("flat", n) for n in (4, 1020, 1024, 1028)] + [("cm", N) for N in (1, 255, 256, 257)]
KNOWN_STREAM = 2
# known_ms tables of 8 rows (the kernel reads row cur[7] <= 6): a generic (m, s) that differs from row to row, and (1, 0)
MS = {"generic": [(0.8125 - 0.03125 * i, 0.58203125 + 0.015625 * i) for i in range(8)], "clean": [(1.0, 0.0)] * 8}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _words(keys):
    from lion_amd.chain import key_words
    return key_words(list(keys), "cuda")


def _cur(row, step):
    """cur as lion_chain_begin_step leaves it for table row `step` holding `row` = a0..a5"""
    cur = torch.zeros(8, device="cuda")
    cur[1:1 + len(row)] = torch.tensor([float(v) for v in row], device="cuda")
    cur.view(torch.int32)[7] = step
    return cur


def _special(x):
    """values whose bits a copy must keep, in the first quad of every sample"""
    flat = x.view(x.shape[0], -1)
    flat[:, 0] = -0.0
    flat[:, 1] = float("inf")
    _bits(flat)[:, 2] = 0x7FC00123                          # a NaN with a payload
    _bits(flat)[:, 3] = 0x00000001                          # the smallest denormal
    return x


def _operands(layout, B, size, seed):
    """x, eps as the kernel takes it, known_x0, the entry-point infix, (B, n or N), quads per sample"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if layout == "flat":
        x = torch.randn(B, size, device="cuda", generator=g)
        eps = torch.randn(B, size, device="cuda", generator=g)
        x0 = torch.randn(B, size, device="cuda", generator=g)
        return _special(x), eps, _special(x0), "", (B, size), size // 4
    x = torch.randn(B, size, 4, device="cuda", generator=g)
    eps = torch.randn(B, 4, size, device="cuda", generator=g)
    x0 = torch.randn(B, size, 4, device="cuda", generator=g)
    return _special(x), eps, _special(x0), "_cm", (B, size), size


def _mask(kind, quads):
    """one sample's mask bytes: nobody, everybody (any non-zero byte counts), or every third quad plus quads 255 and 256"""
    m = torch.zeros(quads, dtype=torch.uint8)
    if kind == "all":
        m[:] = torch.arange(quads) % 255 + 1
    elif kind == "mixed":
        m[::3] = 1
        for q in (255, 256):
            if q < quads:
                m[q] = 0x80
    return m


# ---- 1. the "_known" kernels against a composition of existing kernels ------------------------------------------------------------
@pytest.mark.parametrize("layout,size", LAYOUTS)
@pytest.mark.parametrize("kind", list(UN_ROWS))
def test_update_known_equals_composition_per_quad(kind, layout, size):
    from lion_amd import _lib, diffusion_ops
    row, B = UN_ROWS[kind], len(FIRST_ROW)
    x, eps, x0, infix, sizes, quads = _operands(layout, B, size, 37)
    x_keep, eps_keep, x0_keep = x.clone(), eps.clone(), x0.clone()
    first = torch.tensor(FIRST_ROW, dtype=torch.int32, device="cuda")
    words = _words(KEYS)
    frm, known = "lion_chain_update_noise%s_keyed_from" % infix, "lion_chain_update_noise%s_keyed_known" % infix
    n = x[0].numel()
    zero = torch.zeros_like(x[0])

    def call(x_, eps_, i, first_, keep_, ms_, out, z, x0_=x0):
        _lib.call(known, row[0], x_, eps_, *sizes, _cur(row[1:], i), first_, words, 0, x0_, keep_, ms_, KNOWN_STREAM, out, z)

    from_ref, draw_ref = {}, {}

    def from_at(i):                                         # the existing per-sample-start kernel at row i: (out, z)
        if i not in from_ref:
            out, z = torch.empty_like(x), torch.empty_like(x)
            _lib.call(frm, row[0], x, eps, *sizes, _cur(row[1:], i), first, words, 0, out, z)
            from_ref[i] = (out, z)
        return from_ref[i]

    def draw_at(word):                                      # every sample's draw at its step word `word` on the known stream
        if word not in draw_ref:
            draw_ref[word] = diffusion_ops.philox_normal_keyed(words, B, [n], word, stream_id=KNOWN_STREAM).view(x.shape)
        return draw_ref[word]

    fresh_ref = {}

    def fresh_at(name, i, word, m, s):                      # lion_chain_diffuse of x0 with that draw as z_in, at table row i
        if (name, i, word) not in fresh_ref:
            fresh_ref[name, i, word] = diffusion_ops.diffuse(x0, m, s, noise=draw_at(word))
        return fresh_ref[name, i, word]

    seen = {"held": 0, "not kept": 0, "kept, drawn": 0, "kept, clean": 0}
    kinds = ("none", "all", "mixed")
    for shift in range(3):                                  # every sample meets every mask
        keep = torch.stack([_mask(kinds[(b + shift) % 3], quads) for b in range(B)]).cuda()
        keep_before = keep.clone()
        elems = (keep != 0).repeat_interleave(4, dim=1).view(x.shape)
        for name, pairs in MS.items():
            ms = torch.tensor(pairs, device="cuda")
            for i in ROWS:
                m, s = (float(v) for v in ms[i].tolist())
                out, z = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
                call(x, eps, i, first, keep, ms, out, z)                    # a separate out
                x2 = x.clone()
                call(x2, eps, i, first, keep, ms, x2, None)                 # out aliased to x, no z_out
                x3, z3 = x.clone(), torch.full_like(x, float("nan"))
                call(x3, eps, i, first, keep, ms, x3, z3)                   # aliased, with z_out
                o_from, z_from = from_at(i)
                for b, f in enumerate(FIRST_ROW):
                    kept = int(elems[b].sum().item()) // 4
                    if i < f:                               # held: x bit for bit, kept quads included, nothing drawn
                        want, want_z = x_keep[b], zero
                        seen["held"] += quads
                    else:
                        if s != 0.0:                        # the forward draw of x0 under the sample's own row count
                            fresh, fresh_z = fresh_at(name, i, i - f, m, s)[b], draw_at(i - f)[b]
                            seen["kept, drawn"] += kept
                        else:
                            fresh, fresh_z = x0_keep[b], zero
                            seen["kept, clean"] += kept
                        seen["not kept"] += quads - kept
                        want = torch.where(elems[b], fresh, o_from[b])
                        want_z = torch.where(elems[b], fresh_z, z_from[b])
                        if kept < quads:
                            assert not _same(want, x_keep[b])
                        if kept and s != 0.0:
                            assert fresh_z.any()
                    where = (kind, layout, size, shift, name, i, b)
                    assert _same(out[b], want) and _same(z[b], want_z), where
                    assert _same(x2[b], want) and _same(x3[b], want) and _same(z3[b], want_z), where
        # a NULL first_row is a first_row of zeros
        ms = torch.tensor(MS["generic"], device="cuda")
        zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
        o0, z0, o1, z1 = (torch.empty_like(x) for _ in range(4))
        call(x, eps, 4, zeros, keep, ms, o0, z0)
        call(x, eps, 4, None, keep, ms, o1, z1)
        assert _same(o0, o1) and _same(z0, z1)
        # a kept quad reads neither eps nor x: NaN under the kept quads changes no output bit (row 6: nobody is held)
        if layout == "flat":
            eps_nan = torch.where(elems, torch.full_like(eps, float("nan")), eps)
        else:
            eps_nan = torch.where((keep != 0)[:, None, :], torch.full_like(eps, float("nan")), eps)
        x_nan = torch.where(elems, torch.full_like(x, float("nan")), x)
        call(x, eps, 6, first, keep, ms, o0, z0)
        call(x_nan, eps_nan, 6, first, keep, ms, o1, z1)
        assert _same(o0, o1) and _same(z0, z1)
        assert torch.equal(keep, keep_before)
    assert all(v > 0 for v in seen.values()), seen
    assert _same(x, x_keep) and _same(eps, eps_keep) and _same(x0, x0_keep)         # inputs untouched
    # the draw counts the sample's own rows on a stream of its own: sample 1 at row 2 draws its word 0, and not what the
    # ancestral step draws there
    assert not _same(draw_at(0)[1], draw_at(2)[1]) and not _same(draw_at(0)[1], from_at(2)[1][1])


# ---- the real priors --------------------------------------------------------------------------------------------------------------
STARTS = (3, 0, 2)
S = max(STARTS)


@pytest.fixture(scope="module")
def small_lion():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.lion import LION
    torch.manual_seed(3)
    lion = LION(released_prior_cfg())
    lion.priors.eval()
    lion.vae.eval()
    return lion


def _prior(lion, k, B):
    """the prior, its latent shape, its conditioning and the number of mask groups: 32 groups of 4 floats for the global
    latent, one group per point for the local one"""
    sh = lion.vae.latent_shape()
    if k == 0:
        return lion.priors[0], sh[0], None, 32
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda", generator=g))
    return lion.priors[1], sh[1], style, int(np.prod(sh[1])) // 4


def _groups(t, P):
    return t.reshape(t.shape[0], P, -1)


@pytest.mark.parametrize("k", [0, 1], ids=["global", "local"])
def test_known_region_tails_hold_the_contract(small_lion, k):
    from lion_amd import chain, diffusion_ops
    lion, d = small_lion, small_lion.diffusion
    B = len(STARTS)
    prior, shape, cond, P = _prior(lion, k, B)
    x0 = d._keyed_start([7, 8, 9], B, shape)                # the clean latent
    x_t = d.diffuse(x0, S, seeds=list(KEYS))                # the chain's start
    x0_keep, x_t_keep = x0.clone(), x_t.clone()
    g = torch.Generator().manual_seed(5)
    mixed = torch.rand(B, P, generator=g) < 0.4
    mixed[:, 0], mixed[:, 1] = True, False                  # both kinds in every sample
    nobody, everybody = torch.zeros(B, P, dtype=torch.bool), torch.ones(B, P, dtype=torch.bool)
    state = torch.get_rng_state(), torch.cuda.get_rng_state()

    def run(starts, keep, clean=x0, **kw):
        known = {} if keep is None else {"known": (clean, keep)}
        return d.run_denoising_diffusion_from_t(prior, B, shape, starts, x_t, condition_input=cond, seeds=list(KEYS), **known,
                                                **kw)

    def known_entries():
        return [ch for ch in d._chains._entries.values() if ch.known and ch.model is prior]
    out, traj = run(S, mixed)
    assert torch.isfinite(out).all() and len(traj) == S
    entries = known_entries()
    assert len(entries) == 1 and entries[0].keyed and entries[0].from_rows and entries[0].mode == chain.DDPM
    graphs = entries[0].graph
    # A: the eager composition gives the same bits, states included -- for an int start and for per-sample starts
    eager, traj_e = run(S, mixed, graph=False)
    assert _same(eager, out) and len(traj_e) == S and all(_same(a, b) for a, b in zip(traj_e, traj))
    per, traj_p = run(torch.tensor(STARTS), mixed.cuda())   # a mask on the device is taken as it is
    eager, traj_e = run(torch.tensor(STARTS), mixed, graph=False)
    assert _same(eager, per) and len(traj_e) == len(traj_p) == S and all(_same(a, b) for a, b in zip(traj_e, traj_p))
    # B: with nobody kept it is the call without `known` on the per-sample-start path
    for starts in (torch.tensor([S] * B), torch.tensor(STARTS)):
        plain, traj_plain = run(starts, None)
        masked, traj_m = run(starts, nobody)
        assert _same(masked, plain) and all(_same(a, b) for a, b in zip(traj_m, traj_plain))
    assert _same(run(S, nobody, keep_trajectory=False)[0], run(torch.tensor([S] * B), None, keep_trajectory=False)[0])
    # C: with everybody kept the call returns x0
    assert _same(run(S, everybody, keep_trajectory=False)[0], x0)
    # D: the kept groups of the result are x0, the others are not; on the way the kept groups are the forward draw of x0 at
    # the level the state has after the row -- lion_philox_normal_keyed on stream 2 into lion_chain_diffuse
    kept = mixed.cuda()
    og, xg = _groups(out, P), _groups(x0, P)
    equal = (_bits(og) == _bits(xg)).all(dim=2)
    assert torch.equal(equal, kept), (k, int(equal.sum()), int(kept.sum()))
    ms = d.known_levels(S)
    words = _words(KEYS)
    for i in range(S - 1):
        m, s = float(ms[i, 0]), float(ms[i, 1])
        assert s != 0.0
        z = diffusion_ops.philox_normal_keyed(words, B, shape, i, stream_id=KNOWN_STREAM)
        fresh = diffusion_ops.diffuse(x0, m, s, noise=z)
        equal = (_bits(_groups(traj[i], P)) == _bits(_groups(fresh, P))).all(dim=2)
        assert torch.equal(equal, kept), (k, i)
    assert _same(traj[S - 1], traj[S - 2])                  # the last entry repeats the state before the final update
    # E: per-sample starts under a mask: sample b is sample b of the uniform call with its start and the same mask
    for b, s in enumerate(STARTS):
        if s == 0:
            assert _same(per[b], x_t[b])                    # start 0 comes back as it went in, kept groups included
        else:
            want = out if s == S else run(s, mixed, keep_trajectory=False)[0]
            assert _same(per[b], want[b]), (k, b)
    for i in range(S):                                      # held until its first row
        assert _same(traj_p[i][1], x_t[1])
    # F: changing only sample 1's mask leaves samples 0 and 2 as they were
    other = mixed.clone()
    other[1] = ~other[1]
    changed, _ = run(S, other, keep_trajectory=False)
    assert _same(changed[0], out[0]) and _same(changed[2], out[2]) and not _same(changed[1], out[1])
    # G: a second call repeats the first; another mask, x0 and first_row (all of the above, and these) add no capture
    again, _ = run(S, mixed, keep_trajectory=False)
    assert _same(again, out)
    moved, _ = run(S, mixed, clean=x0 + 1.0, keep_trajectory=False)
    assert _same(_groups(moved, P)[kept], _groups(x0 + 1.0, P)[kept]) and not _same(moved, out)
    run(np.array([1, 3, 0]), other, keep_trajectory=False)
    entries = known_entries()
    assert len(entries) == 1 and entries[0].graph is graphs                 # one capture, never re-captured
    assert entries[0].first_row.tolist() == [2, 0, 3]
    # without seeds the call is keyed under split_seed(seed, B)
    split, _ = d.run_denoising_diffusion_from_t(prior, B, shape, S, x_t, condition_input=cond, seed=77, known=(x0, mixed),
                                                keep_trajectory=False)
    want, _ = d.run_denoising_diffusion_from_t(prior, B, shape, S, x_t, condition_input=cond, seeds=chain.split_seed(77, B),
                                               known=(x0, mixed), keep_trajectory=False)
    assert _same(split, want) and not _same(split, out)
    assert _same(x0, x0_keep) and _same(x_t, x_t_keep)      # the caller's tensors are never written
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])


# ---- editing.diffuse_denoise(keep=) -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    g = torch.Generator(device="cuda").manual_seed(17)
    return (torch.randn(1, 2048, 3, device="cuda", generator=g) * 0.5).expand(3, 2048, 3).contiguous()


def test_diffuse_denoise_keeps_the_marked_latent_points(small_lion, cloud):
    from lion_amd.editing import diffuse_denoise
    lion = small_lion
    B, N = cloud.shape[:2]
    g = torch.Generator().manual_seed(9)
    mask = torch.rand(B, N, generator=g) < 0.5
    state = torch.get_rng_state(), torch.cuda.get_rng_state()

    def run(keep, **kw):
        return diffuse_denoise(lion.vae, lion.priors, lion.diffusion, cloud, (0, 3), seeds=list(KEYS), keep=keep, **kw)

    def points(latent):
        return latent.reshape(B, N, -1)
    pts, info = run(mask)
    assert tuple(pts.shape) == (B, N, 3) and torch.isfinite(pts).all()
    assert info["keep"].dtype == torch.bool and torch.equal(info["keep"].cpu(), mask)
    assert info["time_start"] == (0, 3) and info["tail_steps"] == ([], [2, 1, 0])
    equal = (_bits(points(info["local_edited"])) == _bits(points(info["local_original"]))).all(dim=2)
    assert torch.equal(equal.cpu(), mask)                   # the kept latent points bit for bit, and no other
    assert info["global_edited"] is info["global_original"]
    # under seeds, sample 1 does not depend on its batchmates' masks
    other = torch.rand(B, N, generator=g) < 0.5
    other[1] = mask[1]
    pts_o, info_o = run(other)
    assert _same(pts_o[1], pts[1]) and _same(info_o["local_edited"][1], info["local_edited"][1])
    assert not _same(info_o["local_edited"][0], info["local_edited"][0])
    # [N] and [B, N] masks agree, tensor or array
    one = mask[1]
    pts_b, info_b = run(one.expand(B, N))
    for form in (one, one.numpy(), one.cuda()):
        pts_1, info_1 = run(form)
        assert _same(pts_1, pts_b) and _same(info_1["local_edited"], info_b["local_edited"])
        assert tuple(info_1["keep"].shape) == (B, N)
    assert _same(pts_b[1], pts[1])
    # keep_first and per-sample starts combine with it
    pts_k, info_k = run(mask, keep_first=True)
    assert _same(info_k["local_edited"][0], info_k["local_original"][0]) and _same(info_k["local_edited"][1:], info["local_edited"][1:])
    pair = ((0, 0, 0), (3, 0, 2))
    pts_s, info_s = diffuse_denoise(lion.vae, lion.priors, lion.diffusion, cloud, pair, seeds=list(KEYS), keep=mask)
    assert _same(info_s["local_edited"][0], info["local_edited"][0]) and _same(info_s["local_edited"][1], info_s["local_original"][1])
    equal = (_bits(points(info_s["local_edited"])) == _bits(points(info_s["local_original"]))).all(dim=2)
    assert torch.equal(equal[2].cpu(), mask[2])
    # a call without keep creates no known-region capture
    chains = lion.diffusion._chains
    chains.clear()
    plain, info_p = diffuse_denoise(lion.vae, lion.priors, lion.diffusion, cloud, (0, 3), seeds=list(KEYS))
    assert chains._entries and not any(ch.known for ch in chains._entries.values())
    assert info_p["keep"] is None and not _same(plain, pts)
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
