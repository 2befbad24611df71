"""-m gpu: per-sample start steps.  The "_from" update kernels and the "_at" forward draw against the existing
keyed kernels, sample by sample and bit for bit, on both sides of a workgroup's 256 quads; then the contract on the real priors:
a sample with start s in a mixed batch is the bits of that sample in a batch where everybody starts at s (A), start 0 comes
back as it went in (B), equal entries are the int call (C), graph equals eager (D), a second call repeats the first and another
first_row reuses the capture (E)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KA, KB, KC = 0x1234567890ABCDEF, 0x0FEDCBA987654321, 0xDEADBEEF00000001
KEYS = (KA, KB, KC)
FIRST_ROW = (0, 2, 5)
ROWS = (0, 1, 2, 4, 5, 6)
#            mode  a0     a1     a2    a3    a4   a5       the rows of tests/test_sample_seeds_gpu.py
UN_ROWS = {"ddim": (0, 1.002, -0.03, 0.05, 0.0, 0.0, 0.0),            # out = x*s + (c*eps + sigma*z)
           "ddpm": (1, 1.01, 0.02, 0.7, 0.14, 0.9, 0.0),              # t > 0: a0*(x - a1*eps/a2) + (a3*z)*a4
           "ddpm_t0": (1, 1.01, 0.02, 1.0, 0.14, 0.9, 1.0)}           # t == 0 (a5 != 0): a0*(x - a1*eps)
LAYOUTS = [("flat", n) for n in (4, 1020, 1024, 1028)] + [("cm", N) for N in (1, 255, 256, 257)]


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


def _operands(layout, B, size, seed):
    """x, eps as the kernel takes it, the entry-point infix, (B, n or N).  x holds values whose bits a copy must keep."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    if layout == "flat":
        x = torch.randn(B, size, device="cuda", generator=g)
        eps = torch.randn(B, size, device="cuda", generator=g)
        infix = ""
    else:
        x = torch.randn(B, size, 4, device="cuda", generator=g)
        eps = torch.randn(B, 4, size, device="cuda", generator=g)
        infix = "_cm"
    flat = x.view(B, -1)
    flat[:, 0] = -0.0
    flat[:, 1] = float("inf")
    _bits(flat)[:, 2] = 0x7FC00123                          # a NaN with a payload
    _bits(flat)[:, 3] = 0x00000001                          # the smallest denormal
    return x, eps, infix, (B, size)


# ---- 1. the "_from" kernels against the keyed kernels -----------------------------------------------------------------------------
@pytest.mark.parametrize("layout,size", LAYOUTS)
@pytest.mark.parametrize("kind", list(UN_ROWS))
def test_update_from_equals_keyed_update_per_sample(kind, layout, size):
    from lion_amd import _lib
    row, B = UN_ROWS[kind], len(FIRST_ROW)
    x, eps, infix, sizes = _operands(layout, B, size, 23)
    x_keep, eps_keep = x.clone(), eps.clone()
    first = torch.tensor(FIRST_ROW, dtype=torch.int32, device="cuda")
    words = _words(KEYS)
    keyed, frm = "lion_chain_update_noise%s_keyed" % infix, "lion_chain_update_noise%s_keyed_from" % infix
    ref = {}                                                # local step word -> (out, z) of the existing keyed kernel

    def keyed_at(word):
        if word not in ref:
            out, z = torch.empty_like(x), torch.empty_like(x)
            _lib.call(keyed, row[0], x, eps, *sizes, _cur(row[1:], word), words, 0, out, z)
            ref[word] = (out, z)
        return ref[word]
    seen = {"held": 0, "active": 0}
    for i in ROWS:
        out, z = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
        _lib.call(frm, row[0], x, eps, *sizes, _cur(row[1:], i), first, words, 0, out, z)       # a separate out
        x2 = x.clone()
        _lib.call(frm, row[0], x2, eps, *sizes, _cur(row[1:], i), first, words, 0, x2, None)    # out aliased to x, no z_out
        x3, z3 = x.clone(), torch.full_like(x, float("nan"))
        _lib.call(frm, row[0], x3, eps, *sizes, _cur(row[1:], i), first, words, 0, x3, z3)      # aliased, with z_out
        for b, f in enumerate(FIRST_ROW):
            if i < f:                                       # held: x bit for bit, nothing drawn
                want, want_z = x_keep[b], torch.zeros_like(x[b])
                seen["held"] += 1
            else:                                           # the keyed update for the row's coefficients, step word i - f
                o, zz = keyed_at(i - f)
                want, want_z = o[b], zz[b]
                seen["active"] += 1
                assert want_z.any() and not _same(want, x_keep[b])
            assert _same(out[b], want) and _same(z[b], want_z), (kind, layout, size, i, b)
            assert _same(x2[b], want) and _same(x3[b], want) and _same(z3[b], want_z), (kind, layout, size, i, b)
    assert seen == {"held": 6, "active": 12}
    assert _same(x, x_keep) and _same(eps, eps_keep)        # inputs untouched
    # sample 1 at rows 2 and 4 draws what sample 1 of a chain that started there draws at its rows 0 and 2 -- not rows 2 and 4
    assert not _same(keyed_at(0)[1][1], keyed_at(2)[1][1])
    # a held sample reads no key: a poisoned key buffer for the held samples changes nothing
    poisoned = words.clone()
    poisoned[1:] = 0x5A5A5A5A
    out_p, z_p = torch.empty_like(x), torch.empty_like(x)
    _lib.call(frm, row[0], x, eps, *sizes, _cur(row[1:], 1), first, poisoned, 0, out_p, z_p)
    out_c, z_c = torch.empty_like(x), torch.empty_like(x)
    _lib.call(frm, row[0], x, eps, *sizes, _cur(row[1:], 1), first, words, 0, out_c, z_c)
    assert _same(out_p, out_c) and _same(z_p, z_c)


# ---- 2. the "_at" forward draw against the keyed forward draw ---------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "offset"])
@pytest.mark.parametrize("n", [4, 1020, 1024, 1028])
def test_diffuse_at_equals_keyed_diffuse_per_sample(n, aligned):
    from lion_amd import _lib, diffusion_ops
    B = 3
    ms = [(0.8125, 0.58203125), (1.0, 0.0), (0.25, 0.96875)]               # sample 1 is skipped
    x0, _, _, _ = _operands("flat", B, n, 29)
    if not aligned:                                         # 4 bytes off a 16-byte boundary: the element-by-element path
        base = torch.empty(B * n + 1, device="cuda")
        base[1:].copy_(x0.view(-1))
        x0 = base[1:].view(B, n)
        assert x0.data_ptr() % 16 == 4
    keep = x0.clone()
    words = _words(KEYS)
    ms_dev = torch.tensor(ms, device="cuda")
    out, z = torch.full_like(keep, float("nan")), torch.full_like(keep, float("nan"))
    _lib.call("lion_chain_diffuse_keyed_at", x0, B, n, ms_dev, words, 1, out, z)
    for b, (m, s) in enumerate(ms):
        o1, z1 = torch.empty_like(keep), torch.empty_like(keep)
        _lib.call("lion_chain_diffuse_keyed", x0, B, n, m, s, words, 1, o1, z1)
        if (m, s) == (1.0, 0.0):
            assert _same(out[b], keep[b]) and not z[b].any() and z1[b].any()
        else:
            assert _same(out[b], o1[b]) and _same(z[b], z1[b]) and z[b].any(), (n, b)
    assert _same(x0, keep)
    x2 = x0.clone() if aligned else x0                      # in place
    _lib.call("lion_chain_diffuse_keyed_at", x2, B, n, ms_dev, words, 1, x2, None)
    assert _same(x2, out)
    if aligned:                                             # the wrapper: host pairs, return_noise
        o3, z3 = diffusion_ops.diffuse_at(keep, ms, list(KEYS), return_noise=True)
        assert _same(o3, out) and _same(z3, z)
        with pytest.raises(ValueError):
            diffusion_ops.diffuse_at(keep, ms[:2], list(KEYS))
        with pytest.raises(ValueError):
            diffusion_ops.diffuse_at(keep, ms, [1, 2])


# ---- the real priors --------------------------------------------------------------------------------------------------------------
STARTS = (3, 0, 2)


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
    sh = lion.vae.latent_shape()
    if k == 0:
        return lion.priors[0], sh[0], None
    g = torch.Generator(device="cuda").manual_seed(21)
    with torch.no_grad():
        style = lion.vae.global2style(torch.randn([B] + sh[0], device="cuda", generator=g))
    return lion.priors[1], sh[1], style


@pytest.fixture(scope="module")
def uniform_tails(small_lion):
    """per prior: the start latent and, for every start that occurs, the uniform call on the full batch of 3 under KEYS
    (result, trajectory) -- computed once, never written afterwards"""
    lion, d = small_lion, small_lion.diffusion
    B, made = len(STARTS), {}
    for k in (0, 1):
        prior, shape, cond = _prior(lion, k, B)
        x0 = d._keyed_start([7, 8, 9], B, shape)
        made[k] = (x0, {s: d.run_denoising_diffusion_from_t(prior, B, shape, s, x0, condition_input=cond, seeds=list(KEYS))
                        for s in (1, 2, 3)})
    return made


@pytest.mark.parametrize("k", [0, 1], ids=["global", "local"])
def test_tails_from_rows_hold_the_contract(small_lion, uniform_tails, k):
    from lion_amd import chain
    lion, d = small_lion, small_lion.diffusion
    B = len(STARTS)
    prior, shape, cond = _prior(lion, k, B)
    x0, uni = uniform_tails[k]
    x0_keep = x0.clone()
    state = torch.get_rng_state(), torch.cuda.get_rng_state()

    def run(starts, **kw):
        return d.run_denoising_diffusion_from_t(prior, B, shape, starts, x0, condition_input=cond, seeds=list(KEYS), **kw)
    mixed, traj = run(torch.tensor(STARTS))
    assert torch.isfinite(mixed).all() and len(traj) == max(STARTS)
    for b, s in enumerate(STARTS):
        if s:                                               # A: the uniform call with time_start = s, on the full batch
            assert _same(mixed[b], uni[s][0][b]), (k, b, (mixed[b] - uni[s][0][b]).abs().max().item())
            assert not _same(mixed[b], x0[b])
            for other in set(STARTS) - {0, s}:
                assert not _same(mixed[b], uni[other][0][b])
        else:                                               # B: start 0 comes back as it went in
            assert _same(mixed[b], x0[b])
    # the reported states: held until the sample's first row, then the states of its uniform call
    S = max(STARTS)
    for i in range(S):
        for b, s in enumerate(STARTS):
            want = x0[b] if i < S - s else uni[s][1][i - (S - s)][b]
            assert _same(traj[i][b], want), (k, i, b)
    # C: equal entries are the int call
    for form in (torch.tensor([2, 2, 2]), np.array([2, 2, 2], dtype=np.int32)):
        same, _ = run(form, keep_trajectory=False)
        assert _same(same, uni[2][0])
    # D: the eager debug path gives the same bits, states included
    eager, traj_e = run(torch.tensor(STARTS), graph=False)
    assert _same(eager, mixed) and len(traj_e) == len(traj) and all(_same(a, b) for a, b in zip(traj_e, traj))
    # E: a second call repeats the first; another first_row reuses the capture
    entries = dict(d._chains._entries)
    from_rows = [ch for ch in entries.values() if ch.from_rows and ch.model is prior]
    assert len(from_rows) == 1 and from_rows[0].keyed and from_rows[0].mode == chain.DDPM
    graphs = from_rows[0].graph
    again, _ = run(torch.tensor(STARTS), keep_trajectory=False)
    assert _same(again, mixed)
    other, _ = run(np.array([1, 3, 0]), keep_trajectory=False)
    assert dict(d._chains._entries) == entries and from_rows[0].graph is graphs        # no re-capture
    assert from_rows[0].first_row.tolist() == [2, 0, 3]
    assert _same(other[0], uni[1][0][0]) and _same(other[1], uni[3][0][1]) and _same(other[2], x0[2])
    # without seeds the call is keyed under split_seed(seed, B)
    split, _ = d.run_denoising_diffusion_from_t(prior, B, shape, torch.tensor(STARTS), x0, condition_input=cond, seed=77,
                                                keep_trajectory=False)
    want, _ = d.run_denoising_diffusion_from_t(prior, B, shape, torch.tensor(STARTS), x0, condition_input=cond,
                                               seeds=chain.split_seed(77, B), keep_trajectory=False)
    assert _same(split, want) and not _same(split, mixed)
    assert _same(x0, x0_keep)                               # the caller's start is never written
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])


def test_diffuse_per_sample_indices(small_lion):
    d = small_lion.diffusion
    B = 3
    for shape in small_lion.vae.latent_shape():
        g = torch.Generator(device="cuda").manual_seed(31)
        x0 = torch.randn([B] + shape, device="cuda", generator=g)
        keep = x0.clone()
        for t in ((3, 0, 2), (3, -1, 2), (-5, d._diffusion_steps - 1, -1)):
            out, z = d.diffuse(x0, torch.tensor(t), seeds=list(KEYS), return_noise=True)
            for b, tb in enumerate(t):
                if tb < 0:                                  # skipped: bit for bit, nothing drawn
                    assert _same(out[b], x0[b]) and not z[b].any()
                else:                                       # A: the int call on the full batch
                    o1, z1 = d.diffuse(x0, tb, seeds=list(KEYS), return_noise=True)
                    assert _same(out[b], o1[b]) and _same(z[b], z1[b]) and z[b].any(), (t, b)
            assert _same(d.diffuse(x0, np.array(t), seeds=list(KEYS)), out)
        from lion_amd.chain import split_seed
        assert _same(d.diffuse(x0, torch.tensor([3, 0, 2]), seed=5), d.diffuse(x0, torch.tensor([3, 0, 2]), seeds=split_seed(5, B)))
        assert _same(x0, keep)


@pytest.fixture(scope="module")
def cloud():
    g = torch.Generator(device="cuda").manual_seed(17)
    return (torch.randn(1, 2048, 3, device="cuda", generator=g) * 0.5).expand(3, 2048, 3).contiguous()


LATENTS = ("global_original", "global_edited", "local_original", "local_edited")


@pytest.mark.parametrize("keep_first", [False, True], ids=["plain", "keep_first"])
def test_diffuse_denoise_sample_equals_its_uniform_call(small_lion, cloud, keep_first):
    from lion_amd.editing import diffuse_denoise
    lion = small_lion
    pair = ((3, 0, 2), (1, 2, 0))
    state = torch.get_rng_state(), torch.cuda.get_rng_state()

    def run(time_start):
        return diffuse_denoise(lion.vae, lion.priors, lion.diffusion, cloud, time_start, seeds=list(KEYS), keep_first=keep_first)
    pts, info = run(pair)
    assert tuple(pts.shape) == (3, 2048, 3) and torch.isfinite(pts).all()
    assert info["time_start"] == pair and info["tail_steps"] == ([2, 1, 0], [1, 0])
    assert all(type(v) is int for t in info["time_start"] for v in t)
    for b in range(3):
        p1, i1 = run((pair[0][b], pair[1][b]))
        assert i1["time_start"] == (pair[0][b], pair[1][b])
        assert _same(pts[b], p1[b]), (b, (pts[b] - p1[b]).abs().max().item())
        for name in LATENTS:
            assert _same(info[name][b], i1[name][b]), (b, name)
    # what ran: sample 1's global latent and sample 2's local latent were left alone; the others were edited
    first = 1 if keep_first else 0
    for b in range(first, 3):
        assert _same(info["global_edited"][b], info["global_original"][b]) == (pair[0][b] == 0)
        assert _same(info["local_edited"][b], info["local_original"][b]) == (pair[1][b] == 0)
    if keep_first:
        assert _same(info["global_edited"][0], info["global_original"][0])
        assert _same(info["local_edited"][0], info["local_original"][0])
    # the other accepted forms of the same request
    p2, i2 = run((torch.tensor(pair[0]), np.array(pair[1])))
    assert _same(p2, pts) and i2["time_start"] == pair
    p3, i3 = run(torch.tensor([2, 2, 2]))                   # C, through the recipe: equal entries are the int call
    p4, i4 = run(2)
    assert _same(p3, p4) and i3["time_start"] == ((2, 2, 2), (2, 2, 2)) and i4["time_start"] == (2, 2)
    assert i3["tail_steps"] == i4["tail_steps"] == ([1, 0], [1, 0])
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
