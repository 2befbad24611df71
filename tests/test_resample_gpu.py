"""-m gpu: RePaint's resampling jumps on region-preserving diffuse-denoise.  The "_known_resample" update
kernels against a composition of existing kernels -- the "_known" update, then on the quads that are not kept
lion_philox_normal_keyed on stream 3 into lion_chain_diffuse -- quad by quad and bit for bit, on both sides of a workgroup's 256
quads; then the contract on the real priors over a walk of 6 rows: graph equals eager, the kept groups are x0, an all-True mask
returns x0, n_resample = 1 is the call without `resample` on its capture, the jumps change the result, batchmates' masks do not
matter, one capture serves every mask and x0; then editing.diffuse_denoise(keep=, resample=)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KA, KB, KC = 0x1234567890ABCDEF, 0x0FEDCBA987654321, 0xDEADBEEF00000001
KEYS = (KA, KB, KC)
FIRST_ROW = (0, 2, 5)
ROWS = (0, 1, 2, 4, 5, 6)                                   # below, at and above every first row
#            mode  a0     a1     a2    a3    a4   a5       the rows of tests/test_known_region_gpu.py
UN_ROWS = {"ddim": (0, 1.002, -0.03, 0.05, 0.0, 0.0, 0.0),            # out = x*s + (c*eps + sigma*z)
           "ddpm": (1, 1.01, 0.02, 0.7, 0.14, 0.9, 0.0),              # t > 0: a0*(x - a1*eps/a2) + (a3*z)*a4
           "ddpm_t0": (1, 1.01, 0.02, 1.0, 0.14, 0.9, 1.0)}           # t == 0 (a5 != 0): a0*(x - a1*eps)
LAYOUTS = [("flat", n) for n in (4, 1020, 1024, 1028)] + [("cm", N) for N in (1, 255, 256, 257)]
KNOWN_STREAM, RESAMPLE_STREAM = 2, 3
# tables of 8 rows (the kernel reads row cur[7] <= 6).  known_ms: a generic (m, s) that differs from row to row, and (1, 0)
MS = {"generic": [(0.8125 - 0.03125 * i, 0.58203125 + 0.015625 * i) for i in range(8)], "clean": [(1.0, 0.0)] * 8}
# known_jump: (1, 0) rows mixed with generic ones -- row 1 (only sample 0 runs), row 4 (samples 0 and 1), row 6 (everybody)
JUMP = [(1.0, 0.0), (0.96875, 0.2421875), (1.0, 0.0), (1.0, 0.0), (0.875, 0.484375), (1.0, 0.0), (0.9921875, 0.12109375),
        (1.0, 0.0)]


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


# ---- 1. the "_known_resample" kernels against a composition of existing kernels ---------------------------------------------------
@pytest.mark.parametrize("layout,size", LAYOUTS)
@pytest.mark.parametrize("kind", list(UN_ROWS))
def test_update_known_resample_equals_composition_per_quad(kind, layout, size):
    from lion_amd import _lib, diffusion_ops
    row, B = UN_ROWS[kind], len(FIRST_ROW)
    x, eps, x0, infix, sizes, quads = _operands(layout, B, size, 41)
    x_keep, eps_keep, x0_keep = x.clone(), eps.clone(), x0.clone()
    first = torch.tensor(FIRST_ROW, dtype=torch.int32, device="cuda")
    words = _words(KEYS)
    known, resample = "lion_chain_update_noise%s_keyed_known" % infix, "lion_chain_update_noise%s_keyed_known_resample" % infix
    n = x[0].numel()
    zero = torch.zeros_like(x[0])
    jump = torch.tensor(JUMP, device="cuda")
    jump_before = jump.clone()

    def call(x_, i, keep_, ms_, out, z, jump_=jump, first_=first):
        _lib.call(resample, row[0], x_, eps, *sizes, _cur(row[1:], i), first_, words, 0, x0, keep_, ms_, KNOWN_STREAM, jump_,
                  RESAMPLE_STREAM, out, z)

    def known_at(i, keep_, ms_):                            # the existing known-region kernel at row i: (out, z)
        out, z = torch.empty_like(x), torch.empty_like(x)
        _lib.call(known, row[0], x, eps, *sizes, _cur(row[1:], i), first, words, 0, x0, keep_, ms_, KNOWN_STREAM, out, z)
        return out, z

    draw_ref = {}

    def draw_at(word):                                      # every sample's draw at its step word `word` on the jumps' stream
        if word not in draw_ref:
            draw_ref[word] = diffusion_ops.philox_normal_keyed(words, B, [n], word, stream_id=RESAMPLE_STREAM).view(x.shape)
        return draw_ref[word]

    seen = {"held": 0, "kept": 0, "moved": 0, "not moved": 0}
    kinds = ("none", "all", "mixed")
    for shift in range(3):                                  # every sample meets every mask
        keep = torch.stack([_mask(kinds[(b + shift) % 3], quads) for b in range(B)]).cuda()
        keep_before = keep.clone()
        elems = (keep != 0).repeat_interleave(4, dim=1).view(x.shape)
        for name, pairs in MS.items():
            ms = torch.tensor(pairs, device="cuda")
            for i in ROWS:
                mf, sf = JUMP[i]
                out, z = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
                call(x, i, keep, ms, out, z)                                # a separate out
                x2 = x.clone()
                call(x2, i, keep, ms, x2, None)                             # out aliased to x, no z_out
                x3, z3 = x.clone(), torch.full_like(x, float("nan"))
                call(x3, i, keep, ms, x3, z3)                               # aliased, with z_out
                o_known, z_known = known_at(i, keep, ms)
                for b, f in enumerate(FIRST_ROW):
                    kept = int(elems[b].sum().item()) // 4
                    want, want_z = o_known[b], z_known[b]                   # z_out is the step's draw, jump or not
                    if i < f:                               # held: x bit for bit, special values included, nothing drawn
                        assert _same(want, x_keep[b]) and _same(want_z, zero)
                        seen["held"] += quads
                    elif sf != 0.0:                         # the quads that are not kept move on from their update
                        zr = draw_at(i - f)                 # ... under the sample's own row count
                        moved = diffusion_ops.diffuse(o_known, mf, sf, noise=zr)[b]
                        want = torch.where(elems[b], o_known[b], moved)
                        seen["kept"] += kept
                        seen["moved"] += quads - kept
                        if kept < quads:
                            assert not _same(want, o_known[b])
                            assert not _same(torch.where(elems[b], zero, zr[b]), torch.where(elems[b], zero, z_known[b]))
                    else:                                   # a (1, 0) row: the "_known" entry point bit for bit
                        seen["kept"] += kept
                        seen["not moved"] += quads - kept
                    where = (kind, layout, size, shift, name, i, b)
                    assert _same(out[b], want) and _same(z[b], want_z), where
                    assert _same(x2[b], want) and _same(x3[b], want) and _same(z3[b], want_z), where
        ms = torch.tensor(MS["generic"], device="cuda")
        # a table of (1, 0) rows is the "_known" entry point at every row, and a NULL first_row is a first_row of zeros
        no_jump = torch.tensor([(1.0, 0.0)] * 8, device="cuda")
        o0, z0, o1, z1 = (torch.empty_like(x) for _ in range(4))
        for i in (4, 6):
            call(x, i, keep, ms, o0, z0, jump_=no_jump)
            o_known, z_known = known_at(i, keep, ms)
            assert _same(o0, o_known) and _same(z0, z_known)
        zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
        call(x, 4, keep, ms, o0, z0, first_=zeros)
        call(x, 4, keep, ms, o1, z1, first_=None)
        assert _same(o0, o1) and _same(z0, z1)
        assert torch.equal(keep, keep_before)
    assert all(v > 0 for v in seen.values()), seen
    assert _same(x, x_keep) and _same(eps, eps_keep) and _same(x0, x0_keep) and _same(jump, jump_before)   # inputs untouched
    # the jump's draw is on a stream of its own: not the known region's draw of that word
    other = diffusion_ops.philox_normal_keyed(words, B, [n], 0, stream_id=KNOWN_STREAM).view(x.shape)
    assert not _same(draw_at(0), other)


# ---- the real priors --------------------------------------------------------------------------------------------------------------
START, RESAMPLE, ROWS_OF_WALK = 4, (2, 2), 6                # the walk t = 3 2^ 3 2 1 0: one jump of two levels, after row 1


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
def test_resampling_tails_hold_the_contract(small_lion, k):
    from lion_amd import chain, diffusion_ops
    lion, d = small_lion, small_lion.diffusion
    B = 3
    prior, shape, cond, P = _prior(lion, k, B)
    assert d.resample_walk(START, *RESAMPLE) == [(3, 0), (2, 2), (3, 0), (2, 0), (1, 0), (0, 0)]
    x0 = d._keyed_start([7, 8, 9], B, shape)                # the clean latent
    x_t = d.diffuse(x0, START, seeds=list(KEYS))            # the chain's start
    x0_keep, x_t_keep = x0.clone(), x_t.clone()
    g = torch.Generator().manual_seed(5)
    mixed = torch.rand(B, P, generator=g) < 0.4
    mixed[:, 0], mixed[:, 1] = True, False                  # both kinds in every sample
    everybody = torch.ones(B, P, dtype=torch.bool)
    state = torch.get_rng_state(), torch.cuda.get_rng_state()

    def run(keep, clean=x0, **kw):
        return d.run_denoising_diffusion_from_t(prior, B, shape, START, x_t, condition_input=cond, seeds=list(KEYS),
                                                known=(clean, keep), **kw)

    def entries(resample):
        return [ch for ch in d._chains._entries.values() if ch.known and ch.resample == resample and ch.model is prior]
    plain, traj_plain = run(mixed)                          # the call without resample: the known-region capture
    assert len(traj_plain) == START and len(entries(False)) == 1 and not entries(True)
    plain_graph = entries(False)[0].graph
    count = len(d._chains._entries)
    # n_resample = 1 is that call, on its capture: no new cache entry, nothing captured again
    for one in (1, (2, 1), (10, 1)):
        same, traj_same = run(mixed, resample=one)
        assert _same(same, plain) and len(traj_same) == START and all(_same(a, b) for a, b in zip(traj_same, traj_plain))
        assert _same(run(mixed, resample=one, graph=False, keep_trajectory=False)[0], plain)
    assert len(d._chains._entries) == count and entries(False)[0].graph is plain_graph and not entries(True)
    # the jumps: one more capture, 6 rows, another result
    out, traj = run(mixed, resample=RESAMPLE)
    assert torch.isfinite(out).all() and len(traj) == ROWS_OF_WALK
    made = entries(True)
    assert len(made) == 1 and made[0].keyed and made[0].from_rows and made[0].mode == chain.DDPM
    assert made[0].capacity >= d._diffusion_steps and len(entries(False)) == 1
    graphs = made[0].graph
    assert not _same(out, plain)
    # graph=False gives the same bits, every state included
    eager, traj_e = run(mixed, resample=RESAMPLE, graph=False)
    assert _same(eager, out) and len(traj_e) == ROWS_OF_WALK and all(_same(a, b) for a, b in zip(traj_e, traj))
    assert _same(traj[-1], traj[-2])                        # the last entry repeats the state before the final update
    # the kept groups of the result are x0 and the others are not; with everybody kept the call returns x0
    kept = mixed.cuda()
    equal = (_bits(_groups(out, P)) == _bits(_groups(x0, P))).all(dim=2)
    assert torch.equal(equal, kept), (k, int(equal.sum()), int(kept.sum()))
    assert _same(run(everybody, resample=RESAMPLE, keep_trajectory=False)[0], x0)
    # on the way the kept groups are the forward draw of x0 at the level behind the jump, and up to the jump the walk is the
    # plain tail: rows 0 and 1 have the plain tail's free groups (row 1's before its jump: its kept groups sit a level higher)
    table, ms, jump = d.resample_tables(START, *RESAMPLE)
    assert [float(v) != 0.0 for v in jump[:, 1]] == [False, True, False, False, False, False]
    words = _words(KEYS)
    for i in range(ROWS_OF_WALK - 1):
        z = diffusion_ops.philox_normal_keyed(words, B, shape, i, stream_id=KNOWN_STREAM)
        fresh = diffusion_ops.diffuse(x0, float(ms[i, 0]), float(ms[i, 1]), noise=z)
        equal = (_bits(_groups(traj[i], P)) == _bits(_groups(fresh, P))).all(dim=2)
        assert torch.equal(equal, kept), (k, i)
    assert _same(traj[0], traj_plain[0])
    zr = diffusion_ops.philox_normal_keyed(words, B, shape, 1, stream_id=RESAMPLE_STREAM)
    moved = diffusion_ops.diffuse(traj_plain[1], float(jump[1, 0]), float(jump[1, 1]), noise=zr)
    free = ~kept
    assert _same(_groups(traj[1], P)[free], _groups(moved, P)[free])
    # changing only sample 1's mask leaves samples 0 and 2 as they were
    other = mixed.clone()
    other[1] = ~other[1]
    changed, _ = run(other, resample=RESAMPLE, keep_trajectory=False)
    assert _same(changed[0], out[0]) and _same(changed[2], out[2]) and not _same(changed[1], out[1])
    # a second call repeats the first; another mask (above), another x0 and another walk add no capture
    again, _ = run(mixed, resample=RESAMPLE, keep_trajectory=False)
    assert _same(again, out)
    shifted, _ = run(mixed, clean=x0 + 1.0, resample=RESAMPLE, keep_trajectory=False)
    assert _same(_groups(shifted, P)[kept], _groups(x0 + 1.0, P)[kept]) and not _same(shifted, out)
    longer, traj_l = run(mixed, resample=(1, 2))            # t = 3^ 3 2^ 2 1^ 1 0
    assert len(traj_l) == 7 and not _same(longer, out)
    made = entries(True)
    assert len(made) == 1 and made[0].graph is graphs and len(entries(False)) == 1          # one capture, never re-captured
    assert entries(False)[0].graph is plain_graph
    assert _same(x0, x0_keep) and _same(x_t, x_t_keep)      # the caller's tensors are never written
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])


# ---- editing.diffuse_denoise(keep=, resample=) ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    g = torch.Generator(device="cuda").manual_seed(17)
    return (torch.randn(1, 2048, 3, device="cuda", generator=g) * 0.5).expand(3, 2048, 3).contiguous()


def test_diffuse_denoise_resamples_the_local_tail(small_lion, cloud):
    from lion_amd.editing import diffuse_denoise
    lion = small_lion
    B, N = cloud.shape[:2]
    g = torch.Generator().manual_seed(9)
    mask = torch.rand(B, N, generator=g) < 0.5
    state = torch.get_rng_state(), torch.cuda.get_rng_state()

    def run(start=(0, 4), **kw):
        return diffuse_denoise(lion.vae, lion.priors, lion.diffusion, cloud, start, seeds=list(KEYS), keep=mask, **kw)

    def points(latent):
        return latent.reshape(B, N, -1)
    pts, info = run(resample=RESAMPLE)
    assert tuple(pts.shape) == (B, N, 3) and torch.isfinite(pts).all() and torch.isfinite(info["local_edited"]).all()
    assert info["resample"] == RESAMPLE and info["tail_rows"] == (0, ROWS_OF_WALK)
    assert info["time_start"] == (0, 4) and info["tail_steps"] == ([], [3, 2, 1, 0])
    equal = (_bits(points(info["local_edited"])) == _bits(points(info["local_original"]))).all(dim=2)
    assert torch.equal(equal.cpu(), mask)                   # the kept latent points bit for bit, and no other
    assert info["global_edited"] is info["global_original"]
    # seeds= repeats the call bit for bit
    pts_2, info_2 = run(resample=RESAMPLE)
    assert _same(pts_2, pts) and _same(info_2["local_edited"], info["local_edited"])
    # the global latent's tail stays plain; an int is jump length 10, which has no anchor below 20
    pts_g, info_g = run((2, 4), resample=RESAMPLE)
    assert info_g["tail_rows"] == (2, ROWS_OF_WALK) and info_g["tail_steps"] == ([1, 0], [3, 2, 1, 0])
    plain, info_p = run()
    assert info_p["resample"] is None and info_p["tail_rows"] == (0, 4) and not _same(info_p["local_edited"], info["local_edited"])
    for one in (3, (2, 1)):
        pts_1, info_1 = run(resample=one)
        assert _same(pts_1, plain) and info_1["tail_rows"] == (0, 4)
        assert info_1["resample"] == ((10, 3) if one == 3 else (2, 1))
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
