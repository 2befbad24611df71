"""-m gpu: the inputs of guided synthesis.  csrc/perturb.hip against tests/perturb_ref.py bit for bit (voxel-surface points and
their face counts; uniform noise; outliers), normal noise against the forward process's keyed draw, addressing by sample,
stream capture, the entry points' refusals, and editing.voxel_guided on the released configuration with a 12-step schedule."""
import functools

import numpy as np
import pytest
import torch

import perturb_ref as ref
from test_perturb_reference_cpu import SEED, TWO_VOXELS, einval_cases

pytestmark = pytest.mark.gpu

KA, KB, KC, KD = SEED, 0x0FEDCBA987654321, 0xDEADBEEF00000001, 2 ** 64 - 7
KEYS = (KA, KB, KC)
T = 12


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int32)


def _pad(x, N):
    """x [n, 3] -> [N, 3] by repeating its first point: neither the box nor the occupancy changes"""
    x = np.asarray(x, dtype=np.float32)
    return np.concatenate([x, np.repeat(x[:1], N - len(x), axis=0)])


@functools.lru_cache(maxsize=None)
def _batch(kind, N, r):
    """float32 [3, N, 3], three different clouds (computed once, never written afterwards)"""
    if kind == "gauss":
        x = [ref.gaussian_cloud(N, 10 * N + b) * np.float32(0.5 + b) + np.float32(b) for b in range(3)]
    elif kind == "shell":
        x = [ref.shell_cloud(N, 100 + b) for b in range(3)]
    elif kind == "boundary":           # points on cell boundaries and on the box's max face; N = 3 (r + 1)
        x = [ref.boundary_cloud(r), ref.boundary_cloud(r)[::-1], ref.boundary_cloud(r) * np.float32(2.0)]
    elif kind == "closed2":            # F = 6 (identical points: h = 0), 24 (a full 2 x 2 x 2), 10 (two adjacent voxels) at r = 2
        x = [_pad([[0.3, -1.2, 2.5]], N), _pad(ref.grid_cloud(2), N), _pad(TWO_VOXELS, N)]
    elif kind == "closed3":            # the solid 3 x 3 x 3 block: the whole grid at r = 3 (F = 54); inside r = 8 with the two
        x = [_pad(ref.grid_cloud(3), N), ref.lattice_cloud(8, ref.block_cells(2, 3)), _pad([[1.0, 1.0, 1.0]], N)]   # corners
    x = np.stack([np.ascontiguousarray(c, dtype=np.float32) for c in x])
    assert x.shape == (3, N, 3)
    return x


@functools.lru_cache(maxsize=None)
def _ref_voxel(kind, N, r, K):
    x = _batch(kind, N, r)
    pts, faces = zip(*[ref.voxel_surface_points(x[b], r, K, KEYS[b])[:2] for b in range(3)])
    return np.stack(pts), list(faces)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# r in {1, 2, 8, 16, 32} x N in {1, 7, 64, 2048} x K in {1, 4, 100, 2048, 4096}: every value with several partners, the
# extremes together, K above and below the 1024 points one pass of the workgroup draws, one word (r <= 3) and 1024 words (r = 32)
VOXEL_CASES = [("gauss", 1, 1, 1), ("gauss", 1, 32, 4), ("gauss", 1, 8, 2048), ("gauss", 7, 2, 100), ("gauss", 7, 16, 4),
               ("gauss", 7, 32, 4096), ("gauss", 64, 1, 4), ("gauss", 64, 8, 100), ("gauss", 64, 16, 2048),
               ("gauss", 64, 32, 1), ("gauss", 2048, 1, 100), ("gauss", 2048, 2, 1), ("gauss", 2048, 8, 4096),
               ("gauss", 2048, 16, 2048), ("gauss", 2048, 32, 4096), ("gauss", 2048, 32, 2048),
               ("shell", 2048, 16, 2048), ("shell", 2048, 32, 100), ("shell", 64, 8, 4096), ("shell", 2048, 2, 4),
               ("boundary", 27, 8, 100), ("boundary", 51, 16, 2048), ("boundary", 99, 32, 4096),
               ("closed2", 9, 2, 4096), ("closed3", 29, 3, 2048), ("closed3", 29, 8, 2048), ("closed2", 9, 32, 100)]


@pytest.mark.parametrize("kind,N,r,K", VOXEL_CASES)
def test_voxel_surface_points_equal_the_reference(kind, N, r, K):
    from lion_amd.perturb import voxel_surface_points
    x = _batch(kind, N, r)
    want, faces = _ref_voxel(kind, N, r, K)
    got, info = voxel_surface_points(_dev(x), r, K, seeds=list(KEYS))
    assert tuple(got.shape) == (3, K, 3) and got.dtype == torch.float32
    assert info["faces"].dtype == torch.int32 and info["faces"].tolist() == faces
    assert info["seeds"] == list(KEYS)
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    if (kind, r) == ("closed2", 2):
        assert faces == [6, 24, 10]
    if kind == "closed3" and r in (3, 8):
        assert faces[0 if r == 3 else 1] == (54 if r == 3 else 66)
    if kind == "boundary":              # the clamp: the max face's points land in the last cell
        assert max(ref.voxel_indices(c, r).max() for c in x) == r - 1


def test_every_face_of_two_voxels_is_hit_on_the_device():
    from lion_amd.perturb import voxel_surface_points
    got, info = voxel_surface_points(_dev(TWO_VOXELS[None]), 2, 4096, seeds=[SEED])
    assert info["faces"].tolist() == [10]
    want, F, aux = ref.voxel_surface_points(TWO_VOXELS, 2, 4096, SEED)
    assert np.array_equal(_bits(got[0]), _bits(want))
    assert len({(tuple(v), int(f)) for v, f in zip(aux["voxel"], aux["face"])}) == 10


@pytest.mark.parametrize("N", [1, 5, 64, 2048, 2500])     # 2500: past the 8 x 256 points one pass of the outlier grid covers
@pytest.mark.parametrize("kind,amount", [("uniform", 0.05), ("uniform", 0.0), ("outlier", 0.0), ("outlier", 0.1),
                                         ("outlier", 0.5), ("outlier", 1.0)])
def test_uniform_and_outlier_equal_the_reference(kind, amount, N):
    from lion_amd.perturb import add_noise
    x = _batch("gauss", N, 0)
    xd = _dev(x)
    got = add_noise(xd, kind, amount, seeds=list(KEYS))
    assert got.shape == xd.shape and np.array_equal(_bits(xd), _bits(x))          # the input is not written
    for b in range(3):
        want, hit = ref.perturb_points(x[b], 0 if kind == "uniform" else 1, amount, KEYS[b])
        assert np.array_equal(_bits(got[b]), _bits(want)), (b, int((_bits(got[b]) != _bits(want)).sum()))
        if kind == "outlier" and amount in (0.0, 1.0):
            assert hit.all() if amount else not hit.any()


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


@pytest.mark.parametrize("N", [4, 64, 2048])
def test_normal_noise_is_the_forward_draw_with_unit_mean_factor(lion, N):
    """x + sigma*z with z the keyed draw DiffusionDiscretized.diffuse reports for these seeds: one product and one sum in float32,
    and the very call diffuse makes with m = 1"""
    from lion_amd import diffusion_ops
    from lion_amd.perturb import add_noise
    sigma = 0.02
    x = _batch("gauss", N, 0)
    xd = _dev(x)
    got = add_noise(xd, "normal", sigma, seeds=list(KEYS))
    _, z = lion.diffusion.diffuse(xd, 3, seeds=list(KEYS), return_noise=True)
    want = x + np.float32(sigma) * z.cpu().numpy()
    assert want.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))
    assert torch.equal(got, diffusion_ops.diffuse(xd, 1.0, sigma, seeds=list(KEYS)))


# ---- addressing --------------------------------------------------------------------------------------------------------------------
def _calls():
    from lion_amd.perturb import add_noise, voxel_surface_points
    return {"voxel": lambda x, **kw: voxel_surface_points(x, 8, 100, **kw)[0],
            "normal": lambda x, **kw: add_noise(x, "normal", 0.02, **kw),
            "uniform": lambda x, **kw: add_noise(x, "uniform", 0.05, **kw),
            "outlier": lambda x, **kw: add_noise(x, "outlier", 0.3, **kw)}


@pytest.mark.parametrize("what", ["voxel", "normal", "uniform", "outlier"])
def test_a_sample_is_addressed_by_its_seed(what):
    from lion_amd.sampling import shape_seeds
    f = _calls()[what]
    x = _dev(_batch("gauss", 64, 0))
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    full = f(x, seeds=list(KEYS))
    assert torch.equal(full, f(x, seeds=list(KEYS)))                               # the same seeds: the same bits
    for b in range(3):
        alone = f(x[b:b + 1].contiguous(), seeds=[KEYS[b]])                        # alone, B = 1
        assert torch.equal(alone[0], full[b]), (what, b)
    order = [2, 0, 1]                                                              # every sample first, last and in the middle
    moved = f(x[order].contiguous(), seeds=[KEYS[i] for i in order])
    for pos, b in enumerate(order):
        assert torch.equal(moved[pos], full[b]), (what, pos)
    mates = f(torch.cat([x[2:3] * 3.0, x[1:2], x[0:1] + 1.0, x[1:2]]).contiguous(), seeds=[KD, KB, KA, KB])   # other batchmates
    assert torch.equal(mates[1], full[1]) and torch.equal(mates[3], full[1])
    assert not torch.equal(full[0], f(x[0:1].contiguous(), seeds=[KB])[0])         # another seed: another draw
    assert torch.equal(f(x, seed=77), f(x, seeds=shape_seeds(77, 0, 3)))           # seed = s is seeds = shape_seeds(s, 0, B)
    assert torch.equal(f(x, seeds=torch.tensor([KA, KB, KC - 2 ** 64])), full)     # an int64 tensor, mod 2^64
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    torch.manual_seed(11)                                                          # neither: torch.manual_seed governs the call
    a = f(x)
    assert not torch.equal(torch.get_rng_state(), state[0])
    torch.manual_seed(11)
    assert torch.equal(a, f(x)) and not torch.equal(a, full)
    torch.set_rng_state(state[0])


def test_only_xyz_is_perturbed():
    from lion_amd.perturb import add_noise, voxel_surface_points
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.randn(3, 64, 6, device="cuda", generator=g)
    xyz = x[..., :3].contiguous()
    for kind, amount in (("normal", 0.02), ("uniform", 0.05), ("outlier", 0.3)):
        out = add_noise(x, kind, amount, seeds=list(KEYS))
        assert out.shape == x.shape and torch.equal(out[..., 3:], x[..., 3:])
        assert torch.equal(out[..., :3], add_noise(xyz, kind, amount, seeds=list(KEYS)))
    pts, _ = voxel_surface_points(x, 8, seeds=list(KEYS))
    assert tuple(pts.shape) == (3, 64, 3) and torch.equal(pts, voxel_surface_points(xyz, 8, 64, seeds=list(KEYS))[0])


def test_stream_ids_are_separate_streams():
    from lion_amd.perturb import voxel_surface_points
    x = _dev(_batch("gauss", 64, 0))
    a, _ = voxel_surface_points(x, 8, 100, seeds=list(KEYS), stream_id=1)
    want = np.stack([ref.voxel_surface_points(_batch("gauss", 64, 0)[b], 8, 100, KEYS[b], stream_id=1)[0] for b in range(3)])
    assert np.array_equal(_bits(a), _bits(want))
    assert not torch.equal(a, voxel_surface_points(x, 8, 100, seeds=list(KEYS))[0])


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
def test_calls_replay_from_a_captured_graph():
    """one linear capture of all four calls on device key words; the replay gives the eager bits, also for new data in x"""
    from lion_amd.chain import key_words
    from lion_amd.perturb import add_noise, voxel_surface_points
    x = _dev(_batch("gauss", 64, 0))
    words = key_words(list(KEYS), "cuda")

    def run():
        pts, info = voxel_surface_points(x, 8, 100, seeds=words)
        return [pts, info["faces"], add_noise(x, "normal", 0.02, seeds=words), add_noise(x, "uniform", 0.05, seeds=words),
                add_noise(x, "outlier", 0.3, seeds=words)]

    eager = [t.clone() for t in run()]
    assert torch.equal(eager[0], voxel_surface_points(x, 8, 100, seeds=list(KEYS))[0])     # device words are the ints' words
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, captured):
        assert torch.equal(a, b)
    x.copy_(_dev(_batch("shell", 64, 8)))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(run(), captured):
        assert torch.equal(a, b)
    assert not torch.equal(captured[0], eager[0])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_return_einval():
    from lion_amd import _lib
    out = torch.full((3, 100, 3), 7.0, device="cuda")
    for what, rc in einval_cases(_lib.load()):
        assert rc == -1, what
    # through _lib.call, with real tensors: the refusal raises and nothing is written
    x, words = _dev(_batch("gauss", 64, 0)), _dev(np.zeros((3, 2), np.int32))
    for args in ((x, 3, 64, 0, words, 0, 100, out, None, None, 0), (x, 3, 64, 33, words, 0, 100, out, None, None, 0),
                 (x, 3, 64, 8, words, 0, 0, out, None, None, 0), (x, 0, 64, 8, words, 0, 100, out, None, None, 0),
                 (x, 3, 0, 8, words, 0, 100, out, None, None, 0), (x, 3, 64, 8, None, 0, 100, out, None, None, 0)):
        with pytest.raises(RuntimeError, match="LION_EINVAL"):
            _lib.call("lion_voxel_surface_points_keyed", *args)
    for args in ((2, x, 3, 64, 0.1, words, 0, out), (0, x, 3, 64, -0.1, words, 0, out), (1, x, 3, 64, 1.5, words, 0, out)):
        with pytest.raises(RuntimeError, match="LION_EINVAL"):
            _lib.call("lion_perturb_points_keyed", *args)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- voxel-guided synthesis ------------------------------------------------------------------------------------------------------------
def test_voxel_guided_is_diffuse_denoise_on_the_voxel_surface_cloud(lion):
    from lion_amd.editing import diffuse_denoise, voxel_guided
    from lion_amd.perturb import voxel_surface_points
    g = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn(2, 2048, 3, device="cuda", generator=g) * 0.5
    seeds = [KA, KB]
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    points, info = voxel_guided(lion.vae, lion.priors, lion.diffusion, x, 16, (1, 2), seeds=seeds, graph=False)
    assert points.shape == x.shape and torch.isfinite(points).all()
    want_in, made = voxel_surface_points(x, 16, 2048, seeds=seeds)
    assert info["input"].shape == x.shape and torch.equal(info["input"], want_in)
    assert torch.equal(info["faces"], made["faces"]) and int(info["faces"].min()) >= 6
    by_hand, hand_info = diffuse_denoise(lion.vae, lion.priors, lion.diffusion, want_in, (1, 2), seeds=seeds, graph=False)
    assert torch.equal(points, by_hand)
    assert info["seeds"] == hand_info["seeds"] and info["time_start"] == (1, 2)
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])
    assert not torch.equal(info["input"], x)
