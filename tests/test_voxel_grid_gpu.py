"""-m gpu: voxel grids as inputs of guided synthesis and the voxel IoU.  The three new kernels of
csrc/perturb.hip against tests/voxel_grid_ref.py bit for bit (occupancy grids, frames and clamp counts; from-grid points and face
counts; IoU counts and quotients), the device's own consistency with the merged cloud kernel, addressing by sample, stream ids,
stream capture, the entry points' refusals, and editing.voxel_grid_guided / voxel_guided(iou=) on the released configuration
with a 12-step schedule.  B = 3 with three different clouds or grids and three keys unless a case says otherwise."""
import functools

import numpy as np
import pytest
import torch

import perturb_ref as pref
import voxel_grid_ref as ref
from test_perturb_gpu import KA, KB, KC, KD, KEYS, _batch, _bits, _dev, lion   # noqa: F401  (lion: the module's fixture)
from test_perturb_reference_cpu import SEED, TWO_VOXELS
from test_voxel_grid_reference_cpu import einval_cases

pytestmark = pytest.mark.gpu

FRAMES = np.array([[-1.0, -1.0, -1.0, 2.0], [0.3, -1.2, 2.5, 0.7], [-4.0, 5.0, 0.125, 3.0]], dtype=np.float32)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _grids(kind, r):
    """bool or uint8 [3, r, r, r], three different grids (computed once, never written afterwards)"""
    if kind == "random":               # sparse, half full, nearly full
        g = [ref.random_grid(r, 100 * r + b, d) for b, d in enumerate((0.1, 0.5, 0.95))]
    elif kind == "full":               # the full grid (r = 32: F = 6144, 1024 full words, bit 31 in use) beside two others
        g = [np.ones((r, r, r), bool), ref.random_grid(r, 7, 0.5), ref.corner_grid(r, 7)]
    elif kind == "checkerboard":       # every face of every occupied voxel is exposed; its complement; both at once = full
        g = [ref.checkerboard_grid(r), ~ref.checkerboard_grid(r), ref.random_grid(r, 8, 0.3)]
    elif kind == "empty":              # an empty grid between two non-empty ones
        g = [ref.random_grid(r, 9, 0.4), np.zeros((r, r, r), bool), ref.corner_grid(r, 5)]
    elif kind == "bytes":              # uint8: occupied voxels hold 2 or 255
        rng = np.random.default_rng(r)
        g = [np.where(ref.random_grid(r, 20 + b, 0.4), rng.choice([2, 255], size=(r, r, r)), 0).astype(np.uint8) for b in range(3)]
    g = np.stack(g)
    assert g.shape == (3, r, r, r)
    return g


@functools.lru_cache(maxsize=None)
def _ref_points(kind, r, K, stream_id=0):
    g = _grids(kind, r)
    pts, faces = zip(*[ref.surface_points_from_grid(g[b], FRAMES[b], K, KEYS[b], stream_id) for b in range(3)])
    return np.stack(pts), list(faces)


def _from_grid(g, K, frames=FRAMES, keys=KEYS, **kw):
    from lion_amd.perturb import voxel_surface_points_from_grid
    on_device = [_dev(t) if isinstance(t, np.ndarray) else t for t in (g, frames)]
    return voxel_surface_points_from_grid(*on_device, K, seeds=list(keys), **kw)


# ---- occupancy -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 7, 64, 2048])
@pytest.mark.parametrize("r", [1, 2, 3, 8, 16, 32])
def test_occupancy_in_the_own_frame_equals_the_reference(r, N):
    from lion_amd.perturb import voxel_occupancy
    x = _batch("gauss", N, 0)
    grid, info = voxel_occupancy(_dev(x), r)
    assert grid.dtype == torch.bool and tuple(grid.shape) == (3, r, r, r)
    assert info["frame"].dtype == torch.float32 and info["clamped"].dtype == torch.int32
    for b in range(3):
        want, frame, clamped = ref.occupancy(x[b], r)
        assert np.array_equal(_np(grid[b]), want), (b, int((_np(grid[b]) != want).sum()))
        assert np.array_equal(_bits(info["frame"][b]), _bits(frame)) and int(info["clamped"][b]) == clamped, b
    assert set(np.unique(_np(grid.view(torch.uint8)))) <= {0, 1}      # the memory of a bool tensor


@pytest.mark.parametrize("kind,N,r", [("shell", 2048, 16), ("boundary", 27, 8), ("boundary", 99, 32), ("closed2", 9, 2),
                                      ("closed3", 29, 3), ("closed3", 29, 8), ("gauss", 64, 5), ("gauss", 2048, 31)])
def test_occupancy_of_the_merged_suites_clouds(kind, N, r):
    from lion_amd.perturb import voxel_occupancy
    x = _batch(kind, N, r)
    grid, info = voxel_occupancy(_dev(x), r)
    for b in range(3):
        want, frame, clamped = ref.occupancy(x[b], r)
        assert np.array_equal(_np(grid[b]), want) and int(info["clamped"][b]) == clamped, b
        assert np.array_equal(_bits(info["frame"][b]), _bits(frame))
    if kind == "boundary":             # the max face's points are clamped inside their own frame
        assert int(info["clamped"].min()) > 0


@pytest.mark.parametrize("r", [3, 8, 32])
@pytest.mark.parametrize("how", ["half", "double", "host", "one for the batch"])
def test_occupancy_in_given_frames_that_cut_the_cloud(how, r):
    from lion_amd.perturb import voxel_occupancy
    x = _batch("gauss", 2048, 0)
    own = np.stack([ref.own_frame(c) for c in x])
    mid = own[:, :3] + own[:, 3:] * np.float32(0.5)
    scale = np.float32(0.5 if how == "half" else 2.0)
    side = own[:, 3:] * scale
    frames = np.concatenate([mid - side * np.float32(0.5), side], 1).astype(np.float32)
    if how == "one for the batch":
        frames = np.repeat(frames[1:2], 3, 0)
    given = _dev(frames) if how in ("half", "double") else frames[1].tolist() if how == "one for the batch" else frames.tolist()
    grid, info = voxel_occupancy(_dev(x), r, given)
    assert np.array_equal(_bits(info["frame"]), _bits(frames))
    counts = []
    for b in range(3):
        want, _, clamped = ref.occupancy(x[b], r, frames[b])
        assert np.array_equal(_np(grid[b]), want) and int(info["clamped"][b]) == clamped, (b, int(info["clamped"][b]), clamped)
        counts.append(clamped)
    if how == "half":
        assert min(counts) > 100        # many points lie beyond half the side
    if how == "double":
        assert counts == [0, 0, 0]


def test_occupancy_given_the_own_frame_is_the_own_frame():
    from lion_amd.perturb import voxel_occupancy
    for kind, N, r in (("gauss", 2048, 32), ("boundary", 51, 16), ("shell", 2048, 16), ("closed2", 9, 2)):
        x = _dev(_batch(kind, N, r))
        grid, info = voxel_occupancy(x, r)
        again, info2 = voxel_occupancy(x, r, info["frame"])
        assert torch.equal(grid, again) and torch.equal(info["clamped"], info2["clamped"])
        assert np.array_equal(_bits(info["frame"]), _bits(info2["frame"]))


# ---- from grid -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 100, 2048, 4096])       # 2048, 4096: above the 1024 points one pass of the workgroup draws
@pytest.mark.parametrize("r", [1, 2, 3, 8, 16, 32])
def test_points_from_grids_equal_the_reference(r, K):
    want, faces = _ref_points("random", r, K)
    got, info = _from_grid(_grids("random", r), K)
    assert tuple(got.shape) == (3, K, 3) and got.dtype == torch.float32
    assert info["faces"].dtype == torch.int32 and info["faces"].tolist() == faces
    assert info["seeds"] == list(KEYS) and np.array_equal(_bits(info["frame"]), _bits(FRAMES))
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


@pytest.mark.parametrize("kind,r,K", [("full", 32, 2048), ("full", 3, 2048), ("full", 1, 100), ("checkerboard", 8, 2048),
                                      ("empty", 8, 100), ("empty", 32, 2048), ("empty", 5, 100), ("bytes", 5, 2048),
                                      ("bytes", 8, 2048), ("bytes", 32, 100), ("random", 5, 100), ("random", 7, 2048),
                                      ("random", 31, 4096), ("random", 4, 100)])
def test_points_from_special_grids_equal_the_reference(kind, r, K):
    g = _grids(kind, r)
    want, faces = _ref_points(kind, r, K)
    got, info = _from_grid(g, K)
    assert info["faces"].tolist() == faces
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())
    if kind == "full":
        assert faces[0] == 6 * r * r and (r < 3 or faces[2] == 6)     # r = 32: 6144; the solid 3^3 block: 54
    if kind == "checkerboard":
        assert faces[0] == 6 * int(g[0].sum()) and faces[0] + faces[1] == 6 * r ** 3
    if kind == "empty":                # no face: every point is the frame's centre
        centre = FRAMES[1, :3] + FRAMES[1, 3] * np.float32(0.5)
        assert faces[1] == 0 and faces[0] > 0 and faces[2] == 6
        assert np.array_equal(_bits(got[1]), _bits(np.tile(centre, (K, 1))))
    if kind == "bytes":                # any non-zero byte is an occupied voxel
        assert g.dtype == np.uint8 and set(np.unique(g)) == {0, 2, 255}
        as_bool, info_bool = _from_grid(g != 0, K)
        assert torch.equal(got, as_bool) and torch.equal(info["faces"], info_bool["faces"])


def test_a_single_voxel_at_each_corner():
    keys = [KA, KB, KC, KD, KA + 1, KB + 1, KC + 1, KD - 1]
    g = np.stack([ref.corner_grid(32, c) for c in range(8)])
    frames = np.repeat(FRAMES, 3, 0)[:8]
    got, info = _from_grid(g, 100, frames, keys)
    assert info["faces"].tolist() == [6] * 8
    for c in range(8):
        want, F = ref.surface_points_from_grid(g[c], frames[c], 100, keys[c])
        assert F == 6 and np.array_equal(_bits(got[c]), _bits(want)), c


def test_unit_frame_is_the_default_and_host_frames_are_uploaded():
    from lion_amd.perturb import UNIT_FRAME, voxel_surface_points_from_grid
    g = _dev(_grids("random", 8))
    a, info = voxel_surface_points_from_grid(g, seeds=list(KEYS))
    assert tuple(a.shape) == (3, 2048, 3) and UNIT_FRAME == (-1.0, -1.0, -1.0, 2.0)
    assert np.array_equal(_bits(info["frame"]), _bits(np.tile(ref.UNIT_FRAME, (3, 1))))
    for b in range(3):
        assert np.array_equal(_bits(a[b]), _bits(ref.surface_points_from_grid(_grids("random", 8)[b], ref.UNIT_FRAME, 2048, KEYS[b])[0]))
    assert float(a.min()) >= -1.0 and float(a.max()) <= 1.0
    b_, _ = voxel_surface_points_from_grid(g, FRAMES.tolist(), 100, seeds=list(KEYS))
    assert torch.equal(b_, _from_grid(g, 100)[0])
    c_, _ = voxel_surface_points_from_grid(g, torch.from_numpy(FRAMES[2]), 100, seeds=list(KEYS))
    assert torch.equal(c_, _from_grid(g, 100, np.repeat(FRAMES[2:3], 3, 0))[0])


def test_a_grid_that_is_not_dword_aligned_moves_by_bytes():
    """r % 4 == 0 grids move by dwords when their base is 4-byte aligned; one byte further they move by bytes, to the same bits"""
    from lion_amd.metrics import voxel_iou
    from lion_amd.perturb import voxel_surface_points_from_grid
    for r in (8, 32):
        g = _grids("bytes", r)
        flat = torch.zeros(3 * r ** 3 + 1, dtype=torch.uint8, device="cuda")
        flat[1:] = _dev(g).view(-1)
        odd = flat[1:].view(3, r, r, r)
        assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
        got, info = voxel_surface_points_from_grid(odd, _dev(FRAMES), 100, seeds=list(KEYS))
        want, faces = _ref_points("bytes", r, 100)
        assert info["faces"].tolist() == faces and np.array_equal(_bits(got), _bits(want))
        other = _dev(_grids("random", r))
        for a, b in ((odd, other), (other, odd), (odd, odd)):        # unequal alignments: all bytes; equal: 15 bytes, then 16 at a time
            value, m = voxel_iou(a, b)
            for s in range(3):
                assert (float(value[s]), int(m["intersection"][s]), int(m["union"][s])) == ref.iou(_np(a[s]), _np(b[s])), (r, s)


# ---- the device's own consistency: the new kernels against the merged one ---------------------------------------------------------
@pytest.mark.parametrize("kind,N,r,K", [("gauss", 1, 1, 1), ("gauss", 7, 2, 100), ("gauss", 64, 8, 100), ("gauss", 2048, 16, 2048),
                                        ("gauss", 2048, 32, 4096), ("gauss", 2048, 31, 2048), ("shell", 2048, 16, 2048),
                                        ("shell", 64, 3, 4096), ("boundary", 27, 8, 100), ("boundary", 99, 32, 4096),
                                        ("closed2", 9, 2, 4096), ("closed3", 29, 3, 2048), ("closed3", 29, 8, 2048)])
def test_occupancy_then_from_grid_is_voxel_surface_points(kind, N, r, K):
    from lion_amd.perturb import voxel_occupancy, voxel_surface_points, voxel_surface_points_from_grid
    x = _dev(_batch(kind, N, r))
    want, made = voxel_surface_points(x, r, K, seeds=list(KEYS))
    grid, occ = voxel_occupancy(x, r)
    got, info = voxel_surface_points_from_grid(grid, occ["frame"], K, seeds=list(KEYS))
    assert torch.equal(info["faces"], made["faces"]) and int(info["faces"].min()) >= 6
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


# ---- IoU -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 3, 5, 16, 32])
def test_iou_of_random_grids(r):
    from lion_amd.metrics import voxel_iou
    a, b = _grids("random", r), _grids("bytes" if r > 1 else "full", r)
    value, m = voxel_iou(_dev(a), _dev(b))
    assert value.dtype == torch.float32 and m["intersection"].dtype == torch.int32 and m["clamped"] == (None, None)
    for s in range(3):
        want, inter, union = ref.iou(a[s], b[s])
        assert inter == int(((a[s] != 0) & (b[s] != 0)).sum()) and union == int(((a[s] != 0) | (b[s] != 0)).sum())
        assert (int(m["intersection"][s]), int(m["union"][s])) == (inter, union), (r, s)
        assert _bits(value[s]) == _bits(want)
    assert torch.equal(m["counts"], torch.stack([m["intersection"], m["union"]], 1))
    same, ms = voxel_iou(_dev(a), _dev(a))
    assert torch.equal(ms["intersection"], ms["union"]) and all(v == 1.0 for v in same.tolist())
    none, mn = voxel_iou(_dev(a != 0), _dev(a == 0))                  # disjoint: 0 of r^3
    assert none.tolist() == [0.0] * 3 and mn["intersection"].tolist() == [0] * 3 and mn["union"].tolist() == [r ** 3] * 3


def test_iou_edges_and_the_hand_counted_case():
    from lion_amd.metrics import voxel_iou
    from lion_amd.perturb import voxel_occupancy
    empty = torch.zeros(3, 4, 4, 4, dtype=torch.bool, device="cuda")
    value, m = voxel_iou(empty, empty)
    assert value.tolist() == [1.0] * 3 and m["counts"].tolist() == [[0, 0]] * 3
    x = _dev(TWO_VOXELS[None])
    grid, info = voxel_occupancy(x, 2)
    assert info["frame"].tolist() == [[0.0, -0.5, -0.5, 1.0]] and int(grid.sum()) == 2 and info["clamped"].tolist() == [1]
    origin = torch.zeros(1, 1, 3, device="cuda")
    value, m = voxel_iou(grid, origin, frame=info["frame"])           # a grid and a cloud: two launches
    assert value.tolist() == [0.5] and m["counts"].tolist() == [[1, 2]] and m["clamped"][0] is None
    assert m["clamped"][1].tolist() == [0]
    value, m = voxel_iou(x, origin, 2)                                # two clouds: the first one's own frame serves both
    assert value.tolist() == [0.5] and m["counts"].tolist() == [[1, 2]] and m["frame"].tolist() == [[0.0, -0.5, -0.5, 1.0]]
    assert [c.tolist() for c in m["clamped"]] == [[1], [0]]
    value, m = voxel_iou(origin, grid)                                # a cloud and a grid: the cloud's own frame
    assert m["frame"].tolist() == [[-1.0, -1.0, -1.0, 2.0]] and m["counts"].tolist() == [[1, 2]]
    for kind, N, r in (("shell", 2048, 16), ("gauss", 64, 5)):        # IoU(x, x) = 1
        c = _dev(_batch(kind, N, r))
        value, m = voxel_iou(c, c, r)
        assert value.tolist() == [1.0] * 3 and torch.equal(m["intersection"], m["union"])
        assert torch.equal(m["clamped"][0], m["clamped"][1])


@pytest.mark.parametrize("r,how", [(16, "device"), (32, "device"), (5, "host")])
def test_iou_of_a_cloud_and_its_own_from_grid_points(r, how):
    """the points drawn on a cloud's voxel surface, voxelised again in the cloud's frame: against the reference voxelisation"""
    from lion_amd.metrics import voxel_iou
    from lion_amd.perturb import voxel_occupancy, voxel_surface_points_from_grid
    x = _batch("gauss", 2048, 0)
    grid, occ = voxel_occupancy(_dev(x), r)
    pts, _ = voxel_surface_points_from_grid(grid, occ["frame"], 2048, seeds=list(KEYS))
    frame = occ["frame"] if how == "device" else occ["frame"].cpu().tolist()
    value, m = voxel_iou(grid, pts, frame=frame)
    by_cloud, mc = voxel_iou(_dev(x), pts, r)                         # three launches: the same voxels
    assert torch.equal(value, by_cloud) and torch.equal(m["counts"], mc["counts"])
    for b in range(3):
        again, _, clamped = ref.occupancy(_np(pts[b]), r, _np(occ["frame"][b]))
        want, inter, union = ref.iou(_np(grid[b]), again)
        assert (int(m["intersection"][b]), int(m["union"][b])) == (inter, union) and _bits(value[b]) == _bits(want)
        assert int(m["clamped"][1][b]) == clamped
        assert 0 < inter <= union


# ---- addressing ------------------------------------------------------------------------------------------------------------------------
def test_a_sample_is_addressed_by_its_seed_and_its_own_bytes():
    """a sample alone, first or last of a batch gives the same bits: r = 5 (a sample's 125 bytes start on no boundary) and 8"""
    from lion_amd.metrics import voxel_iou
    from lion_amd.perturb import voxel_occupancy
    x = _dev(_batch("gauss", 64, 0))
    for r in (5, 8):
        g, h = _dev(_grids("random", r)), _dev(_grids("bytes", r))
        frames = _dev(FRAMES)
        full, info = _from_grid(g, 100)
        occ, oinfo = voxel_occupancy(x, r, frames)
        value, m = voxel_iou(g, h)
        for order in ([0], [1], [2], [2, 0, 1], [1, 2, 0]):
            sel = lambda t: t[order].contiguous()
            got, ginfo = _from_grid(sel(g), 100, sel(frames), [KEYS[i] for i in order])
            assert torch.equal(got, full[order]) and torch.equal(ginfo["faces"], info["faces"][order]), (r, order)
            o2, i2 = voxel_occupancy(sel(x), r, sel(frames))
            assert torch.equal(o2, occ[order]) and torch.equal(i2["clamped"], oinfo["clamped"][order])
            v2, m2 = voxel_iou(sel(g), sel(h))
            assert torch.equal(v2, value[order]) and torch.equal(m2["counts"], m["counts"][order])
        assert not torch.equal(full[0], _from_grid(g[0:1].contiguous(), 100, frames[0:1].contiguous(), [KB])[0][0])
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    from lion_amd.perturb import voxel_surface_points_from_grid
    from lion_amd.sampling import shape_seeds
    g = _dev(_grids("random", 8))
    assert torch.equal(voxel_surface_points_from_grid(g, None, 64, seed=77)[0],
                       voxel_surface_points_from_grid(g, None, 64, seeds=shape_seeds(77, 0, 3))[0])
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])


def test_stream_ids_are_separate_streams():
    g = _grids("random", 8)
    a, _ = _from_grid(g, 100, stream_id=1)
    assert np.array_equal(_bits(a), _bits(_ref_points("random", 8, 100, 1)[0]))
    assert not torch.equal(a, _from_grid(g, 100)[0])


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
def test_calls_replay_from_a_captured_graph():
    """one linear capture of the three launches on device key words and device frames; the replay gives the eager bits, also
    for new data in x"""
    from lion_amd.chain import key_words
    from lion_amd.metrics import voxel_iou
    from lion_amd.perturb import voxel_occupancy, voxel_surface_points_from_grid
    x = _dev(_batch("gauss", 64, 0))
    words = key_words(list(KEYS), "cuda")

    def run():
        grid, occ = voxel_occupancy(x, 8)
        pts, info = voxel_surface_points_from_grid(grid, occ["frame"], 100, seeds=words)
        value, m = voxel_iou(grid, pts, frame=occ["frame"])
        return [grid, occ["frame"], occ["clamped"], pts, info["faces"], value, m["counts"], m["clamped"][1]]

    eager = [t.clone() for t in run()]
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
    assert not torch.equal(captured[3], eager[3])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_return_einval():
    from lion_amd import _lib
    for what, rc in einval_cases(_lib.load()):
        assert rc == -1, what
    # through _lib.call, with real tensors: the refusal raises and nothing is written
    out = torch.full((3, 100, 3), 7.0, device="cuda")
    g, frames, words = _dev(_grids("random", 8)), _dev(FRAMES), _dev(np.zeros((3, 2), np.int32))
    for args in ((g, frames, 3, 0, words, 0, 100, out, None), (g, frames, 3, 33, words, 0, 100, out, None),
                 (g, frames, 3, 8, words, 0, 0, out, None), (g, frames, 0, 8, words, 0, 100, out, None),
                 (g, None, 3, 8, words, 0, 100, out, None), (g, frames, 3, 8, None, 0, 100, out, None)):
        with pytest.raises(RuntimeError, match="LION_EINVAL"):
            _lib.call("lion_voxel_surface_points_grid_keyed", *args)
    with pytest.raises(RuntimeError, match="LION_EINVAL"):
        _lib.call("lion_voxel_occupancy", out, 3, 100, 33, None, g, None, None)
    with pytest.raises(RuntimeError, match="LION_EINVAL"):
        _lib.call("lion_voxel_iou", g, g, 3, 0, out, None)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and np.array_equal(_np(g), _grids("random", 8))


# ---- voxel-guided synthesis from a grid, and the IoU of input and output -------------------------------------------------------------
def test_voxel_grid_guided_is_diffuse_denoise_on_the_from_grid_cloud(lion):   # noqa: F811
    from lion_amd.editing import diffuse_denoise, voxel_grid_guided
    from lion_amd.metrics import voxel_iou
    from lion_amd.perturb import voxel_surface_points_from_grid
    grid = _dev(_grids("random", 16)[:2])
    frames = _dev(FRAMES[:2])
    seeds = [KA, KB]
    state = torch.get_rng_state(), torch.cuda.get_rng_state()
    points, info = voxel_grid_guided(lion.vae, lion.priors, lion.diffusion, grid, (1, 2), frames, iou=True, seeds=seeds,
                                     graph=False)
    assert tuple(points.shape) == (2, 2048, 3) and torch.isfinite(points).all()
    want_in, made = voxel_surface_points_from_grid(grid, frames, 2048, seeds=seeds)
    assert torch.equal(info["input"], want_in) and torch.equal(info["faces"], made["faces"])
    assert info["input grid"] is grid and torch.equal(info["frame"], frames)
    by_hand, hand_info = diffuse_denoise(lion.vae, lion.priors, lion.diffusion, want_in, (1, 2), seeds=seeds, graph=False)
    assert torch.equal(points, by_hand) and info["seeds"] == hand_info["seeds"] and info["time_start"] == (1, 2)
    value, m = voxel_iou(info["input grid"], points, frame=info["frame"])
    assert torch.equal(info["iou"], value) and torch.equal(info["iou_counts"], m["counts"])
    assert tuple(info["iou"].shape) == (2,) and bool(((info["iou"] >= 0) & (info["iou"] <= 1)).all())
    plain, plain_info = voxel_grid_guided(lion.vae, lion.priors, lion.diffusion, grid, (1, 2), frames, seeds=seeds, graph=False)
    assert torch.equal(plain, points) and set(info) - set(plain_info) == {"iou", "iou_counts"}
    assert torch.equal(torch.get_rng_state(), state[0]) and torch.equal(torch.cuda.get_rng_state(), state[1])


def test_voxel_guided_reports_the_iou_only_when_asked(lion):   # noqa: F811
    from lion_amd.editing import diffuse_denoise, voxel_guided
    from lion_amd.metrics import voxel_iou
    from lion_amd.perturb import voxel_occupancy, voxel_surface_points
    g = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn(2, 2048, 3, device="cuda", generator=g) * 0.5
    seeds = [KA, KB]
    points, info = voxel_guided(lion.vae, lion.priors, lion.diffusion, x, 16, (1, 2), iou=False, seeds=seeds, graph=False)
    want_in, made = voxel_surface_points(x, 16, 2048, seeds=seeds)
    by_hand, hand_info = diffuse_denoise(lion.vae, lion.priors, lion.diffusion, want_in, (1, 2), seeds=seeds, graph=False)
    assert torch.equal(points, by_hand) and torch.equal(info["input"], want_in) and torch.equal(info["faces"], made["faces"])
    assert set(info) == set(hand_info) | {"input", "faces"}           # the keys of before
    default, default_info = voxel_guided(lion.vae, lion.priors, lion.diffusion, x, 16, (1, 2), seeds=seeds, graph=False)
    assert torch.equal(default, points) and set(default_info) == set(info)
    measured, with_iou = voxel_guided(lion.vae, lion.priors, lion.diffusion, x, 16, (1, 2), iou=True, seeds=seeds, graph=False)
    assert torch.equal(measured, points) and set(with_iou) - set(info) == {"iou", "iou_counts", "input grid", "frame"}
    grid, occ = voxel_occupancy(x, 16)
    value, m = voxel_iou(grid, points, frame=occ["frame"])
    assert torch.equal(with_iou["input grid"], grid) and torch.equal(with_iou["frame"], occ["frame"])
    assert torch.equal(with_iou["iou"], value) and torch.equal(with_iou["iou_counts"], m["counts"])
