"""-m gpu: what the coordinates alone decide about a forward pass -- the voxel index plan, the tile occupancy per
consumer-aware level, the r = 32 devoxelisation plan -- is computed once per (cloud, resolution) pair inside
pvcnn2_ada.voxel_plans() and once per use outside it.  Counted at the C entry points (a spy on lion_amd._lib.call) against
what forward pre-hooks on the PVConvs saw; every result is compared bit for bit with an evaluation that shares nothing."""
import pytest
import torch

from conftest import fill_

pytestmark = pytest.mark.gpu

INDEX = "lion_voxel_index"
SCATTER, SCATTER_READ = "lion_voxel_scatter", "lion_voxel_scatter_read"
ONE_LAUNCH = "lion_voxelize_points_forward"
OCCUPANCY = "lion_conv3d_tile_occupancy_aware"
DEVOX_PLAN, DEVOX_PLANNED = "lion_trilinear_devoxelize_plan", "lion_trilinear_devoxelize_planned_forward"
DEVOX_AFFINE = "lion_trilinear_devoxelize_affine_forward"
GEOMETRY_ENTRIES = (INDEX, SCATTER, SCATTER_READ, ONE_LAUNCH, OCCUPANCY, DEVOX_PLAN)


def spy_on_calls(mp):
    """names of the C entry points launched from here on, in order"""
    from lion_amd import _lib
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)
    mp.setattr(_lib, "call", spy)
    return names


@pytest.fixture()
def calls(monkeypatch):
    return spy_on_calls(monkeypatch)


# ---------------------------------------------------------------- one denoiser forward

@pytest.fixture(scope="module")
def denoiser():
    from lion_amd.config import released_prior_cfg
    from lion_amd.models.latent_points_ada_localprior import PVCNN2Prior
    cfg = released_prior_cfg()
    loc = PVCNN2Prior(cfg.sde, 1, cfg)
    fill_(loc)
    loc.cuda().eval()
    B = 2
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, loc.num_points * loc.num_classes, 1, 1, device="cuda", generator=g)
    t = torch.rand(B, device="cuda", generator=g)
    cond = torch.randn(B, 128, 1, 1, device="cuda", generator=g)
    return loc, x, t, cond


def forward(denoiser, mp, **switches):
    """one eager forward with the three plans on except where `switches` says otherwise -> (output, entry-point names,
    [(coords address, resolution, consumer-aware level)] of the PVConv calls in order)"""
    from lion_amd.models import pvcnn2_ada as m
    loc, x, t, cond = denoiser
    for name, on in {"VOX_PLAN": True, "OCC_PLAN": True, "DEVOX_PLAN": True, "OCC_CLONE": False, **switches}.items():
        mp.setattr(m, name, on)
    seen = []

    def hook(mod, args):
        coords = args[0][1]
        # the address the hook sees is the one the forward's cache is keyed on only for coordinates used as they are
        assert coords.shape[1] == 3 and coords.dtype == torch.float32 and coords.is_contiguous()
        seen.append((coords.data_ptr(), mod.resolution, mod._aware_level()))

    handles = [mod.register_forward_pre_hook(hook) for mod in loc.modules() if isinstance(mod, m.PVConv)]
    names = spy_on_calls(mp)
    try:
        with torch.no_grad():
            out = loc(x, t, condition_input=cond).clone()
    finally:
        for h in handles:
            h.remove()
    return out, list(names), seen


@pytest.fixture(scope="module")
def all_on(denoiser):
    with pytest.MonkeyPatch.context() as mp:
        return forward(denoiser, mp)


def test_census_of_one_denoiser_forward(all_on):
    """index plan, occupancy and devoxelisation plan once per pair (and level), one scatter per PVConv"""
    out, names, seen = all_on
    P = len(seen)
    print("PVConv calls (address, r, level):", seen)
    print({n: names.count(n) for n in GEOMETRY_ENTRIES + (DEVOX_PLANNED, DEVOX_AFFINE)})
    assert P > 0 and torch.isfinite(out).all()
    assert names.count(INDEX) == len({(p, r) for p, r, _ in seen})
    assert len({(p, r) for p, r, _ in seen}) < P          # the forward does come back to its clouds
    assert names.count(SCATTER) + names.count(SCATTER_READ) == P
    assert names.count(ONE_LAUNCH) == 0
    assert names.count(OCCUPANCY) == len({(p, r, lv) for p, r, lv in seen if r >= 16})
    assert names.count(DEVOX_PLAN) == len({(p, r) for p, r, _ in seen if r == 32})
    assert names.count(DEVOX_PLANNED) == sum(r == 32 for _, r, _ in seen)
    assert names.count(DEVOX_AFFINE) == P - names.count(DEVOX_PLANNED)


def test_forward_without_index_plans(denoiser, all_on, monkeypatch):
    """VOX_PLAN off: no scope, so every voxelisation is the single launch, every sparse PVConv computes its occupancy in
    front of its first convolution, and no devoxelisation is planned.  Bit-identical output."""
    out, names, seen = forward(denoiser, monkeypatch, VOX_PLAN=False)
    P = len(seen)
    assert [s[1:] for s in seen] == [s[1:] for s in all_on[2]]
    assert not {INDEX, SCATTER, SCATTER_READ, DEVOX_PLAN, DEVOX_PLANNED} & set(names)
    assert names.count(ONE_LAUNCH) == P
    assert names.count(OCCUPANCY) == sum(r >= 16 for _, r, _ in seen)
    assert names.count(DEVOX_AFFINE) == P
    print("VOX_PLAN off: max |difference|", (out - all_on[0]).abs().max().item())
    assert torch.equal(out, all_on[0])


def test_forward_without_shared_occupancy(denoiser, all_on, monkeypatch):
    """OCC_PLAN off: the occupancy is launched once per use -- a PVConv whose scatter is reader-aware (level non-zero,
    r in (16, 32)) uses it twice, for the scatter and for the convolutions.  Bit-identical output."""
    out, names, seen = forward(denoiser, monkeypatch, OCC_PLAN=False)
    assert [s[1:] for s in seen] == [s[1:] for s in all_on[2]]
    assert names.count(OCCUPANCY) == sum((2 if lv and r in (16, 32) else 1) for _, r, lv in seen if r >= 16)
    assert names.count(OCCUPANCY) > all_on[1].count(OCCUPANCY)
    for n in (INDEX, SCATTER, SCATTER_READ, ONE_LAUNCH, DEVOX_PLAN, DEVOX_PLANNED, DEVOX_AFFINE):
        assert names.count(n) == all_on[1].count(n), n
    print("OCC_PLAN off: max |difference|", (out - all_on[0]).abs().max().item())
    assert torch.equal(out, all_on[0])


def test_forward_without_devoxelisation_plans(denoiser, all_on, monkeypatch):
    """DEVOX_PLAN off: every devoxelisation is the one-step form.  Bit-identical output."""
    out, names, seen = forward(denoiser, monkeypatch, DEVOX_PLAN=False)
    assert not {DEVOX_PLAN, DEVOX_PLANNED} & set(names)
    assert names.count(DEVOX_AFFINE) == len(seen)
    for n in (INDEX, SCATTER, SCATTER_READ, ONE_LAUNCH, OCCUPANCY):
        assert names.count(n) == all_on[1].count(n), n
    print("DEVOX_PLAN off: max |difference|", (out - all_on[0]).abs().max().item())
    assert torch.equal(out, all_on[0])


# ---------------------------------------------------------------- small PVConvs: which calls share what

B, C = 2, 32


def make_pv(r, seed=0):
    from lion_amd.config import released_prior_cfg
    from lion_amd.models import pvcnn2_ada as m
    pv = m.PVConv(C, C, 3, r, with_se=True, cfg=released_prior_cfg())
    fill_(pv, seed)
    return pv.cuda().eval()


def cloud(n, seed, channels=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(B, channels, n, device="cuda", generator=g)


def operands(n, seed=0):
    g = torch.Generator(device="cuda").manual_seed(100 + seed)
    return torch.randn(B, C, n, device="cuda", generator=g), torch.randn(B, 128, device="cuda", generator=g)


def run(pv, feat, coords, sty):
    return pv((feat, coords, None, sty))[0].clone()


def alone(pv, feat, coords, sty):
    """the same call in a scope of its own"""
    from lion_amd.models import pvcnn2_ada as m
    with m.voxel_plans():
        return run(pv, feat, coords, sty)


@pytest.fixture(autouse=True)
def plans_on(monkeypatch):
    from lion_amd.models import pvcnn2_ada as m
    for name, on in (("VOX_PLAN", True), ("OCC_PLAN", True), ("DEVOX_PLAN", True), ("OCC_CLONE", False),
                     ("SKIP_UNREAD", True), ("SKIP_UNREAD_LEVEL2", True)):
        monkeypatch.setattr(m, name, on)
    with torch.no_grad():
        yield


def geometry_calls(names):
    return [n for n in names if n in GEOMETRY_ENTRIES]


def test_one_cloud_at_two_resolutions_is_two_pairs(calls):
    from lion_amd.models import pvcnn2_ada as m
    n = 512
    pv16, pv32, pv32b = make_pv(16), make_pv(32), make_pv(32, seed=1)
    coords, (feat, sty) = cloud(n, 1), operands(n)
    want = [alone(pv, feat, coords, sty) for pv in (pv16, pv32, pv32b)]
    del calls[:]
    with m.voxel_plans():
        got = [run(pv, feat, coords, sty) for pv in (pv16, pv32, pv32b)]
    assert calls.count(INDEX) == 2 and calls.count(OCCUPANCY) == 2          # (coords, 16) and (coords, 32)
    assert calls.count(DEVOX_PLAN) == 1 and calls.count(DEVOX_PLANNED) == 2 and calls.count(DEVOX_AFFINE) == 1
    assert calls.count(SCATTER) + calls.count(SCATTER_READ) == 3 and calls.count(ONE_LAUNCH) == 0
    for g, w in zip(got, want):
        assert torch.isfinite(g).all() and torch.equal(g, w)


def test_two_levels_share_the_index_plan_but_not_the_occupancy(calls, monkeypatch):
    from lion_amd import conv_ops
    from lion_amd.models import pvcnn2_ada as m
    n, r = 256, 16
    pv_a, pv_b = make_pv(r), make_pv(r, seed=1)
    coords, (feat, sty) = cloud(n, 2), operands(n)
    monkeypatch.setattr(conv_ops, "SPLIT", True)
    level_a, want_a = pv_a._aware_level(), alone(pv_a, feat, coords, sty)
    monkeypatch.setattr(conv_ops, "SPLIT", False)
    level_b, want_b = pv_b._aware_level(), alone(pv_b, feat, coords, sty)
    assert (level_a, level_b) == (2, 1)
    del calls[:]
    with m.voxel_plans():
        monkeypatch.setattr(conv_ops, "SPLIT", True)
        got_a = run(pv_a, feat, coords, sty)
        assert geometry_calls(calls) == [INDEX, OCCUPANCY, SCATTER_READ]     # reader-aware: the occupancy comes first
        monkeypatch.setattr(conv_ops, "SPLIT", False)
        got_b = run(pv_b, feat, coords, sty)
        assert geometry_calls(calls) == [INDEX, OCCUPANCY, SCATTER_READ, OCCUPANCY, SCATTER_READ]
        monkeypatch.setattr(conv_ops, "SPLIT", True)
        again_a = run(pv_a, feat, coords, sty)                               # both levels are there now
        assert geometry_calls(calls) == [INDEX, OCCUPANCY, SCATTER_READ, OCCUPANCY, SCATTER_READ, SCATTER_READ]
    assert torch.equal(got_a, want_a) and torch.equal(again_a, want_a) and torch.equal(got_b, want_b)


def test_six_channel_coordinates_never_hit(calls):
    """[B,6,N] coordinates: the [:, :3] slice is copied to a new tensor on every call, so no two calls share a pair"""
    from lion_amd.models import pvcnn2_ada as m
    n, r = 256, 16
    pv = make_pv(r)
    coords6, (feat, sty) = cloud(n, 3, channels=6), operands(n)
    want = alone(pv, feat, coords6[:, :3].contiguous(), sty)
    del calls[:]
    with m.voxel_plans():
        got = [run(pv, feat, coords6, sty) for _ in range(2)]
    assert calls.count(INDEX) == 2 and calls.count(OCCUPANCY) == 2
    assert torch.equal(got[0], want) and torch.equal(got[1], want)


def test_a_freed_cloud_does_not_lend_its_plan_to_the_next(calls):
    """a cloud deleted by its owner inside a scope and another one of the same shape allocated right after"""
    from lion_amd.models import pvcnn2_ada as m
    n, r = 256, 16
    pv = make_pv(r)
    feat, sty = operands(n)
    want_b = alone(pv, feat, cloud(n, 5), sty)
    del calls[:]
    with m.voxel_plans():
        a = cloud(n, 4)
        got_a = run(pv, feat, a, sty)
        del a
        b = cloud(n, 5)
        got_b = run(pv, feat, b, sty)
    assert calls.count(INDEX) == 2
    assert torch.equal(got_b, want_b) and not torch.equal(got_a, got_b)


def test_a_nested_scope_has_its_own_cache(calls):
    from lion_amd.models import pvcnn2_ada as m
    n, r = 256, 16
    pv = make_pv(r)
    coords, (feat, sty) = cloud(n, 6), operands(n)
    want = alone(pv, feat, coords, sty)
    del calls[:]
    with m.voxel_plans():
        outer = run(pv, feat, coords, sty)
        assert calls.count(INDEX) == 1
        with m.voxel_plans():
            inner = run(pv, feat, coords, sty)
            assert calls.count(INDEX) == 2 and calls.count(OCCUPANCY) == 2
        back = run(pv, feat, coords, sty)
        assert calls.count(INDEX) == 2 and calls.count(OCCUPANCY) == 2      # the outer scope's record is still there
    assert all(torch.equal(o, want) for o in (outer, inner, back))


@pytest.mark.parametrize("r,n", [(16, 256), (32, 512)])
def test_outside_a_scope_nothing_is_kept(calls, r, n):
    pv = make_pv(r)
    coords, (feat, sty) = cloud(n, 7), operands(n)
    want = alone(pv, feat, coords, sty)
    del calls[:]
    got = [run(pv, feat, coords, sty) for _ in range(2)]
    assert geometry_calls(calls) == [ONE_LAUNCH, OCCUPANCY] * 2             # the occupancy in front of conv1
    assert calls.count(DEVOX_AFFINE) == 2 and calls.count(DEVOX_PLANNED) == 0
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
