"""CPU: the plan, case table, bounds and emulation of tests/conv3d_split_ref.py.  The plan against what the library reports
(host calls); the numpy emulation of the split kernels' arithmetic inside the derived elementwise bound on every dynamic-
range case, at emulated tiles of r = 8 -- so the bound is known to be satisfiable before any GPU run; each seeded defect of the
emulation OUTSIDE the bound on named cases -- so the bound is known to be sharp enough to matter; every case of the table on
the path it names, by the restated plan; and the hand-built clouds with the tile flags they are named for."""
import numpy as np
import pytest
import torch

import conv3d_ref as cr
import conv3d_split_ref as sr

R_EMU, COUT_EMU = 8, 8
EMU_TILES = ((4, 8), (4, 4))     # the r = 8 kernel's half-sample tile, and a 4 x 4 x r tile with halos on every side


def data(cin, cout, r, B, seed):
    torch.manual_seed(seed)
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1)
    x = torch.randn(B, cin, r, r, r)
    pro = (torch.rand(B, cin) + 0.5, torch.randn(B, cin) * 0.5)
    return x, conv.weight.detach(), conv.bias.detach(), pro


def conv64_tiled(x, w, bias, pro, tile):
    """sr.conv64: its floor term takes the halo maximum of the production tile at r = 8, (4, 8, 8) -- the whole (h, w) plane --
    which contains the halo of either emulated tile, so it is never smaller than the emulated tile's own"""
    assert tile in EMU_TILES and x.shape[-1] == R_EMU and cr.tile_dims(R_EMU, sr.VB) == (4, 8, 8)
    return sr.conv64(x, w, bias, pro)


def ratio(y, ref, bound):
    assert bool((bound > 0).all())
    return float(((torch.as_tensor(np.asarray(y)).double() - ref).abs() / bound).max())


def range_data(case, cin=64):
    x, w, bias, _ = data(cin, COUT_EMU, R_EMU, 2, 5)
    return sr.range_case(case, x, w, bias, torch.Generator().manual_seed(11))


# ---- the plan ------------------------------------------------------------------------------------------------------------

def test_plan_mirror_equals_the_librarys_host_calls():
    from lion_amd import _lib
    lib = _lib.load()
    for r in (8, 16, 32):
        for cout in (32, 64, 96, 128, 256):
            p = sr.split_plan(r, 64, cout)
            assert lib.lion_conv3d_split_stat_tiles(r, cout) == p["stat_tiles"]
            td, th, tw = p["tile"]
            assert td * th * tw == 256 and tw == r and (td, th, tw) == cr.tile_dims(r, sr.VB)
            assert p["cb"] == (2 if r > 8 and cout % 64 == 0 else 1) and p["grid"][1] * 32 * p["cb"] == cout
            assert p["grid"][0] == (2 if r == 8 else r ** 3 // 256)
    assert lib.lion_conv3d_split_stat_tiles(12, 64) == 0
    # what the entry point refuses
    assert sr.split_plan(16, 24, 32) is None and sr.split_plan(16, 32, 48) is None and sr.split_plan(12, 32, 32) is None
    assert sr.split_plan(16, 272, 32, pro=True) is None and sr.split_plan(8, 272, 32, pro=True) is None
    assert sr.split_plan(16, 272, 32) is not None and sr.split_plan(16, 256, 32, pro=True) is not None
    assert sr.split_plan(8, 32, 32, occ=True) is None and sr.split_plan(8, 32, 32, pro=True, tconst=True) is None
    # the pro_inst rule of launch_split_t
    assert sr.split_plan(16, 64, 64, stats=True)["inst"] == (True, True)        # re-routed
    assert sr.split_plan(16, 272, 64, stats=True)["inst"] == (False, True)      # the real one
    assert sr.split_plan(16, 64, 32, stats=True)["inst"] == (False, True)       # CB = 1 is not re-routed
    assert sr.split_plan(16, 64, 64)["inst"] == (False, False) and sr.split_plan(8, 64, 64, stats=True)["inst"] == (False, True)


def test_case_table_reaches_the_paths_it_names():
    plans = set()
    for name, ((r, B, cin, cout), (kernel, cb, ctiles)) in {**sr.DENSE_CASES, **sr.CIN_FOUR_FORMS}.items():
        p = sr.split_plan(r, cin, cout)
        assert (p["kernel"], p["cb"], p["grid"][1]) == (kernel, cb, ctiles), name
        plans.add((r, p["kernel"], p["cb"]))
    # all five plans
    assert plans == {(8, "pipe", 1), (16, "tile", 1), (16, "tile", 2), (32, "tile", 1), (32, "tile", 2)}
    for name, ((r, B, cin, cout), _) in sr.DENSE_CASES.items():
        assert cin == 48 and B == 2 and sr.split_plan(r, cin, cout)["chunks"] == 3, name
    # the one-chunk and two-chunk walks of the r = 8 kernel and of the r16-CB2 tile
    walks = {(sr.split_plan(r, cin, cout)["kernel"], sr.split_plan(r, cin, cout)["chunks"])
             for (r, B, cin, cout), _ in sr.CIN_FOUR_FORMS.values()}
    assert walks == {("pipe", 1), ("pipe", 2), ("tile", 1), ("tile", 2)}
    # the single forms: each instantiation by name; the <false, true> one is the CB = 2 tile beyond 256 channels
    for name, ((r, B, cin, cout), pro, stats, inst) in sr.CIN_SINGLE_FORMS.items():
        p = sr.split_plan(r, cin, cout, pro=pro, stats=stats)
        assert p is not None and p["inst"] == inst, name
    (r, B, cin, cout), pro, stats, _ = sr.CIN_SINGLE_FORMS["r16-cb2-sums-without-prologue-272"]
    p = sr.split_plan(r, cin, cout, pro=pro, stats=stats)
    assert (p["kernel"], p["cb"], p["inst"]) == ("tile", 2, (False, True)) and cin > 256
    # statistics without a prologue at every Cin <= 256 of the table run on the PRO instantiation instead
    for (r, B, cin, cout), (kernel, cb, _) in {**sr.DENSE_CASES, **sr.CIN_FOUR_FORMS}.values():
        if kernel == "tile" and cb == 2:
            assert sr.split_plan(r, cin, cout, stats=True)["inst"] == (True, True)
    for name, (r, B, cin, cout) in sr.REFUSED.items():
        assert sr.split_plan(r, cin, cout, pro=True) is None and sr.split_plan(r, cin, cout) is not None, name
    # dynamic range: the r = 8 kernel and the CB = 1 tile
    assert {(sr.split_plan(r, cin, cout)["kernel"], sr.split_plan(r, cin, cout)["cb"])
            for (r, B, cin, cout) in list(sr.RANGE_SHAPES.values()) + list(sr.RANGE_SHAPES_64.values())} == {("pipe", 1), ("tile", 1)}
    for shape in sr.RANGE_SHAPES:
        assert sr.range_shape(shape, "rising")[2] == 64 and sr.range_shape(shape, "falling")[2] == 64


@pytest.mark.parametrize("shape", list(sr.RANGE_SHAPES))
def test_rising_rescales_at_every_chunk_and_falling_never(shape):
    """the rescale in the r = 8 kernel and in the CB = 1 tile: on `rising` every tile brings its accumulators onto a new scale
    at each of the three later chunks; on `falling` and on normal data (almost) never"""
    r, B, cin, cout = sr.range_shape(shape, "rising")
    x, w, bias, _ = data(cin, cout, r, B, 5)
    gen = torch.Generator().manual_seed(11)
    tiles = B * sr.split_plan(r, cin, cout)["stat_tiles"]
    assert sr.rescales(sr.range_case("rising", x, w, bias, gen)[0], r) == 3 * tiles
    assert sr.rescales(sr.range_case("falling", x, w, bias, gen)[0], r) == 0
    assert sr.rescales(x, r) < tiles // 2
    e = sr.chunk_exponents(sr.range_case("falling", x, w, bias, gen)[0], r)
    assert int((e[..., -1] - e[..., 0]).min()) >= 19        # the last chunk sits ~2^21 under the first


# ---- the bound is satisfiable ----------------------------------------------------------------------------------------------

def test_halo_max_is_the_maximum_over_tile_and_halo():
    r = 16
    z = torch.randn(2, 3, r, r, r).double()
    z[0, 1, 3, 3, 5] = 50.0          # last d-row, last h-row of tile (0, 0): seen by tiles (0..1, 0..1)
    z[1, 0, 9, 9, 9] = float("inf")  # ignored
    M = sr.halo_max(z, r)
    t = cr.tile_view(M, r, sr.VB)[:, 0]
    assert bool((t == t[..., :1]).all())
    got = t[0, :, 0].reshape(4, 4)
    assert bool((got[:2, :2] == 50.0).all()) and float(got[2:].max()) < 50.0 and float(got[:, 2:].max()) < 50.0
    assert bool(torch.isfinite(M).all())
    zp = torch.nn.functional.pad(z[1].abs().nan_to_num(posinf=0.0), (0, 0, 1, 1, 1, 1))
    assert float(t[1, 5, 0]) == float(zp[:, 4:10, 4:10].max())     # tile (1, 1): d, h = 3 .. 8 of the grid


@pytest.mark.parametrize("tile", EMU_TILES)
@pytest.mark.parametrize("cin", [16, 48])
def test_bound_holds_for_the_emulation_plain_and_prologue(tile, cin):
    x, w, bias, pro = data(cin, COUT_EMU, R_EMU, 2, 20 + cin)
    worst = {}
    for p in (None, pro):
        ref, bound = conv64_tiled(x, w, bias, p, tile)
        y = sr.emulate_split(x.numpy(), w.numpy(), bias.numpy(), None if p is None else (p[0].numpy(), p[1].numpy()), tile)
        assert np.all(np.isfinite(y))
        worst[p is not None] = ratio(y, ref, bound)
        sref, sbound = sr.tile_stats64(torch.as_tensor(y), R_EMU)
        assert ratio(cr.emulate_tile_stats32(y, R_EMU, sr.VB), sref, sbound) <= 1.0
    print(f"emulation tile {tile} Cin {cin}: worst error / bound = {worst}")
    assert all(0.0 < v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("tile", EMU_TILES)
@pytest.mark.parametrize("case", sr.RANGE_CASES)
def test_bound_holds_for_the_emulation_on_every_dynamic_range_case(case, tile):
    x, w, bias = range_data(case)
    ref, bound = conv64_tiled(x, w, bias, None, tile)
    y = sr.emulate_split(x.numpy(), w.numpy(), bias.numpy(), None, tile)
    assert np.all(np.isfinite(y))
    q = ratio(y, ref, bound)
    print(f"emulation {case} tile {tile}: worst error / bound = {q:.4f}")
    assert 0.0 < q <= 1.0, (case, q)


def test_emulation_is_exactly_scale_invariant_and_keeps_nonfinite_inputs_local():
    x, w, bias, _ = data(32, COUT_EMU, R_EMU, 1, 3)
    base = sr.emulate_split(x.numpy(), w.numpy(), None)
    for k in (-80, -17, 9, 40, 80):
        f = np.float32(2.0 ** k)
        assert np.array_equal(sr.emulate_split(x.numpy() * f, w.numpy(), None), base * f), k
        assert np.array_equal(sr.emulate_split(x.numpy(), w.numpy() * f, None), base * f), k
    xp = x.clone()
    xp[0, 3, 2, 2, 2] = float("inf")
    y = sr.emulate_split(xp.numpy(), w.numpy(), bias.numpy())
    assert not np.isfinite(y[0, :, 2, 2, 2]).any()
    xc = x.clone()
    xc[0, 3, 2, 2, 2] = 0.0
    ref, bound = conv64_tiled(xc, w, bias, None, (4, 8))
    mask = torch.ones(ref.shape, dtype=torch.bool)
    mask[0, :, 1:4, 1:4, 1:4] = False
    assert np.all(np.isfinite(y[mask.numpy()]))
    assert float(((torch.as_tensor(y).double() - ref).abs() / bound)[mask].max()) <= 1.0


# ---- the bound catches the seeded defects ----------------------------------------------------------------------------------

# (defect, Cin) -> the cases that must leave the bound, worked out from what each defect does (the seven chunk-free cases =
# every case but huge-one-chunk, rising and falling, which need three chunks or more):
#   no-rescale           wherever a later chunk raises the maximum by binades: what was accumulated keeps the old scale
#   scale-not-monotone   wherever a later chunk's maximum lies binades under the running one
#   drop-hi-chunk        wherever chunk 1 carries more of the sum than the bound allows (~K 2^-23 = 2e-4 at Cin = 64): everywhere
#                        but on huge-one-chunk (chunk 1 is 1e-4 of chunk 2) and rising (2^-14 of chunk 3), which the bound
#                        rightly lets pass
#   drop-lo-x            an error of ~2^-12 per product with a random sign, against a worst-case bound of K 2^-23 per product: at
#                        Cin = 16 (K = 432) it leaves the bound on every case; at Cin = 64 (K = 1728, K 2^-23 = 2^-12.2) the
#                        dot-product bound covers it -- a linear-in-K bound cannot see a lost lo piece behind many channels.  The
#                        one-chunk rows of the GPU tests (Cin = 16, every form, r = 8 and r16-CB2) are where it would show, and
#                        the per-sample 5e-6 of max |ref| that the dynamic-range tests also keep sees it at either Cin.
CHUNK_FREE = tuple(c for c in sr.RANGE_CASES if c not in ("huge-one-chunk", "rising", "falling"))
CAUGHT_BY = {
    ("no-rescale", 64): ("rising", "huge-one-chunk"),
    ("scale-not-monotone", 64): ("falling", "huge-one-chunk"),
    ("drop-hi-chunk", 64): CHUNK_FREE + ("falling",),
    ("drop-hi-chunk", 16): CHUNK_FREE,
    ("drop-lo-x", 16): CHUNK_FREE,
}
# ... and the cases on which it stays inside: the rescale pair needs both directions
INSIDE_ON = {("no-rescale", 64): ("falling",), ("scale-not-monotone", 64): ("rising",),
             ("drop-hi-chunk", 64): ("huge-one-chunk", "rising")}


@pytest.mark.parametrize("defect,cin", list(CAUGHT_BY) + [("drop-lo-x", 64)])
def test_each_seeded_defect_leaves_the_bound_on_its_named_cases(defect, cin):
    tile = (4, 8)
    table = {}
    for case in (sr.RANGE_CASES if cin == 64 else CHUNK_FREE):
        x, w, bias = range_data(case, cin)
        ref, bound = conv64_tiled(x, w, bias, None, tile)
        with np.errstate(all="ignore"):
            y = sr.emulate_split(x.numpy(), w.numpy(), bias.numpy(), None, tile, defect=defect)
        err = (torch.as_tensor(y).double() - ref).abs() / bound
        table[case] = float(torch.nan_to_num(err, nan=float("inf")).max())
    print(f"defect {defect} at Cin = {cin}: worst error / bound per case = " + ", ".join(f"{c} {v:.3g}" for c, v in table.items()))
    if defect == "drop-lo-x":
        # what the elementwise bound lets pass behind 64 channels, the per-sample 5e-6 of test_conv_split_gpu.py still sees --
        # the GPU tests hold the dynamic-range cases to both
        for case in table:
            x, w, bias = range_data(case, cin)
            ref, _ = conv64_tiled(x, w, bias, None, tile)
            clean = sr.per_sample_err(torch.as_tensor(sr.emulate_split(x.numpy(), w.numpy(), bias.numpy(), None, tile)), ref)
            bad = sr.per_sample_err(torch.as_tensor(sr.emulate_split(x.numpy(), w.numpy(), bias.numpy(), None, tile, defect=defect)), ref)
            print(f"  {case}: per-sample error / max |ref| clean {clean:.2e}, {defect} {bad:.2e}")
            assert clean < 5e-6 < bad, (case, clean, bad)
    for case in CAUGHT_BY.get((defect, cin), ()):
        assert table[case] > 1.0, (defect, case, table[case])
    for case in INSIDE_ON.get((defect, cin), ()):
        assert table[case] <= 1.0, (defect, case, table[case])


# ---- the clouds -------------------------------------------------------------------------------------------------------------

def brute_masks(cnt, r, margin):
    """conv_tile_occ_kernel's loops, written out"""
    B = cnt.shape[0]
    td, th, _ = cr.tile_dims(r, sr.VB)
    rw = 64 // r
    col = (cnt.reshape(B, r, r, r) > 0).any(-1)
    out = torch.zeros(B, (r // td) * (r // th), dtype=torch.long)
    for b in range(B):
        for t in range(out.shape[1]):
            dt, ht = (t // (r // th)) * td, (t % (r // th)) * th
            for w in range(4):
                dl, hl = dt + (w * rw) // th, ht + (w * rw) % th
                blk = col[b, max(dl - margin, 0):dl + margin + 1, max(hl - margin, 0):hl + rw + margin]
                out[b, t] |= int(bool(blk.any())) << w
    return out


@pytest.mark.parametrize("r", [16, 32])
@pytest.mark.parametrize("kind", sr.CLOUDS)
def test_clouds_produce_the_tile_flags_they_are_named_for(kind, r):
    cnt = sr.cloud_counts(kind, r)
    td, th, _ = cr.tile_dims(r, sr.VB)
    nth = r // th
    T = (r // td) * nth
    kinds = sr.tile_kinds(r)
    fl = {lv: sr.tile_flags(cnt, r, lv) for lv in sr.LEVELS}
    for m in (1, 2):
        assert torch.equal(fl[0][f"mask{m}"], brute_masks(cnt, r, m)), m
    for lv in sr.LEVELS:
        f = fl[lv]
        assert bool(f["stored1"][f["mask1"] != 0].all()) and bool(f["stored2"][f["mask2"] != 0].all())
        assert bool(((f["mask1"] & ~f["mask2"]) == 0).all())
    assert bool(fl[0]["stored1"].all()) and bool(fl[0]["stored2"].all())
    # level 1: the first conv stores what the delta conv stages (its margin-2 tiles and their neighbours), level 2 only its own
    assert torch.equal(fl[2]["stored1"], fl[2]["mask1"] != 0) and bool((fl[1]["stored1"] | ~fl[2]["stored1"]).all())
    assert torch.equal(fl[1]["stored2"], fl[1]["mask2"] != 0) and torch.equal(fl[1]["stored2"], fl[2]["stored2"])
    m1, m2 = fl[0]["mask1"][0], fl[0]["mask2"][0]
    tile_of = lambda d, h: (d // td) * nth + h // th
    if kind == "full":
        assert bool((fl[2]["mask1"] == 0xf).all()) and bool(fl[2]["stored1"].all())
        return
    (d, h, w), = sr.cloud_voxels(kind, r)
    own = tile_of(d, h)
    assert int(m1[own]) != 0 and int((m1 != 0).sum()) < T // 2
    unstored = lambda key, lv: {kinds[t] for t in range(T) if not bool(fl[lv][key][0, t])}
    if kind == "origin":
        assert kinds[own] == "lo-lo" and int(m1[own]) & 1
        assert kinds[tile_of(r - 1 - d, r - 1 - h)] == "hi-hi" and int(fl[0]["mask1"][1, T - 1]) & 8   # sample 1: reflected
    if kind == "far-corner":
        assert kinds[own] == "hi-hi" and int(m1[own]) & 8 and int(fl[0]["mask1"][1, 0]) & 1
    if kind == "interior":
        assert kinds[own] == "in-in" and d % td in (td // 2 - 1, td // 2) and h % th in (1, 2)
        want = {a + "-" + b for a in ("lo", "in", "hi") for b in ("lo", "in", "hi")}
        # unstored tiles on the low face, in the interior and on the high face, in d and in h, for either convolution at
        # either aware level; all nine positions for the first conv at level 2
        for key in ("stored1", "stored2"):
            for lv in (1, 2):
                u = unstored(key, lv)
                assert {k.split("-")[0] for k in u} == {k.split("-")[1] for k in u} == {"lo", "in", "hi"}, (key, lv, u)
        assert unstored("stored1", 2) == want
    if kind == "last-d-row":
        assert d % td == td - 1 and int(m1[tile_of(d + 1, h)]) != 0 and int(m1[tile_of(d - td, h)]) == 0
    if kind == "single-bit":
        single = [int(v) for v in m1.tolist() if v in (1, 2, 4, 8)]
        assert single, m1.tolist()
        assert int(m1[own]) not in (0, 1, 2, 4, 8, 0xf)      # and its own tile runs some waves, not all
