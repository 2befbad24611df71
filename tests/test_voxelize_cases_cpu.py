"""CPU suite: every case of tests/voxelize_cases.py reaches the plan and has the property it is named for.  The restated
launchers are checked against the library's pure host calls (lion_internal_voxelize_plan, lion_voxel_plan_bytes,
lion_avg_voxelize_workspace_bytes), the
builders against the CPU oracle."""
import ctypes
import re

import numpy as np
import pytest

import voxelize_cases as vc


@pytest.fixture(scope="module")
def lib():
    from lion_amd import _lib
    return _lib.load()


def ids(cases):
    return [c.id for c in cases]


PLAN_FIELDS = ("S", "CS", "SV", "NP", "n_words", "arena_words", "lds", "grid")
EUNSUPPORTED = -2


def library_plan(lib, B, C, N, r, kind):
    """lion_internal_voxelize_plan -> (return code, dict of its eight fields)"""
    out = (ctypes.c_int32 * 8)()
    rc = lib.lion_internal_voxelize_plan(B, C, N, r, kind, out, None)
    return rc, dict(zip(PLAN_FIELDS, out))


def assert_restatement_equals_library(lib, B, C, N, r):
    """vox_plan / scatter_plan against lion_internal_voxelize_plan, field for field, for the three kinds.  `lds` and `grid`
    are not among the scatter restatement's fields: they follow from them (ScatterLds: slot[SV] | ust[n_words] | 64 header
    words | arena, then PREFETCH_PAD; clouds in groups of 8, S slabs x CS channel ranges each)."""
    want = vc.vox_plan(B, C, N, r)
    rc, got = library_plan(lib, B, C, N, r, 0)
    assert rc == (0 if want["fast"] else EUNSUPPORTED), (B, C, N, r, rc, want["why"])
    grid = lambda q: vc.cdiv(B, 8) * 8 * q["S"] * q["CS"]
    assert got == dict({k: want[k] for k in PLAN_FIELDS[:7]}, grid=grid(want)), (B, C, N, r, got, want)
    for kind, read in ((1, False), (2, True)):
        want = vc.scatter_plan(B, C, N, r, read=read)
        rc, got = library_plan(lib, B, C, N, r, kind)
        assert rc == (0 if want is not None else EUNSUPPORTED), (B, C, N, r, kind, rc)
        if want is not None:
            lds = (want["SV"] + want["n_words"] + 64 + want["arena_words"]) * 4 + vc.PREFETCH_PAD
            assert got == dict(want, lds=lds, grid=grid(want)), (B, C, N, r, kind, got, want)
            assert lds + (1024 if read else 0) <= vc.LDS_LIMIT // (2 if N <= vc.VT else 1)


def oracle_ids(orc, case):
    """voxel ids [B, N] the oracle gives the case's cloud under its canonical normalisation"""
    co, _ = vc.forward_inputs(case)
    normalize, eps = vc.canonical(case)
    _, vox = orc.voxelize_coords(co, case.p["r"], normalize, eps)
    return vc.vox_ids(vox, case.p["r"])


def test_case_ids_are_unique_and_grids_stay_small():
    names = ids(vc.ALL_FORWARD + vc.GRAD)
    assert len(set(names)) == len(names)
    for c in vc.ALL_FORWARD:
        p = c.p
        assert p["B"] * p["C"] * p["r"] ** 3 * 4 <= vc.OUT_CAP_BYTES, c.id


@pytest.mark.parametrize("case", vc.ALL_FORWARD, ids=ids(vc.ALL_FORWARD))
def test_restated_plan_agrees_with_the_host_calls(lib, case):
    p = case.p
    B, C, N, r = p["B"], p["C"], p["N"], p["r"]
    plan = vc.vox_plan(B, C, N, r)
    nbytes = lib.lion_voxel_plan_bytes(B, N, r)
    assert (nbytes != 0) == plan["fast"] == vc.vox_plan(B, 0, N, r)["fast"]
    assert nbytes == vc.plan_bytes(B, N, r)
    if plan["fast"]:
        assert vc.slabs_of_plan_bytes(nbytes, B, N) == plan["S"]
        assert plan["lds"] <= vc.LDS_LIMIT // (2 if plan["two_per_cu"] else 1)
    assert lib.lion_avg_voxelize_workspace_bytes(B, C, N, r) == plan["ws_bytes"]
    assert not plan["fast"] or plan["two_per_cu"] == (plan["NP"] == 1) and N <= plan["NP"] * vc.VT and (plan["NP"] == 1 or N > plan["NP"] * vc.VT // 2)
    # the path in the name
    if case.path == "fallback":
        assert not plan["fast"] and vc.scatter_plan(B, C, N, r) is None
        if "why" in p:
            assert plan["why"] == vc.FALLBACK_WHY.get(p["why"], p["why"])
            if p["why"] == "s1":
                assert plan["S"] == 1 and r == 32
    else:
        assert plan["fast"] and vc.scatter_plan(B, C, N, r) is not None
        if r in (16, 32):
            assert vc.scatter_plan(B, C, N, r, read=True) is not None
    m = re.match(r"S(\d+)-CS(\d+)-NP(\d+)-", case.id)
    if m:
        assert (plan["S"], plan["CS"], plan["NP"]) == tuple(int(g) for g in m.groups())
    assert_restatement_equals_library(lib, B, C, N, r)


SWEEP_R = sorted(set(range(2, 51, 2)) | {9, 15, 33})


@pytest.mark.parametrize("r", SWEEP_R)
def test_restated_plans_equal_the_library_across_every_threshold(lib, r):
    """every rule of vox_plan has a threshold among these: S and CS (B, C, r), NP and two workgroups per CU (N at 1024,
    2048, 4096, 8192), the LDS fit (r, N), the scatter's coarsening (N <= 1024, small SV x channels), divisibility (odd r)"""
    for B in (1, 2, 8, 32, 64):
        for C in (1, 8, 17, 64, 128):
            for N in (1, 7, 1024, 1025, 2048, 2049, 4096, 8192, 8193):
                assert_restatement_equals_library(lib, B, C, N, r)


def test_plan_query_refuses_bad_arguments(lib):
    out = (ctypes.c_int32 * 8)()
    for args in ((0, 8, 64, 8, 0), (1, -1, 64, 8, 0), (1, 0, 64, 8, 1), (1, 8, 0, 8, 0), (1, 8, 64, 0, 0), (1, 8, 64, 8, 3),
                 (1, 8, 64, 8, -1)):
        assert lib.lion_internal_voxelize_plan(*args, out, None) == -1, args
    assert lib.lion_internal_voxelize_plan(1, 8, 64, 8, 0, None, None) == -1
    assert lib.lion_internal_voxelize_plan(1, 0, 64, 8, 0, out, None) == 0                # the index kernel: C = 0
    assert lib.lion_internal_voxelize_plan(1, 8, 64, 1025, 0, out, None) == EUNSUPPORTED  # r^3 > 2^30


def test_the_case_tables_plans():
    """the plan values the case table was chosen for"""
    want = {(3, 64, 2048, 32): (16, 8), (32, 16, 2048, 32): (8, 1), (64, 2, 1200, 32): (4, 1), (128, 2, 64, 16): (4, 1),
            (128, 2, 1200, 32): (2, 1), (256, 2, 64, 16): (2, 1), (512, 2, 64, 16): (1, 1), (1, 8, 64, 12): (2, 1),
            (1, 8, 64, 14): (2, 1), (1, 8, 2048, 30): (2, 1), (1, 8, 64, 20): (8, 1), (1, 8, 64, 24): (16, 1),
            (1, 8, 2048, 36): (16, 1), (32, 64, 2048, 32): (8, 1)}
    for shape, (S, CS) in want.items():
        plan = vc.vox_plan(*shape)
        assert (plan["S"], plan["CS"]) == (S, CS) and plan["fast"], shape
    assert vc.vox_plan(1, 8, 64, 20)["SV"] == 1000 and vc.vox_plan(1, 8, 64, 24)["SV"] == 864
    assert vc.vox_plan(1, 8, 2048, 36)["SV"] == 2916
    for shape in ((1, 8, 2048, 34), (1, 8, 8192, 46)):
        assert vc.vox_plan(*shape)["why"] == "lds"
    for N, r in ((2048, 30), (2048, 36), (8192, 44), (8192, 48)):
        assert vc.vox_plan(1, 8, N, r)["fast"]
    # the scatter launcher's own channel split
    assert vc.vox_plan(32, 128, 256, 8)["CS"] == 16 and vc.scatter_plan(32, 128, 256, 8)["CS"] == 8
    assert vc.vox_plan(32, 192, 64, 8)["CS"] == 16 and vc.scatter_plan(32, 192, 64, 8)["CS"] == 8
    assert vc.scatter_plan(32, 128, 1024, 16)["CS"] == 2


def test_no_fast_shape_is_refused_by_the_scatter_launcher(lib):
    """the scatter's arena check of vox_plan (arena / 4 < N + 1 + nocc, 1088 bytes less for the reader-aware form) never
    refuses a shape that its fused form calls fast: its fixed part is smaller than the fused kernel's by SV / 32 + 36 words and more, and
    a fast shape has room for hist + tmp >= SV + N words, which exceeds N + 1 + nocc + 272"""
    for r in range(2, 52, 2):
        for N in (1, 64, 1000, 1024, 1025, 2048, 3000, 3516, 3517, 4096, 5000, 8192):
            for B in (1, 8, 9, 32, 128, 256, 512, 1024):
                for C in (1, 16, 128, 512):
                    if vc.vox_plan(B, C, N, r)["fast"]:
                        assert vc.scatter_plan(B, C, N, r) is not None, (B, C, N, r)
                        assert r not in (16, 32) or vc.scatter_plan(B, C, N, r, read=True) is not None, (B, C, N, r)
                        assert library_plan(lib, B, C, N, r, 1)[0] == 0, (B, C, N, r)
                        assert r not in (16, 32) or library_plan(lib, B, C, N, r, 2)[0] == 0, (B, C, N, r)


ID_BUILT = [c for c in vc.ALL_FORWARD if c.p["kind"] not in ("gauss", "clump")]


@pytest.mark.parametrize("case", ID_BUILT, ids=ids(ID_BUILT))
def test_id_built_clouds_land_on_their_voxels(orc, case):
    assert np.array_equal(oracle_ids(orc, case), vc.forward_ids(case)[0])


CHUNKED = [c for c in vc.PLANS if c.p["kind"] == "oneslab"]


@pytest.mark.parametrize("case", CHUNKED, ids=ids(CHUNKED))
def test_one_slab_clouds_chunk_their_channels(orc, case):
    p = case.p
    plan = vc.vox_plan(p["B"], p["C"], p["N"], p["r"])
    pts, occ = vc.slab_headers(oracle_ids(orc, case)[0], plan)
    assert pts[0] == p["N"] - 1 and occ[0] == min(p["N"] - 1, plan["SV"]) and pts[1:] == [0] * (plan["S"] - 2) + [1]
    chm = vc.ch_max_of(plan["arena_words"], pts[0], occ[0], p["C"])
    c_per = vc.cdiv(p["C"], plan["CS"])
    assert chm < c_per and chm == {16: 3, 48: 1}[p["r"]]


def test_odd_chunk_remainders_are_among_the_plans():
    """C % CS != 0 (the last channel range is short) and C no multiple of 16 / NP (B1's clamped row loads), for every NP"""
    seen = set()
    for c in vc.PLANS:
        p = c.p
        plan = vc.vox_plan(p["B"], p["C"], p["N"], p["r"])
        if vc.cdiv(p["C"], plan["CS"]) % (16 // plan["NP"]) and p["C"] % 2:
            seen.add((plan["NP"], plan["CS"] > 1 and p["C"] % plan["CS"] != 0))
    assert {np_ for np_, _ in seen} == {1, 2, 4, 8} and {(1, True), (2, True)} <= seen


@pytest.mark.parametrize("case", vc.ADOPT, ids=ids(vc.ADOPT))
def test_adoption_clouds_have_their_headers_and_moves(orc, case):
    p = case.p
    plan = vc.scatter_plan(p["B"], p["C"], p["N"], p["r"])
    assert plan["NP"] >= 2 and plan["S"] == len(p["slabs"])
    got = oracle_ids(orc, case)
    for b in range(p["B"]):
        pts, occ = vc.slab_headers(got[b], plan)
        want = [tuple(s) for s in p["slabs"]]
        assert (pts[p["lands"]], occ[p["lands"]]) in [(want[p["lands"]][0] + 1, want[p["lands"]][1] + d) for d in (0, 1)]
        want[p["lands"]] = (pts[p["lands"]], occ[p["lands"]])
        assert list(zip(pts, occ)) == want
    for cs in range(plan["CS"]):
        chm, nc, moves, rem = vc.chunking(plan, pts, occ, p["C"], cs)
        assert moves == p["moves"], (cs, moves)
        for s in range(plan["S"]):
            assert rem[s] == nc[s] - sum(1 for m in moves if m[1] == s)
    chm, nc, moves, rem = vc.chunking(plan, pts, occ, p["C"])
    name = case.id[len("adopt-"):]
    if name == "many-adopters":
        assert (chm[0], nc[0]) == (14, 5) and len({m[0] for m in moves}) == 4
    elif name == "one-adopter-three-chunks":
        assert nc[15] == 6 and [m[0] for m in moves] == [14] * 3
    elif name == "cap-of-five":
        assert (plan["CS"], chm[15], nc[15]) == (1, 1, 15) and len(moves) == 5 and rem[15] == 10
    elif name == "two-crowded":
        assert {m[1] for m in moves} == {0, 4} and nc[0] == nc[4] == 3
    elif name == "partial-last-chunk":
        c_per = vc.cdiv(p["C"], plan["CS"])
        assert (c_per, chm[0], nc[0]) == (30, 14, 3) and moves[0] == (1, 0, 2) and c_per - 2 * chm[0] == 2
    elif name == "no-empty-slab":
        assert nc[0] >= 2 and moves == [] and min(pts) > 0
    else:
        raise AssertionError(name)


def test_chunking_stops_as_the_kernel_does():
    """the greedy loop's three stops on hand-made headers: nmax < 2, la + 2 >= 2 nmax, taken == 5"""
    plan = dict(S=4, CS=1, NP=2, arena_words=1000)
    # slab 0: 999 | 1 + 0 words per channel -> 1 channel per chunk, 12 chunks; slab 1 empty, slabs 2, 3 small
    chm, nc, moves, rem = vc.chunking(plan, [998, 0, 10, 10], [1, 0, 1, 1], 12)
    assert (chm[0], nc[0]) == (1, 12) and [m[2] for m in moves] == [11, 10, 9, 8, 7] and rem[0] == 7
    chm, nc, moves, rem = vc.chunking(plan, [998, 0, 0, 10], [1, 0, 0, 1], 4)      # 4 chunks, two adopters
    assert moves == [(1, 0, 3), (2, 0, 2)] and rem[0] == 2                        # then 1 + 2 >= 2 * 2
    assert vc.chunking(dict(plan, NP=1), [998, 0, 0, 10], [1, 0, 0, 1], 4)[2] == []
    assert vc.chunking(plan, [100, 0, 0, 10], [1, 0, 0, 1], 4)[2] == []           # one chunk: nothing to give


STAIRS = [c for c in vc.RUNS]


@pytest.mark.parametrize("case", STAIRS, ids=ids(STAIRS))
def test_staircase_clouds_have_their_run_lengths(orc, case):
    p = case.p
    plan = vc.vox_plan(p["B"], p["C"], p["N"], p["r"])
    got = oracle_ids(orc, case)[0]
    vs, counts = np.unique(got, return_counts=True)
    in_slab = (vs // plan["SV"]) == vc.STAIR_SLAB
    want = list(range(1, p["top"] + 1)) + ([p["long"]] if p["long"] else [])
    assert sorted(counts[in_slab].tolist()) == want
    if not p["long"]:
        assert p["top"] == 3 * vc.pw_of(plan["NP"]) + 3 and set(vc.run_edges(plan["NP"])) <= set(want)
    # a voxel's points sit in several waves (and, for NP >= 2, several point slots)
    big = vs[in_slab][np.argmax(counts[in_slab])]
    where = np.flatnonzero(got == big)
    assert np.unique((where % vc.VT) // 64).size >= 2 and (plan["NP"] == 1 or np.unique(where // vc.VT).size >= 2)
    # the order of a sum shows in its bits
    _, feat = vc.forward_inputs(case)
    assert vc.order_sensitive_fraction(feat[0], got) >= 0.5


@pytest.mark.parametrize("case", vc.COUNTERS, ids=ids(vc.COUNTERS))
def test_counter_clouds_have_their_distinct_voxels_per_wave(orc, case):
    p = case.p
    plan = vc.vox_plan(p["B"], p["C"], p["N"], p["r"])
    got = oracle_ids(orc, case)
    first = vc.wave_first(p["N"])
    for b in range(p["B"]):
        for j, (_, k, layout) in enumerate(vc.WAVE_PATTERNS):
            w = got[b, (first + j) * 64:(first + j + 1) * 64]
            assert np.unique(w).size == k and np.unique(w // plan["SV"]).size == 1
            _, cnt = np.unique(w, return_counts=True)
            if layout == "singles":                                # lanes 0 and 1 are alone on their voxels
                assert np.count_nonzero(w == w[0]) == 1 and np.count_nonzero(w == w[1]) == 1 and np.sort(cnt)[2] >= 2
            elif k <= 32:
                assert cnt.min() >= 2
    assert plan["NP"] == (1 if p["N"] <= 1024 else 2) and (plan["NP"] == 1 or first * 64 >= vc.VT)


def test_fallback_bound_is_the_sum_of_the_rounded_terms():
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((1, 2, 6), dtype=np.float32)
    ind = np.array([[3, 3, 3, 0, -2, 9]], np.int32)                # -2 and 9 clamp to 0 and 7
    cnt = np.array([[2, 0, 0, 3, 0, 0, 0, 1]], np.int32)
    ref, bound = vc.fallback_bound(feat, ind, cnt)
    third = np.float32(1) / np.float32(3)
    want = sum(float(np.float32(feat[0, 1, i] * third)) for i in range(3))
    assert ref[0, 1, 3] == want and ref[0, 1, 1] == 0 and bound[0, 1, 1] == 0
    assert bound[0, 1, 3] == 4 * vc.U32 * sum(abs(float(np.float32(feat[0, 1, i] * third))) for i in range(3))
    assert ref[0, 0, 7] == float(feat[0, 0, 5])


def test_grad_ref_clamps_and_zeroes():
    gy = np.arange(16, dtype=np.float32).reshape(1, 2, 8) + 1
    ind = np.array([[-5, 0, 3, 7, 8, 100, 2]], np.int32)
    cnt = np.array([[2, 0, 0, 3, 0, 0, 0, 4]], np.int32)
    gx = vc.grad_ref(gy, ind, cnt)
    assert gx[0, 0].tolist() == [0.5, 0.5, float(np.float32(4) * (np.float32(1) / np.float32(3))), 2.0, 2.0, 2.0, 0.0]


def test_grad_ref_equals_the_oracle_on_a_forwards_indices(orc):
    from conftest import gaussian_cloud
    rng = np.random.default_rng(11)
    _, vox = orc.voxelize_coords(gaussian_cloud(rng, 3, 257), 4, True, 0.0)
    _, ind, cnt = orc.avg_voxelize_forward(np.zeros((3, 1, 257), np.float32), vox, 4)
    gy = rng.standard_normal((3, 9, 64), dtype=np.float32)
    assert np.array_equal(orc.avg_voxelize_backward(gy, ind, cnt).view(np.int32), vc.grad_ref(gy, ind, cnt).view(np.int32))


def test_no_case_is_left_out(orc):
    S, NP, CS1, CSn, chunked, PW, why, np_scatter = set(), set(), False, False, False, set(), set(), set()
    for c in vc.ALL_FORWARD:
        p = c.p
        plan = vc.vox_plan(p["B"], p["C"], p["N"], p["r"])
        if plan["fast"]:
            S.add(plan["S"]); NP.add(plan["NP"]); PW.add(vc.pw_of(plan["NP"]))
            CS1 |= plan["CS"] == 1
            CSn |= plan["CS"] > 1
            chunked |= c in CHUNKED
            if vc.scatter_plan(p["B"], p["C"], p["N"], p["r"])["CS"] != plan["CS"]:
                np_scatter.add(plan["NP"])
        else:
            why.add(p["why"])
    assert S == {1, 2, 4, 8, 16} and NP == {1, 2, 4, 8} and CS1 and CSn and chunked and PW == {8, 16}
    assert np_scatter == {1}                                       # the scatter's own channel split: NP = 1 only
    assert why == {"odd", "lds", "r3", "s1", "n"} and {c.p["which"] for c in vc.FALLBACKS if c.path == "misaligned"} == {"out", "cnt"}
    assert {vc.vox_plan(c.p["B"], c.p["C"], c.p["N"], c.p["r"])["NP"] for c in vc.RUNS if not c.p["long"]} == {1, 2, 4, 8}
    assert {c.p["long"] for c in vc.RUNS if c.p["long"]} == {8191, 1900}
    assert {vc.vox_plan(c.p["B"], c.p["C"], c.p["N"], c.p["r"])["NP"] for c in vc.COUNTERS} == {1, 2}
    assert {k for _, k, _ in vc.WAVE_PATTERNS} == {1, 2, 8, 9, 10, 64}
    # adoption outcomes
    outcomes = set()
    for c in vc.ADOPT:
        p = c.p
        plan = vc.scatter_plan(p["B"], p["C"], p["N"], p["r"])
        pts, occ = vc.slab_headers(oracle_ids(orc, c)[0], plan)
        chm, nc, moves, rem = vc.chunking(plan, pts, occ, p["C"])
        per = {}
        for a, s, k in moves:
            per.setdefault(a, []).append((s, k))
        if not moves:
            outcomes.add("none")
        if len(per) >= 2 and all(len(v) == 1 for v in per.values()):
            outcomes.add("many-adopters-one-chunk")
        if any(1 < len(v) < 5 for v in per.values()):
            outcomes.add("several-chunks")
        if any(len(v) == 5 for v in per.values()) and rem[moves[0][1]] > 1:
            outcomes.add("cap-of-five")
        if len({s for _, s, _ in moves}) >= 2:
            outcomes.add("two-crowded")
        c_per = vc.cdiv(p["C"], plan["CS"])
        if any(k == nc[s] - 1 and c_per % chm[s] for _, s, k in moves):
            outcomes.add("partial-last-chunk")
    assert outcomes == {"none", "many-adopters-one-chunk", "several-chunks", "cap-of-five", "two-crowded", "partial-last-chunk"}
    assert {c.path for c in vc.ALL_FORWARD} == {"fused", "adopt", "runs", "counters", "fallback", "misaligned"}
    assert len(vc.GRAD) == 4 and set(vc.GRAD_CS) == {1, 8, 9, 17} and set(vc.GRAD_NS) == {1, 255, 256, 257, 1000}
