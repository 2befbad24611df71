"""-m gpu: the host side of the training path as a statement about behaviour -- which C entry points the layer walk of both PVCNN
variants (pvcnn2_ada.run_layers, pvcnn2.run_layers) and the tail of both PVConv voxel branches launch, in which order, forward and
backward; what each of the four AdaGN training ops keeps alive for its backward; which gradient slots it fills.  Counted with a spy on
lion_amd._lib.call.  Shapes are the smallest that reach every branch: B = 2, C = 16 (8 groups), r = 8 grids, N = 64 points, U = 8."""
import pytest
import torch
import torch.nn as nn

from conftest import fill_

pytestmark = pytest.mark.gpu

B, C, R, N, M, U = 2, 16, 8, 64, 32, 8


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


def _cfg():
    from lion_amd.config import released_prior_cfg
    return released_prior_cfg()


# ---------------------------------------------------------------------------------------------------------------- 1. walk census
HEAD = ["lion_row_stats64", "lion_gn_train_fold64"]                      # GroupNorm row sums (double) and the [B, C] fold
FOLD_B, PARAMS = "lion_gn_train_bwd_fold", "lion_gn_train_param_grads"
ACT = (HEAD + ["lion_affine_act"], ["lion_affine_act_bwd_stats", FOLD_B, "lion_affine_act_bwd_apply", PARAMS])
ACT_DROP = (HEAD + ["lion_affine_act_dropout"],
            ["lion_affine_act_dropout_bwd_stats", FOLD_B, "lion_affine_act_dropout_bwd_apply", PARAMS])
ACT_MAX = (HEAD + ["lion_affine_act_max"], ["lion_affine_act_max_bwd_stats", FOLD_B, "lion_affine_act_max_bwd_apply", PARAMS])
NORM_SE = (HEAD + ["lion_gn_se_gate_fwd", "lion_affine_act"],
           ["lion_affine_act_bwd_stats", "lion_gn_se_gate_bwd", FOLD_B, "lion_affine_act_bwd_apply", PARAMS])
SE_ALONE = (["lion_row_stats", "lion_se_gate_fwd", "lion_affine_act"],
            ["lion_affine_act_bwd_stats", "lion_se_gate_bwd", "lion_affine_act_bwd_apply"])
# the 1x1 Conv2d of the adaptive walk goes to its `conv` argument (pvcnn2_ada.conv1x1: train_ops.pwconv from 512 columns on, the
# inference kernel without autograd); the plain walk calls it as a module.  C = 16 is outside the voxel Conv3d kernels (Cout % 32):
# both walks hand the Conv3d to conv3d_module, which leaves it to the vendor library -- no entry point of ours.
PW = (["lion_pwconv_forward"], ["lion_pwconv_pack_weights", "lion_pwconv_forward", "lion_pwconv_wgrad"])   # data gradient: W^T, packed per step
PW_INFER = ["lion_pwconv_forward"]
NOTHING = ([], [])


def _then(*ops):
    """forward in order, backward in reverse order"""
    return [n for o in ops for n in o[0]], [n for o in reversed(ops) for n in o[1]]


def _norm(ada, ndim, c=C):
    from lion_amd.models.adagn import AdaGN
    return AdaGN(ndim, _cfg(), c) if ada else nn.GroupNorm(8, c)


def _voxel_list(ada, p, se):
    from lion_amd.models.pvcnn2_ada import SE3d, Swish
    layers = [nn.Conv3d(C, C, 3, padding=1), _norm(ada, 3), Swish(), nn.Dropout(p), nn.Conv3d(C, C, 3, padding=1), _norm(ada, 3)]
    return layers + ([SE3d(C)] if se else []), (B, C, R, R, R), False


def _sa_list(ada, u, swish=True):
    from lion_amd.models.pvcnn2_ada import Swish
    return [nn.Conv2d(C, C, 1), _norm(ada, 2)] + ([Swish()] if swish else []), (B, C, M, u), True


def _se_alone(ada):
    from lion_amd.models.pvcnn2_ada import SE3d
    return [SE3d(C)], (B, C, R, R, R), False


# case -> (builder(ada) -> (layers, input shape, reduce_max), expected(ada) -> {mode: (forward, backward) of the ordered entry points})
# modes: "train" (grad on, modules in train mode), "eval" (grad on, modules -- the Dropout -- in eval mode), "no_grad" (train mode).
# Without autograd the adaptive walk runs the modules (no entry point but the inference 1x1 convolution), the plain walk the ops.
WALK_CASES = {
    "conv_norm_swish_dropout_conv_norm_se": (
        lambda ada: _voxel_list(ada, 0.1, True),
        lambda ada: {"train": _then(ACT_DROP, NORM_SE), "eval": _then(ACT, NORM_SE),
                     "no_grad": ([], None) if ada else (_then(ACT_DROP, NORM_SE)[0], None)}),
    "conv_norm_swish_dropout_conv_norm": (
        lambda ada: _voxel_list(ada, 0.1, False),
        lambda ada: {"train": _then(ACT_DROP, ACT), "eval": _then(ACT, ACT),
                     "no_grad": ([], None) if ada else (_then(ACT_DROP, ACT)[0], None)}),
    "dropout_0_is_skipped": (
        lambda ada: _voxel_list(ada, 0.0, False),
        lambda ada: {"train": _then(ACT, ACT), "eval": _then(ACT, ACT), "no_grad": ([], None) if ada else (_then(ACT, ACT)[0], None)}),
    "dropout_1_stays_a_module": (
        lambda ada: _voxel_list(ada, 1.0, False),
        lambda ada: {"train": _then(ACT, ACT), "eval": _then(ACT, ACT), "no_grad": ([], None) if ada else (_then(ACT, ACT)[0], None)}),
    "sa_mlp_pooled_u8": (
        lambda ada: _sa_list(ada, 8),
        lambda ada: {"train": _then(PW if ada else NOTHING, ACT_MAX), "eval": _then(PW if ada else NOTHING, ACT_MAX),
                     "no_grad": (PW_INFER, None) if ada else (ACT_MAX[0], None)}),
    "sa_mlp_u7_not_pooled": (
        lambda ada: _sa_list(ada, 7),
        lambda ada: {"train": _then(NOTHING, ACT), "eval": _then(NOTHING, ACT),
                     "no_grad": (PW_INFER, None) if ada else (ACT[0], None)}),
    "norm_without_swish_pooled": (
        lambda ada: _sa_list(ada, 8, swish=False),
        lambda ada: {"train": _then(PW if ada else NOTHING, ACT_MAX), "eval": _then(PW if ada else NOTHING, ACT_MAX),
                     "no_grad": (PW_INFER, None) if ada else (ACT_MAX[0], None)}),
    "se3d_alone": (
        _se_alone,
        lambda ada: {"train": SE_ALONE, "eval": SE_ALONE, "no_grad": ([], None) if ada else (SE_ALONE[0], None)}),
    "norm_of_1032_channels_is_a_module": (
        lambda ada: ([_norm(ada, 1, 1032)], (B, 1032, N), False),
        lambda ada: {"train": NOTHING, "eval": NOTHING, "no_grad": ([], None)}),
}


def _walk(ada, layers, x, style, reduce_max):
    from lion_amd.conv_ops import conv3d_module
    from lion_amd.models import pvcnn2, pvcnn2_ada
    if ada:
        conv = lambda layer, t: conv3d_module(layer, t) if isinstance(layer, nn.Conv3d) else pvcnn2_ada.conv1x1(layer, t)
        return pvcnn2_ada.run_layers(layers, x, style, conv, reduce_max=reduce_max)
    return pvcnn2.run_layers(layers, x, reduce_max=reduce_max)


def walk_census(monkeypatch, calls, build, ada):
    """{mode: (forward names, backward names or None)} of one layer list, and {mode: AdaGN.affine calls per AdaGN} of the forward"""
    from lion_amd.models.adagn import AdaGN
    torch.manual_seed(0)
    layers, shape, reduce_max = build(ada)
    layers = nn.ModuleList(layers).cuda()
    fill_(layers)
    style = torch.randn(B, _cfg().latent_pts.style_dim, device="cuda")
    asked, real_affine = [], AdaGN.affine

    def affine(self, s):
        asked.append(id(self))
        return real_affine(self, s)
    monkeypatch.setattr(AdaGN, "affine", affine)
    adagns = [id(m) for m in layers if isinstance(m, AdaGN)]
    seen, affine_counts = {}, {}
    for mode in ("train", "eval", "no_grad"):
        layers.train(mode != "eval")
        for recorded in (False, True):     # the first pass fills the weight caches: what it launches more is not the walk's
            x = torch.randn(*shape, device="cuda").requires_grad_(mode != "no_grad")
            del calls[:], asked[:]
            with torch.set_grad_enabled(mode != "no_grad"):
                y = _walk(ada, layers, x, style, reduce_max)
            fwd = list(calls)
            affine_counts[mode] = [asked.count(i) for i in adagns]
            assert tuple(y.shape) == (tuple(shape[:-1]) if reduce_max else tuple(shape))
            bwd = None
            if mode != "no_grad":
                del calls[:]
                y.square().mean().backward()
                bwd = list(calls)
                assert x.grad is not None and tuple(x.grad.shape) == tuple(shape)
            if recorded:
                seen[mode] = (fwd, bwd)
    return seen, affine_counts


@pytest.mark.parametrize("ada", [True, False], ids=["adaptive", "plain"])
@pytest.mark.parametrize("case", sorted(WALK_CASES))
def test_walk_launches_these_entry_points_in_this_order(monkeypatch, calls, case, ada):
    build, expected = WALK_CASES[case]
    seen, affine_counts = walk_census(monkeypatch, calls, build, ada)
    want = expected(ada)
    for mode in ("train", "eval", "no_grad"):
        print(case, "adaptive" if ada else "plain", mode, seen[mode])
    for mode in ("train", "eval", "no_grad"):
        assert seen[mode][0] == want[mode][0], (mode, "forward")
        assert seen[mode][1] == want[mode][1], (mode, "backward")
        # AdaGN.affine(style): exactly once per AdaGN per forward, whichever branch the walk takes
        assert all(n == 1 for n in affine_counts[mode]), (mode, affine_counts[mode])


def test_plain_walk_leaves_a_group_norm_without_affine_to_the_module(monkeypatch, calls):
    from lion_amd.models.pvcnn2_ada import Swish
    build = lambda ada: ([nn.GroupNorm(8, C, affine=False), Swish()], (B, C, N), False)
    seen, _ = walk_census(monkeypatch, calls, build, False)
    assert seen == {"train": ([], []), "eval": ([], []), "no_grad": ([], None)}


def test_adaptive_walk_leaves_a_bare_group_norm_to_the_module(monkeypatch, calls):
    """only an AdaGN is the adaptive walk's norm layer"""
    from lion_amd.models.pvcnn2_ada import Swish
    build = lambda ada: ([nn.GroupNorm(8, C), Swish()], (B, C, N), False)
    seen, _ = walk_census(monkeypatch, calls, build, True)
    assert seen == {"train": ([], []), "eval": ([], []), "no_grad": ([], None)}


# ---------------------------------------------------------------------------------------------------------------- 2. tail census
ONE_OP_TAIL = ("lion_rows_dot2", "lion_trilinear_devoxelize_backward_affine")


def _pvconv(ada, r=R, with_se=True):
    from lion_amd.models import pvcnn2, pvcnn2_ada
    kw = dict(with_se=with_se, add_point_feat=False, attention=False, dropout=0.1, verbose=False)
    pv = pvcnn2_ada.PVConv(C, C, 3, r, cfg=_cfg(), **kw) if ada else pvcnn2.PVConv(C, C, 3, r, **kw)
    fill_(pv)
    return pv.cuda()


def _pvconv_step(pv, ada, calls, backward=True):
    """forward (+ backward) of one PVConv (voxel branch only: add_point_feat=False) -> (entry points, debug payload of the plain variant)"""
    torch.manual_seed(1)
    feat = torch.randn(B, C, N, device="cuda", requires_grad=True)
    coords = torch.randn(B, 3, N, device="cuda")
    style = torch.randn(B, _cfg().latent_pts.style_dim, device="cuda")
    del calls[:]
    out = pv((feat, coords, None, style) if ada else (feat, coords, None))
    assert tuple(out[0].shape) == (B, C, N)
    if backward:
        out[0].square().mean().backward()
        assert feat.grad is not None
    return list(calls), (None if ada else out[2])


@pytest.mark.parametrize("ada", [True, False], ids=["adaptive", "plain"])
def test_pvconv_tail_is_one_op_exactly_under_its_condition(monkeypatch, calls, ada):
    from lion_amd import train_ops
    took_tail = lambda names: all(n in names for n in ONE_OP_TAIL)
    took_walk = lambda names: not any(n in names for n in ONE_OP_TAIL) and "lion_trilinear_devoxelize_forward" in names

    names, payload = _pvconv_step(_pvconv(ada).train(), ada, calls)
    # training, with SE: norm -> SE3d -> devoxelize is one op; the only activation pass over a grid is the first norm's (with its
    # dropout) -- no lion_affine_act writes a gated grid -- and the gated grid of the plain variant's debug payload does not exist
    assert took_tail(names) and "lion_affine_act" not in names and "lion_affine_act_dropout" in names
    assert names.count("lion_trilinear_devoxelize_forward") == 1 and "lion_trilinear_devoxelize_backward" not in names
    if not ada:
        assert payload["voxel_features_4d"] is None and payload["resolution"] == R and payload["training"] is True

    def walks(pv, backward=True):   # the layer walk + trilinear_devoxelize instead; the gated grid exists
        names, payload = _pvconv_step(pv, ada, calls, backward)
        assert took_walk(names), names
        if not ada:
            r = pv.resolution
            assert tuple(payload["voxel_features_4d"].shape) == (B, C, r, r, r)
        return names

    monkeypatch.setattr(train_ops, "DEVOX_FUSED", False)
    assert "lion_gn_se_gate_fwd" in walks(_pvconv(ada).train())                 # switched off: norm -> SE3d still one op, then devoxelize
    monkeypatch.setattr(train_ops, "DEVOX_FUSED", True)
    # eval mode, grad on (forward only: an eval-mode devoxelisation keeps nothing for a backward)
    assert "lion_affine_act_dropout" not in walks(_pvconv(ada).eval(), backward=False)
    assert "lion_gn_se_gate_fwd" not in walks(_pvconv(ada, with_se=False).train())   # no SE3d
    r = 36   # a grid row of 36^3 * 4 = 186624 bytes: above the op's 128 KiB (and a multiple of 8 voxels, so only that clause refuses)
    assert r ** 3 * 4 > 128 * 1024 and r ** 3 % 8 == 0
    assert "lion_gn_se_gate_fwd" in walks(_pvconv(ada, r=r).train())


# ---------------------------------------------------------------------------------------------- 3. what each op keeps alive
CR = C // 8                      # SE3d's reduction
L3 = R ** 3
BC4 = B * C * 4                  # one [B, C] float32
COMMON = lambda numel: numel * 4 + 4 * BC4 + 2 * C * 4 + BC4   # x; A, Bs, mean, rstd; norm weight, norm bias; the factor's [B, C] view
STATS = B * C * 2 * 8            # the double row sums of x
GATE = 2 * BC4 + B * CR * 4 + 2 * CR * C * 4                    # um, g; h; w1, w2
DEVOX = B * C * N * 4 + 2 * B * 8 * N * 4 + B * N * 4            # devox(x); corner indices (int32) and weights; their sums
KEEPS = {   # op -> (tensors saved, bytes)
    "adagn_act": (10, COMMON(B * C * L3) + STATS + 0),
    "adagn_act_dropout": (10, COMMON(B * C * L3) + STATS + 8),   # the int64 seed
    "adagn_act_max": (8, COMMON(B * C * M * U)),                 # no row sums
    "adagn_se": (14, COMMON(B * C * L3) + STATS + GATE),
    "adagn_se_devox": (18, COMMON(B * C * L3) + STATS + GATE + DEVOX),
}


def _op_inputs(op, seed=0, points=False):
    """(callable on the leaves, x, parameters by name) of one op at the shapes of this file; points: x is [B, C, N], not a grid"""
    from lion_amd import train_ops
    from lion_amd.models.pvcnn2_ada import SE3d
    torch.manual_seed(seed)
    norm, se = nn.GroupNorm(8, C).cuda(), SE3d(C).cuda()
    fill_(norm)
    fill_(se)
    x = torch.randn(*((B, C, M, U) if op == "adagn_act_max" else (B, C, N) if points else (B, C, R, R, R)), device="cuda")
    factor, bias = 1.0 + 0.3 * torch.randn(B, C, device="cuda"), 0.3 * torch.randn(B, C, device="cuda")
    coords = torch.rand(B, 3, N, device="cuda") * (R - 1)
    run = {"adagn_act": lambda: train_ops.adagn_act(x, norm, factor, bias, act=True),
           "adagn_act_dropout": lambda: train_ops.adagn_act(x, norm, factor, bias, act=True, dropout_p=0.25),
           "adagn_act_max": lambda: train_ops.adagn_act_max(x, norm, factor, bias, act=True),
           "adagn_se": lambda: train_ops.adagn_se(x, norm, factor, bias, se),
           "adagn_se_devox": lambda: train_ops.adagn_se_devox(x, norm, factor, bias, se, coords, R)}[op]
    params = {"norm.weight": norm.weight, "norm.bias": norm.bias, "factor": factor, "bias": bias}
    if op in ("adagn_se", "adagn_se_devox"):
        params.update({"w1": se.fc[0].weight, "w2": se.fc[2].weight})
    return run, x, params


@pytest.mark.parametrize("op", sorted(KEEPS))
def test_op_saves_exactly_these_tensors(op):
    run, x, params = _op_inputs(op)
    x.requires_grad_(True)
    for p in params.values():
        p.requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = run()
    assert y.requires_grad
    count, nbytes = KEEPS[op]
    print(op, len(saved), sum(t.numel() * t.element_size() for t in saved), [tuple(t.shape) for t in saved])
    assert len(saved) == count
    assert sum(t.numel() * t.element_size() for t in saved) == nbytes


# ------------------------------------------------------------------------------------------------------------ 4. gradient slots
DX_PASSES = ("lion_affine_act_bwd_apply", "lion_affine_act_dropout_bwd_apply", "lion_affine_act_max_bwd_apply",
             "lion_trilinear_devoxelize_backward_affine")


@pytest.mark.parametrize("op,points", [(op, False) for op in sorted(KEEPS)] + [("adagn_act", True)])
def test_op_fills_only_the_gradient_slots_that_are_wanted(calls, op, points):
    # x wants none: no dx pass, x.grad stays None, every parameter gets its gradient
    run, x, params = _op_inputs(op, points=points)
    for p in params.values():
        p.requires_grad_(True)
    y = run()
    del calls[:]
    y.square().mean().backward()
    assert not any(n in DX_PASSES for n in calls), calls
    assert "lion_gn_train_param_grads" in calls
    assert x.grad is None and all(p.grad is not None for p in params.values())
    # only x wants one: the parameters' gradients stay None and nothing is launched for them -- behind a grid (5-D x) the launch is
    # there all the same, for its third output alone: the sum of dx per channel, the bias gradient of the Conv3d in front
    # (train_ops.tag_channel_sum; test_train_ops_gpu.py::test_conv3d_bias_gradient_rides_on_the_adagn_backward)
    run, x, params = _op_inputs(op, points=points)
    for p in params.values():
        p.requires_grad_(False)
        p.grad = None
    x.requires_grad_(True)
    y = run()
    del calls[:]
    y.square().mean().backward()
    assert sum(n in DX_PASSES for n in calls) == 1 and calls.count("lion_gn_train_param_grads") == (1 if x.dim() == 5 else 0), calls
    assert x.grad is not None and all(p.grad is None for p in params.values())
    # raw kernels: a backward through the backward raises
    run, x, params = _op_inputs(op, points=points)
    x.requires_grad_(True)
    (gx,) = torch.autograd.grad(run().square().mean(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.square().mean().backward()
