"""CPU suite: the C-ABI library loads here (no GPU) and exports every symbol include/lion_hip.h
declares; the product fails loudly (no CPU fallback) when handed CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

import abi_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = abi_check.header()
    return sorted(set(re.findall(r"\b(lion_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from lion_amd import _lib
    names = _declared()
    assert len(names) >= 20
    abi_check.declared_bound_and_exported(names, returns=r"\w+")
    # and the ctypes table binds exactly the declared set
    assert sorted(_lib.SIGNATURES) == names
    assert _lib.load().lion_abi_version() == 1


def test_workspace_queries_are_pure_host_calls():
    from lion_amd import _lib
    l = _lib.load()
    assert l.lion_avg_voxelize_workspace_bytes(32, 64, 2048, 32) >= 32 * 2048 * 4
    assert l.lion_avg_voxelize_workspace_bytes(0, 1, 1, 1) == 0
    assert l.lion_emd_workspace_bytes(2, 2048, 2048) >= 2 * 4 * 2048 * 4


def test_no_cpu_fallback():
    from lion_amd.functional.backend import _backend
    import lion_amd.functional as F
    with pytest.raises(RuntimeError):
        _backend.avg_voxelize_forward(torch.zeros(1, 2, 8), torch.zeros(1, 3, 8, dtype=torch.int32), 4)
    with pytest.raises(RuntimeError):
        F.ball_query(torch.zeros(1, 3, 4), torch.zeros(1, 3, 8), 0.1, 4)
    with pytest.raises(RuntimeError):
        F.furthest_point_sample(torch.zeros(1, 3, 8), 4)


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: no file under lion_amd/ may mention it."""
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "lion_amd")):
        for fn in fns:
            if fn.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, fn)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M) or "liboracle" in src:
                    bad.append(os.path.join(dp, fn))
    assert not bad, bad


def test_weight_cache_never_serves_a_freed_tensors_copy():
    """lion_amd._wcache.WeightCache: entries are keyed by storage address, validated by the version counter and hold a
    strong reference to their source tensor -- a new tensor can therefore never inherit the derived copy of a freed
    one that happened to live at the same address (the failure mode of an id()-keyed cache)."""
    import gc
    import torch
    from lion_amd._wcache import WeightCache
    builds = []

    def build(w):
        builds.append(w.data_ptr())
        return w.detach().clone() * 2

    cache = WeightCache(build, capacity=4)
    a = torch.arange(6.0).reshape(2, 3)
    assert torch.equal(cache.get(a), a * 2) and len(builds) == 1
    assert cache.get(a) is cache.get(a) and len(builds) == 1          # hit
    a.add_(1.0)                                                         # in-place update bumps the version
    assert torch.equal(cache.get(a), a * 2) and len(builds) == 2
    ptr = a.data_ptr()
    del a
    gc.collect()
    b = torch.full((2, 3), 7.0)                                         # may or may not reuse a's block ...
    assert torch.equal(cache.get(b), b * 2)                             # ... the result is right either way
    assert b.data_ptr() != ptr or len(builds) >= 3                      # and a reused address would have rebuilt
    for i in range(8):                                                  # capacity bound (LRU)
        cache.get(torch.zeros(1 + i))
    assert len(cache._entries) <= 4


def test_host_side_plan_functions():
    """size / plan helpers of the C ABI are pure host code: pin the values the Python shim relies on."""
    from lion_amd import _lib
    lib = _lib.load()
    # Conv3d tile plans: dense 4x2 MFMA tiles where >= 512 workgroups remain, 2x2 tiles for sparse launches
    assert lib.lion_conv3d_stat_tiles(32, 64, 32, 0) == 32768 // 512
    assert lib.lion_conv3d_stat_tiles(32, 64, 32, 1) == 32768 // 256
    assert lib.lion_conv3d_stat_tiles(16, 64, 32, 0) == 4096 // 256      # 8 x 1 x 32 = 256 < 512 -> 2x2 tiles
    assert lib.lion_conv3d_stat_tiles(16, 128, 32, 0) == 4096 // 512
    assert lib.lion_conv3d_stat_tiles(8, 128, 32, 0) == 512 // 128        # r = 8: one MFMA column block per wave
    assert lib.lion_conv3d_stat_tiles(7, 64, 32, 0) == 0
    assert lib.lion_conv3d_occupancy_ints(32, 64, 32) == 2 * 32 * 128 + 4    # flags, list, [queue, exit counter, mode, pad]
    assert lib.lion_conv3d_occupancy_ints(8, 64, 32) == 0                  # never sparse at r = 8
    assert lib.lion_conv3d_packed_floats(64, 3) == 4 * 27 * 64             # Cin padded to 4
    assert lib.lion_conv3d_wgrad_workspace_floats(32, 64, 64, 32) == 32 * 1 * 64 * 64 * 27 + 64   # one partial per workgroup (round 3) + the split kernel's maxima / scales (round 4)
    assert lib.lion_conv3d_wgrad_workspace_floats(32, 32, 32, 32) == 32 * 4 * 32 * 32 * 27 + 64  # 4 spatial splits
    assert lib.lion_conv3d_wgrad_workspace_floats(32, 3, 32, 32) == 0      # Cin % 4 != 0: library fallback
    # devoxelize plans (r = 32, N <= 2048): per cloud a 16-byte header, 2304 piece ids, 8 corner offsets and a status per point
    assert lib.lion_devoxelize_plan_bytes(32, 2048, 32) == 32 * (16 + 2304 * 2 + 2048 * 16 + 2048)
    assert lib.lion_devoxelize_plan_bytes(3, 999, 32) == 3 * (16 + 2304 * 2 + 2048 * 16 + 2048)
    assert lib.lion_devoxelize_plan_bytes(32, 2048, 16) == 0 and lib.lion_devoxelize_plan_bytes(32, 4096, 32) == 0
    # pointwise conv: column tiles of 4 waves x VB x 32 columns
    assert lib.lion_pwconv_stat_tiles(64, 35, 32768) == 32768 // 512
    assert lib.lion_pwconv_stat_tiles(128, 64, 8000) == -(-8000 // 256)
    assert lib.lion_pwconv_stat_tiles(48, 16, 10000) == -(-10000 // 512)   # 48 -> two 32-row tiles, one half masked
    assert lib.lion_pwconv_stat_tiles(256, 320, 8192) == 8192 // 512        # 256 / 128 rows x 320 k do not fit LDS: 64-row tiles
    assert lib.lion_pwconv_stat_tiles(4, 128, 2048) == 2048 // 32           # <= 4096 columns: the K-split kernel, 32-column tiles
    assert lib.lion_pwconv_stat_tiles(128, 256, 64) == 2
    # split-operand 1x1 kernel: 4 waves x VB x 32 columns per workgroup, VB = 1 / 2 / 2 for channel tiles of 128 / 64 / 32
    assert lib.lion_pwconv_split_stat_tiles(128, 192, 2048) == 2048 // 128
    assert lib.lion_pwconv_split_stat_tiles(64, 35, 32768) == 32768 // 256
    assert lib.lion_pwconv_split_stat_tiles(96, 16, 1000) == -(-1000 // 256)
    assert lib.lion_pwconv_split_packed_halfs(128, 35) == 3 * 4 * 128 * 8 + 8      # ceil16(35) = 3 chunks + the scale tail
    assert lib.lion_conv3d_split_stat_tiles(8, 128) == 2 and lib.lion_conv3d_split_stat_tiles(32, 64) == 128
    assert lib.lion_pwconv_packed_floats(64, 35) == 36 * 64 and lib.lion_pwconv_packed_floats(4, 128) == 128 * 64
    # skinny GEMM: split K until ~256 workgroups, >= 8 k-steps per wave
    assert lib.lion_skinny_splits(2048, 2048) == 4
    assert lib.lion_skinny_splits(2048, 256) == 8                        # 8 output tiles only: split K further
    assert lib.lion_skinny_splits(256, 2048) == 1
    assert lib.lion_skinny_splits(128, 48) == 0
    assert lib.lion_skinny_packed_floats(2048, 2048) == 2048 * 8 * 256


_CTYPE = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32,
          "lionStream_t": ctypes.c_void_p}


def _prototypes():
    """include/lion_hip.h -> {name: (restype, [argtypes], [C type words of each parameter])}: comments and preprocessor lines
    stripped, every `ret name(args);`; a parameter with a `*` is a pointer, the others go by their type name"""
    txt = open(os.path.join(ROOT, "include", "lion_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    txt = re.sub(r"^\s*#[^\n]*", "", txt, flags=re.M)
    protos = {}
    for ret, name, args in re.findall(r"\b(\w+)\s+(lion_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt):
        params = [] if args.strip() in ("", "void") else [" ".join(a.split()) for a in args.split(",")]
        kinds = []
        for p in params:
            words = [w for w in re.findall(r"\w+", p) if w != "const"]
            kinds.append("*" if "*" in p else words[0])    # words[-1] is the parameter's name
        protos[name] = (_CTYPE[ret], [ctypes.c_void_p if k == "*" else _CTYPE[k] for k in kinds], kinds)
    return protos


def test_ctypes_table_matches_the_header_by_type():
    """every return and argument type of _lib.SIGNATURES is the header's (an int bound where the header says size_t truncates
    silently), and every entry point has the shape _lib.call relies on: a function with a pointer parameter returns int and
    takes exactly one lionStream_t, as its last parameter; a function without one takes no stream"""
    from lion_amd import _lib
    protos = _prototypes()
    assert sorted(protos) == _declared() == sorted(_lib.SIGNATURES)
    for name, (res, args, kinds) in protos.items():
        assert _lib.SIGNATURES[name][0] is res, f"{name}: return type"
        bound = _lib.SIGNATURES[name][1]
        assert len(bound) == len(args), f"{name}: {len(bound)} bound arguments, {len(args)} declared"
        for i, (a, b) in enumerate(zip(bound, args)):
            assert a is b, f"{name}: argument {i} bound as {a.__name__}, declared {kinds[i]}"
        launches = "*" in kinds
        assert (bool(kinds) and kinds[-1] == "lionStream_t") == launches, f"{name}: stream iff pointers"
        assert kinds.count("lionStream_t") == (1 if launches else 0), name
        assert not launches or res is ctypes.c_int, f"{name}: a launch returns int"


def test_call_refuses_cpu_tensors_before_the_library():
    """_lib.call checks the device of every tensor before the library is entered: a CPU tensor is an exception that says so,
    never a pointer handed to a kernel -- also through entry points that had no check of their own"""
    from lion_amd import _lib, fused_ops, train_ops
    x, out = torch.zeros(4, 8), torch.zeros(4, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _lib.call("lion_row_stats", x, 4, 8, out)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused_ops.row_stats(torch.zeros(2, 3, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        train_ops.linear_attention_core(torch.zeros(1, 96, 8), 1)


def test_call_checks_the_argument_count():
    """one argument too few: a TypeError that names the symbol, raised before anything is launched"""
    from lion_amd import _lib
    with pytest.raises(TypeError, match="lion_row_stats"):
        _lib.call("lion_row_stats", None, 4, 8)
    with pytest.raises(TypeError, match="lion_row_stats"):
        _lib.call("lion_row_stats", None, 4, 8, None, None)


def test_every_launch_goes_through_call():
    """no file under lion_amd/ other than _lib.py builds a launch by hand (pointer, stream and error label per site)"""
    bad = []
    for dp, _, fns in os.walk(os.path.join(ROOT, "lion_amd")):
        for fn in fns:
            path = os.path.join(dp, fn)
            if fn.endswith(".py") and os.path.relpath(path, ROOT) != os.path.join("lion_amd", "_lib.py"):
                src = open(path).read()
                bad += [f"{path}: {w}" for w in ("_lib.ptr(", "_lib.stream_ptr(", "_lib.check(") if w in src]
    assert not bad, bad
