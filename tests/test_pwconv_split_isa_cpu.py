"""Static checks on the compiled split-operand 1x1 convolution (csrc/pwconv_split.hip; no GPU: hipcc cross-compiles): the
WIDE instantiations move the activation in 16-byte pieces only, the 4-byte instantiations are still there as the fallback,
and no instantiation needs more scratch than before the 16-byte transport was added."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lion_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

# bytes of scratch per lane of pwconv_split_kernel<CB, VB, PRO, STATS, 5> before the wide transport (same compiler, the
# flags of csrc/build.sh): the 4-byte instantiations must not exceed their own value, the wide ones not that of the
# 4-byte instantiation they replace
SCRATCH_BEFORE = {(4, 1, 1, 1): 0, (4, 1, 1, 0): 0, (4, 1, 0, 1): 0, (4, 1, 0, 0): 0,
                  (2, 2, 1, 1): 56, (2, 2, 1, 0): 28, (2, 2, 0, 1): 312, (2, 2, 0, 0): 300,
                  (1, 2, 1, 1): 0, (1, 2, 1, 0): 0, (1, 2, 0, 1): 40, (1, 2, 0, 0): 32}


def _build_flags():
    txt = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]+)"', txt, re.M).group(1).split()
    return [f.replace("../../include", os.path.join(ROOT, "include")) for f in flags if f not in ("-fPIC",)]


@pytest.fixture(scope="module")
def instantiations(tmp_path_factory):
    """{(CB, VB, PRO, STATS, WIDE): (instruction lines, scratch bytes)} of every pwconv_split_kernel in the listing"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / "pwconv_split.s")
    subprocess.check_call([HIPCC] + _build_flags() + ["-S", "--cuda-device-only", os.path.join(CSRC, "pwconv_split.hip"),
                                                      "-o", out], cwd=CSRC, stderr=subprocess.DEVNULL)
    lst = open(out).read()
    found = {}
    for m in re.finditer(r'^(\S*pwconv_split_kernelILi(\d)ELi(\d)ELb(\d)ELb(\d)ELi\d+ELb(\d)E\S*):', lst, re.M):
        end = re.compile(r'^\.Lfunc_end\d+:', re.M).search(lst, m.end()).start()
        body = [ln.strip().split(';')[0].strip() for ln in lst[m.end():end].split('\n')]
        scratch = int(re.search(r'^; ScratchSize: (\d+)', lst[m.end():], re.M).group(1))
        found[tuple(int(g) for g in m.groups()[1:])] = ([ln for ln in body if ln], scratch)
    return found


def _is_dma(ln):
    return bool(re.match(r'buffer_load_dwordx4 .*\blds$', ln)) or ln.startswith('global_load_lds')


def test_all_instantiations_exist(instantiations):
    """12 wide + the 12 4-byte ones the launcher falls back to"""
    want = {k + (w,) for k in SCRATCH_BEFORE for w in (0, 1)}
    assert set(instantiations) == want, sorted(set(instantiations) ^ want)


def test_wide_k_loop_has_no_4_byte_activation_loads(instantiations):
    """the activation rows arrive by 16-byte LDS-DMA: the only loads into registers (AdaGN scale / shift, bias) come before
    the first DMA is issued, and there is no buffer load into registers at all"""
    for key, (body, _) in instantiations.items():
        if not key[4]:
            continue
        rows = [i for i, ln in enumerate(body) if re.match(r'buffer_load_dwordx4 .*\blds$', ln)]
        assert len(rows) >= 2 * key[1] * 2, (key, len(rows))      # prologue + loop, 2 VB per wave and chunk
        first = min(i for i, ln in enumerate(body) if _is_dma(ln))
        for i, ln in enumerate(body):
            if re.match(r'(buffer|global|flat|scratch)_load', ln) and not _is_dma(ln):
                assert not ln.startswith('buffer_load') and i < first, (key, i, ln)


def test_wide_epilogue_stores_16_bytes(instantiations):
    """y leaves as 16-byte stores: 4 per 32 x 32 block of a wave; the one narrower store is the (sum, sum of squares) pair"""
    for key, (body, _) in instantiations.items():
        if not key[4]:
            continue
        cb, vb, _, stats, _ = key
        stores = [ln.split()[0] for ln in body if re.match(r'(global|buffer|flat)_store', ln)]
        assert stores.count('global_store_dwordx4') == 4 * cb * vb, (key, stores)
        assert [s for s in stores if s != 'global_store_dwordx4'] == (['global_store_dwordx2'] if stats else []), (key, stores)


def test_fallback_keeps_the_4_byte_transport(instantiations):
    for key, (body, _) in instantiations.items():
        if key[4]:
            continue
        assert any(re.match(r'buffer_load_dword ', ln) for ln in body), key
        assert any(re.match(r'global_store_dword ', ln) for ln in body), key
        assert not any(re.match(r'buffer_load_dwordx4 .*\blds$', ln) for ln in body), key


def test_no_instantiation_gains_scratch(instantiations):
    for key, (_, scratch) in instantiations.items():
        assert scratch <= SCRATCH_BEFORE[key[:4]], (key, scratch)
