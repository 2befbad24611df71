"""Static checks on the compiled gfx950 code of csrc/conv3d_half.hip (no GPU: hipcc cross-compiles), for every
instantiation of its kernel: the MFMA count of one product per operand pair, no scratch access inside the tap walk, and
no weight DMA waited for in front of the MFMAs of its tap group."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lion_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _build_flags():
    """the compile flags of the product build, read from csrc/build.sh"""
    txt = open(os.path.join(CSRC, "build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]+)"', txt, re.M).group(1).split()
    return [f.replace("../../include", os.path.join(ROOT, "include")) for f in flags if f not in ("-fPIC",)]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """[(mangled name, instruction lines)] of every conv3d_half kernel"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("isa") / "conv3d_half.s")
    subprocess.check_call([HIPCC] + _build_flags() + ["-S", "--cuda-device-only", os.path.join(CSRC, "conv3d_half.hip"), "-o", out],
                          cwd=CSRC, stderr=subprocess.DEVNULL)
    listing = open(out).read()
    found = []
    for m in re.finditer(r'^(\S*conv3d_split_kernelILi\S*):', listing, re.M):
        end = re.compile(r'^\.Lfunc_end\d+:', re.M).search(listing, m.end()).start()
        body = [ln.strip().split(';')[0].strip() for ln in listing[m.end():end].split('\n')]
        found.append((m.group(1), [ln for ln in body if ln]))
    assert len(found) == 16, [n for n, _ in found]   # 2 resolutions x 2 channel tiles x (prologue, statistics)
    assert "conv3d_half" in open(os.path.join(CSRC, "build.sh")).read()   # and the file is part of the library
    return found


def test_one_mfma_per_operand_pair(kernels):
    """27 taps x CB channel blocks x 2 column blocks in the (single, straight-line) K-walk copy of the working waves: one
    third of the split kernel's 27 * 3 * CB * 2"""
    for name, body in kernels:
        cb = int(re.search(r'kernelILi\d+ELi\d+ELi\d+ELi(\d+)E', name).group(1))
        mf = [ln for ln in body if ln.startswith('v_mfma')]
        assert len(mf) == 27 * cb * 2, (name, len(mf))
        assert all(ln.startswith('v_mfma_f32_32x32x16_f16') for ln in mf), name


def test_no_scratch_access_inside_the_tap_walk(kernels):
    for name, body in kernels:
        mf = [i for i, ln in enumerate(body) if ln.startswith('v_mfma')]
        bad = [ln for ln in body[mf[0]:mf[-1]] if ln.startswith('scratch_')]
        assert not bad, (name, len(bad))


def test_weight_dma_is_not_drained_before_its_tap_groups_mfmas(kernels):
    """an LDS-DMA instruction followed, before the next MFMA, by a vmcnt wait that reaches it (wait vmcnt(N) reaches the DMA
    iff N <= VM operations issued behind it) would put the NEXT group's round trip in front of this group's MFMAs"""
    for name, body in kernels:
        n = n_mfma = drained_mfma = 0
        for i, ln in enumerate(body):
            if not ln.startswith('global_load_lds'):
                continue
            n += 1
            younger, hit, before_mfma = 0, False, False
            for b in body[i + 1:i + 400]:
                if b.startswith('v_mfma'):
                    before_mfma = True
                    break
                if b.startswith('s_barrier'):
                    break
                if re.match(r'(buffer|global|scratch|flat)_(load|store|atomic)', b):
                    younger += 1
                w = re.search(r'vmcnt\((\d+)\)', b) if b.startswith('s_waitcnt') else None
                if w and int(w.group(1)) <= younger:
                    hit = True
            n_mfma += before_mfma
            drained_mfma += hit and before_mfma
        assert n > 0 and n_mfma >= 27 and drained_mfma == 0, (name, n, n_mfma, drained_mfma)
