"""-m gpu: lion_skinny_gemm and lion_skinny_gemm_se_finish -- every load of a round requested before the first wait,
dead chunks not loaded, the tail's inputs requested at kernel entry -- against the plain kernel they replaced
(lion_internal_skinny_gemm_plain / lion_internal_skinny_gemm_se_finish_plain), bit for bit on int32 views, so that a NaN
and the sign of a zero count.  Only the memory schedule differs between the two: any difference at all is a bug."""
import pytest
import torch

from test_skinny_numerics_gpu import BATCH, KS_IN, TABLE, gen_for, lib, pack, plan

pytestmark = pytest.mark.gpu

RELEASED = [(2048, 2048), (2048, 256), (256, 2048)]   # conv1 / conv2, SE fc1, SE fc2 of the released global prior
SHAPES = sorted(TABLE) + RELEASED
DATA = ("gauss", "nan-inf-last-channel", "zero-operand")


def bits(t):
    return t.contiguous().view(torch.int32)


def slices(cin, cout):
    """(s_lo, s_hi, per) of every wave of every k-split, by the kernel's formulas"""
    ks, per, _ = plan(cin, cout)
    ksteps = (cin + 1) // 2
    out = []
    for s in range(ks):
        for wave in range(16):
            s_lo = min(ksteps, (s * 16 + wave) * per)
            out.append((s_lo, min(ksteps, s_lo + per), per))
    return out


def test_table_holds_dead_chunks_and_repeated_rounds():
    """a chunk (4 k-steps) of a round is dead when it starts at or beyond the slice's s_hi: the new kernel loads nothing for
    it.  The shapes must hold slices with live and dead chunks in one round, wholly dead slices, and slices of more than
    one round; the released SE layers run two live and two dead chunks per slice."""
    mixed = idle = rounds = 0
    for cin, cout in SHAPES:
        assert lib().lion_skinny_splits(cin, cout) == plan(cin, cout)[0]
        for s_lo, s_hi, per in slices(cin, cout):
            rounds += per > 16
            idle += s_lo == s_hi
            for r0 in range(0, per, 16):
                live = [s_lo + r0 + 4 * g < s_hi for g in range(4)]
                mixed += any(live) and not all(live)
    assert mixed and idle and rounds, (mixed, idle, rounds)
    for cin, cout in RELEASED[1:]:
        for s_lo, s_hi, per in slices(cin, cout):
            assert per == 8 and [s_lo + 4 * g < s_hi for g in range(4)] == [True, True, False, False]


def inputs(cin, cout, nb, data):
    gen = gen_for("roundtrips", cin, cout, nb, data)

    def rn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen)
    w, pin8 = rn(cout, cin), rn(max(KS_IN), nb, cin, 32)
    if data == "nan-inf-last-channel":   # the channel that lanes beyond the end re-read before their operand is zeroed
        pin8[0, nb - 1, cin - 1, 5] = float("nan")
        pin8[-1, 0, cin - 1, 9] = float("inf")
    if data == "zero-operand":   # every product is -0 or +0, but for one -inf weight: 0 * -inf must stay the NaN it is
        pin8.zero_()
        w = -w.abs()
        w[0, cin - 1] = float("-inf")
    return dict(wp=pack(w), pin8=pin8, bias_in=rn(cin), addT=rn(nb, cin, 32), A4=rn(4, nb, cout, 32), bias_a=rn(cout),
                resid=rn(nb, cout, 32))


def run_gemm(name, pin, bias_in, act_in, addT, wp, cout):
    from lion_amd import _lib
    ks_in, nb, cin, _ = pin.shape
    out = torch.full((lib().lion_skinny_splits(cin, cout), nb, cout, 32), float("nan"), device="cuda")
    _lib.call(name, pin, ks_in, bias_in, act_in, addT, wp, nb, cin, cout, out)
    return out


def run_fin(name, pin, bias_in, act_in, wp, cout, A, bias_a, resid):
    from lion_amd import _lib
    ks_in, nb, cin, _ = pin.shape
    y = torch.full((nb, cout, 32), float("nan"), device="cuda")
    _lib.call(name, pin, ks_in, bias_in, act_in, wp, nb, cin, cout, A, A.shape[0], bias_a, resid, y)
    return y


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_public_entry_points_equal_the_plain_kernel_bit_for_bit(cin, cout, nb):
    assert nb in BATCH
    fin = lib().lion_skinny_splits(cin, cout) == 1
    for data in DATA:
        t = inputs(cin, cout, nb, data)
        if data == "gauss":   # the plain output is a real result, not a tensor of NaNs
            assert torch.isfinite(run_gemm("lion_internal_skinny_gemm_plain", t["pin8"][:4].contiguous(), t["bias_in"], 1,
                                           t["addT"], t["wp"], cout)).all()
        for ks_in in KS_IN:
            pin = t["pin8"][:ks_in].contiguous()
            for act_in in (0, 1):
                for bi in (None, t["bias_in"]):
                    for ad in (None, t["addT"]):
                        got = run_gemm("lion_skinny_gemm", pin, bi, act_in, ad, t["wp"], cout)
                        ref = run_gemm("lion_internal_skinny_gemm_plain", pin, bi, act_in, ad, t["wp"], cout)
                        tag = (cin, cout, nb, data, ks_in, act_in, bi is not None, ad is not None)
                        assert torch.equal(bits(got), bits(ref)), (tag, int((bits(got) != bits(ref)).sum()))
                    if not fin:
                        continue
                    for ks_a in (1, 4):
                        A = t["A4"][:ks_a].contiguous()
                        for ba in (None, t["bias_a"]):
                            got = run_fin("lion_skinny_gemm_se_finish", pin, bi, act_in, t["wp"], cout, A, ba, t["resid"])
                            ref = run_fin("lion_internal_skinny_gemm_se_finish_plain", pin, bi, act_in, t["wp"], cout, A, ba,
                                          t["resid"])
                            tag = (cin, cout, nb, data, ks_in, act_in, bi is not None, "fin", ks_a, ba is not None)
                            assert torch.equal(bits(got), bits(ref)), (tag, int((bits(got) != bits(ref)).sum()))


def test_more_than_eight_partials_take_the_plain_kernel():
    """ks_in > 8 is the cut between the two kernels: both entry points run the plain one there"""
    cin, cout, nb = 129, 32, 1
    t = inputs(cin, cout, nb, "gauss")
    pin = torch.randn(9, nb, cin, 32, device="cuda", generator=gen_for("nine"))
    got = run_gemm("lion_skinny_gemm", pin, t["bias_in"], 1, t["addT"], t["wp"], cout)
    ref = run_gemm("lion_internal_skinny_gemm_plain", pin, t["bias_in"], 1, t["addT"], t["wp"], cout)
    assert torch.isfinite(ref).all() and torch.equal(bits(got), bits(ref))
