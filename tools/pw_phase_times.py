"""Per-chunk timeline (s_memtime) of wave 0 of workgroup 0 of the split-operand 1x1 convolution: wait, barrier, prefetch issue,
cut, MFMAs, then the epilogue (needs tools/exp/liblion_timing.so, see tools/build_timing_lib.sh).
usage: pw_phase_times.py [CIN:COUT:L[:p] ...]   (p = with the AdaGN prologue); B = 32, statistics on."""
import ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lion_amd import _lib, fused_ops as fo
lib = _lib.load()
lib.lion_debug_pws_times.restype = ctypes.c_int
lib.lion_debug_pws_times.argtypes = [ctypes.c_void_p]
shapes = [(192, 128, 2048, False), (128, 128, 2048, True), (128, 128, 256, False)]
if len(sys.argv) > 1:
    shapes = [tuple(int(v) for v in a.split(":")[:3]) + (a.endswith(":p"),) for a in sys.argv[1:]]
B = 32
for cin, cout, L, pro in shapes:
    torch.manual_seed(0)
    conv = torch.nn.Conv1d(cin, cout, 1).cuda(); x = torch.randn(B, cin, L, device="cuda")
    p = (torch.randn(B, cin, device="cuda") * 0.5 + 1.0, torch.randn(B, cin, device="cuda") * 0.3) if pro else None
    with torch.no_grad():
        for _ in range(3): fo.pwconv_fused(x, conv, p, split=True)
    torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * 128)()
    lib.lion_debug_pws_times(buf)
    t0 = buf[0]
    n = (cin + 15) // 16
    print(f"{cin}->{cout} L={L}{' +prologue' if pro else ''}: prologue issued {buf[1]-t0}")
    tot = dict(wait=buf[1] - t0, barrier=0, issue=0, cut=0, mfma=0)
    prev = buf[1]
    for q in range(n + 4):
        if not prev <= buf[2 + 4*q] <= buf[100] or 5 + 4*q >= 100: break   # outside this launch: left over from an earlier, longer one
        cut, mf = ((buf[64+q]-buf[4+4*q]), (buf[5+4*q]-buf[64+q])) if q < n else (0, 0)
        print(f"  chunk {q}: wait_done +{buf[2+4*q]-t0}  barrier +{buf[3+4*q]-buf[2+4*q]}  issue +{buf[4+4*q]-buf[3+4*q]}  cut +{cut} mfma +{mf}")
        tot["wait"] += buf[2+4*q] - prev; tot["barrier"] += buf[3+4*q]-buf[2+4*q]; tot["issue"] += buf[4+4*q]-buf[3+4*q]
        tot["cut"] += cut; tot["mfma"] += mf
        prev = buf[5+4*q] if q < n else buf[4+4*q]
    print(f"  loop end {buf[100]-t0}  stores +{buf[102]-buf[100]}  stats regs +{buf[103]-buf[102]}  stats out +{buf[101]-buf[103]}")
    whole = buf[101] - t0
    print(f"  split of {whole} ticks: rows wait {tot['wait']}  barrier {tot['barrier']}  prefetch issue {tot['issue']}  cut {tot['cut']}  mfma {tot['mfma']}"
          f"  stores {buf[102]-buf[100]}  statistics {buf[101]-buf[102]}")
