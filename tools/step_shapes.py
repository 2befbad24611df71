"""Shapes of a sampling step's small serial launches, for tools/small_launch_bench.py: runs bench.py's sampler for two steps
with lion_amd._lib.call wrapped, and writes one JSON list of the distinct cases (per batch size) of
  fold_tconst  conv1's lion_groupnorm_fold + conv2's lion_conv3d_const_response of a PVConv
  fold_se      lion_groupnorm_fold_se
  pw           lion_pwconv_forward / lion_pwconv_grouped_forward at L <= 4096 (the short-activation kernel)
with the number of launches of each per step.  usage: step_shapes.py OUT.json [BATCH]"""
import collections, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
out, batch = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "32")
from lion_amd import _lib

seen, real, last_fold = collections.Counter(), _lib.call, [0, 0, 0]


def call(name, *a, **kw):
    if name == "lion_groupnorm_fold":
        last_fold[:] = [a[2], a[3], a[4]]
    elif name == "lion_conv3d_const_response":   # follows the fold of the convolution in front of it
        seen[("fold_tconst", ("C", last_fold[0]), ("T", last_fold[1]), ("G", last_fold[2]), ("Cout", a[7]))] += 1
    elif name == "lion_groupnorm_fold_se":
        seen[("fold_se", ("C", a[2]), ("T", a[3]), ("G", a[4]), ("H", a[14]))] += 1
    elif name == "lion_pwconv_forward" and a[6] <= 4096:
        seen[("pw", ("Cin", a[4]), ("Cout", a[5]), ("L", a[6]), ("pro", a[7] is not None), ("stats", a[10] is not None))] += 1
    elif name == "lion_pwconv_grouped_forward" and a[9] * a[10] <= 4096:
        seen[("pw_grouped", ("C", a[7]), ("N", a[8]), ("M", a[9]), ("U", a[10]), ("Cout", a[11]), ("stats", a[13] is not None))] += 1
    return real(name, *a, **kw)


_lib.call = call
import bench
sys.argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "0", "--batch", batch, "--repeats", "1", "--no-graph",
            "--no-cpu-baseline", "--no-dense-check", "--no-full-chain", "--forced-steps", "0", "--small-batches", ""]
bench.main()
cases = [dict(kind=k[0], launches=n, **dict(k[1:])) for k, n in sorted(seen.items())]
json.dump(cases, open(out, "w"), indent=1)
for c in cases:
    print(c)
