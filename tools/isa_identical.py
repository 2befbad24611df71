#!/usr/bin/env python3
"""Is the device code of two trees the same?  tools/isa_identical.py [--rename OLD=NEW[<ARGS>] ...] TREE_A TREE_B [file.hip ...]

Compiles every lion_amd/csrc/*.hip of both trees (or the named ones) with the FLAGS of csrc/build.sh without -fPIC, plus
-S --cuda-device-only, and compares the listings -- what a host-only refactor has to show.  A file whose two listings are
byte-identical is reported as such.  Otherwise (a listing carries a per-source id, and a changed host-side type can rename
a symbol) every device function is compared on its own, by the method of profiles/conv_split_unify_isa.txt:
  the lines from the function's label up to its .Lfunc_end, ';' comments stripped, .LBB<n>_<m> labels -> one token,
  mangled _Z... symbols -> one token, compared as lists; and NumVgprs, ScratchSize, Occupancy and
  .amdhsa_group_segment_fixed_size (static LDS; the dynamic part is a launch argument) compared as numbers.
Functions are paired by their demangled names.  --rename OLD=NEW (repeatable; kernel names without template arguments)
pairs TREE_A's OLD<args> with TREE_B's NEW<args>, --rename OLD=NEW<ARGS> with NEW<ARGS> whatever OLD's arguments and
parameter list were -- a kernel folded into a template:
  --rename 'devox_bwd_lds_kernel=devox_bwd_lds_kernel<false>' --rename 'devox_bwd_affine_kernel=devox_bwd_lds_kernel<true>'
One line per function, then ALL IDENTICAL or the number that differ
(exit status 1).  Needs no GPU.
"""
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_flags(tree):
    """FLAGS of that tree's csrc/build.sh, -fPIC and the relative include path replaced."""
    text = open(os.path.join(tree, "lion_amd/csrc/build.sh")).read()
    flags = re.search(r'^FLAGS="([^"]*)"', text, re.M).group(1).split()
    out = []
    for f in flags:
        if f == "-fPIC":
            continue
        if f.startswith("-I") and not os.path.isabs(f[2:]):
            f = "-I" + os.path.normpath(os.path.join(tree, "lion_amd/csrc", f[2:]))
        out.append(f)
    return out


def listing(tree, name, out):
    src = os.path.join(tree, "lion_amd/csrc", name)
    cmd = [HIPCC] + build_flags(tree) + ["-S", "--cuda-device-only", "-Wno-unused-command-line-argument", src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit("%s does not compile:\n%s" % (src, r.stdout))
    return open(out).read()


METRICS = (("vgprs", r"^; NumVgprs: (\d+)"), ("scratch", r"^; ScratchSize: (\d+)"), ("occupancy", r"^; Occupancy: (\d+)"),
           ("lds", r"^\s*\.amdhsa_group_segment_fixed_size (\d+)"))


def functions(text):
    """mangled name -> (normalised instruction list, metrics)"""
    lines = text.split("\n")
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", l)]
              if m and i >= 1 and any("@function" in p for p in lines[max(0, i - 3):i])]
    out = {}
    for k, (i, name) in enumerate(starts):
        stop = starts[k + 1][0] if k + 1 < len(starts) else len(lines)
        end = next((j for j in range(i, stop) if lines[j].startswith(".Lfunc_end")), stop)
        body = []
        for l in lines[i + 1:end]:
            l = l.split(";", 1)[0].strip()
            if not l:
                continue
            l = re.sub(r"\.LBB\d+_\d+", ".LBB", l)
            l = re.sub(r"\b_Z\w+", "SYM", l)
            body.append(re.sub(r"\s+", " ", l))
        tail = "\n".join(lines[i:stop])
        metrics = {}
        for key, pat in METRICS:
            m = re.search(pat, tail, re.M)
            metrics[key] = int(m.group(1)) if m else None
        out[name] = (body, metrics)
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not names or not filt:
        return {n: n for n in names}  # without a demangler the mangled names pair the functions
    r = subprocess.run([filt], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def short(name):
    name = name.replace("(anonymous namespace)::", "")
    head = re.match(r"^(?:void )?([\w:]+)(<.*>)?\(", name)
    if not head:
        return name, ""
    return head.group(1), head.group(2) or "<>"


def renamed(by_a, by_b, renames):
    """by_a re-keyed: a function of A that a rename names goes under the demangled name of its partner in B (if B has it)"""
    out = {}
    for d, k in by_a.items():
        kn, targs = short(d)
        if kn in renames:
            new, want = renames[kn]
            hits = [e for e in by_b if short(e) == (new, (want or targs).replace(" ", "")) or short(e) == (new, want or targs)]
            if len(hits) == 1:
                d = hits[0]
        out[d] = k
    return out


def main():
    argv, renames = [], {}
    it = iter(sys.argv[1:])
    for x in it:
        if x == "--rename" or x.startswith("--rename="):
            old, _, new = (next(it, "") if x == "--rename" else x[len("--rename="):]).partition("=")
            m = re.match(r"^([\w:]+)(<.*>)?$", new)
            if not old or not m:
                raise SystemExit("--rename OLD=NEW[<ARGS>]")
            renames[old] = (m.group(1), m.group(2))
        else:
            argv.append(x)
    if len(argv) < 2:
        raise SystemExit(__doc__)
    a, b = argv[0], argv[1]
    names = argv[2:] or sorted(set(f for t in (a, b) for f in os.listdir(os.path.join(t, "lion_amd/csrc"))
                                       if f.endswith(".hip")))
    ver = subprocess.run([HIPCC, "--version"], stdout=subprocess.PIPE, text=True).stdout.split("\n")
    print("compiler %s\n         %s" % (ver[1].strip(), ver[0].strip()))
    print("flags    %s -S --cuda-device-only" % " ".join(f for f in build_flags(b) if not f.startswith("-I")))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        jobs = {}
        for n in names:
            for side, tree in (("a", a), ("b", b)):
                if os.path.exists(os.path.join(tree, "lion_amd/csrc", n)):
                    jobs[n, side] = pool.submit(listing, tree, n, os.path.join(tmp, "%s.%s.s" % (n, side)))
        for n in names:
            if (n, "a") not in jobs or (n, "b") not in jobs:
                print("%-20s only in %s" % (n, a if (n, "a") in jobs else b))
                bad += 1
                continue
            ta, tb = jobs[n, "a"].result(), jobs[n, "b"].result()
            whole = ta == tb
            fa, fb = functions(ta), functions(tb)
            da, db = demangle(list(fa)), demangle(list(fb))
            by_a = {da[k]: k for k in fa}
            by_b = {db[k]: k for k in fb}
            by_a = renamed(by_a, by_b, renames)
            if not whole and not (set(by_a) & set(by_b)):  # nothing to compare: the listing's format is not understood
                print("%-20s listings differ and no device function was found in both  identical NO" % n)
                bad += 1
            width = max([len(short(d)[0]) for d in list(by_a) + list(by_b)] + [1])
            for d in sorted(set(by_a) | set(by_b)):
                kn, targs = short(d)
                if d not in by_a or d not in by_b:
                    print("%-20s %-*s %s  only in %s  identical NO" % (n, width, kn, targs, "A" if d in by_a else "B"))
                    bad += 1
                    continue
                (ia, ma), (ib, mb) = fa[by_a[d]], fb[by_b[d]]
                same = ia == ib and ma == mb
                bad += not same
                print("%-20s %-*s %s  insts %d  vgprs %s  scratch %s  occupancy %s  lds %s  identical %s" %
                      (n, width, kn, targs, len(ib), mb["vgprs"], mb["scratch"], mb["occupancy"], mb["lds"],
                       ("yes (whole listing byte-identical)" if whole else "yes") if same else
                       "NO (A: insts %d %s)" % (len(ia), ma)))
    print("ALL IDENTICAL" if not bad else "DIFFERENT: %d" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
