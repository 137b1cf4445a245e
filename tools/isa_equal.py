#!/usr/bin/env python3
"""Is the gfx950 device code of a .hip file the same as at another revision, kernel by kernel?

    tools/isa_equal.py <rev> <file.hip> [--old-file PATH] [--map OLD=NEW ...]

Compiles <file.hip> as it is at <rev> (taken from git together with the headers of that revision) and as it is in the
working tree, with the flags of tests/test_isa_checks.py, and compares every kernel: the lines from its label to its
.Lfunc_end plus its register-count records.  Normalised before comparing: __hip_cuid_<hex> (differs between any two
compiles), the function ordinal in local labels (.LBB<n>_, .Lfunc_end<n>, BB<n>_ in trailing comments: it follows the order
of instantiation), the padding in front of a trailing comment, and the renames given with --map (plain text replacement in
the OLD assembly, e.g. a template-argument list that lost members or an argument struct that was renamed).
Prints SAME / DIFF per kernel with the first differing lines; exits 1 on any DIFF or if the sets of kernels differ.
--old-file PATH: the kernels moved; PATH at <rev> is the old side (flow.hip at <rev> against the working tree's conv_f32.hip).
Then only the kernels both files hold are compared (ONLY lists the others), and REGS prints each compared kernel's register
records side by side.
Every instruction, label and directive must match; lines that hold only a comment are reported when they differ, not failed.
A refactor that is meant to leave the instructions alone is checked with this before it goes near a GPU.
"""
import argparse, difflib, io, os, re, subprocess, sys, tarfile, tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-result"]
RECORDS = ("num_vgpr", "num_agpr", "numbered_sgpr", "private_seg_size")


def assembly(src, out):
    subprocess.run(["hipcc", *FLAGS, src, "-o", out], check=True)
    with open(out) as f:
        text = f.read()
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", text)
    text = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+", r".\1", text)
    return re.sub(r"[ \t]+; (.*)\bBB\d+_", r" ; \1BB_", re.sub(r"[ \t]+;", " ;", text))   # the ordinal in a trailing "in Loop: Header=BB<n>_" too


def kernels(text):
    lines = text.split("\n")
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        recs = [l for l in lines if any(l.strip().startswith(".set %s.%s," % (name, r)) for r in RECORDS)]
        out[name] = lines[start:end + 1] + recs
    return out


def code(lines):
    return [l for l in lines if not l.lstrip().startswith(";")]   # everything but lines that hold only a comment


def records(lines):
    return " / ".join(l.split(",")[-1].strip() for l in lines if l.strip().startswith(".set "))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev")
    ap.add_argument("file")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--old-file", metavar="PATH", help="the file that held the kernels at <rev>, when they have moved")
    args = ap.parse_args()
    root = subprocess.run(["git", "rev-parse", "--show-toplevel"], check=True, capture_output=True, text=True).stdout.strip()
    rel = os.path.relpath(os.path.abspath(args.file), root)
    old_rel = os.path.relpath(os.path.abspath(args.old_file), root) if args.old_file else rel
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", root, "archive", args.rev], check=True, capture_output=True).stdout
        with tarfile.open(fileobj=io.BytesIO(tar)) as t:   # the file and every header of that revision, in place
            t.extractall(tmp, [m for m in t.getmembers() if m.name == old_rel or m.name.endswith((".h", ".hpp"))])
        old = assembly(os.path.join(tmp, old_rel), os.path.join(tmp, "old.s"))
        new = assembly(os.path.join(root, rel), os.path.join(tmp, "new.s"))
    for m in args.map:
        o, n = m.split("=", 1)
        old = old.replace(o, n)
    ko, kn = kernels(old), kernels(new)
    bad = 0
    for name in sorted(set(ko) | set(kn)):
        if name not in ko or name not in kn:
            where = "the working tree" if name in kn else args.rev
            if args.old_file:            # the two files are expected to hold other kernels too
                print("ONLY %s: in %s" % (name, where))
            else:
                print("DIFF %s: only in %s" % (name, where))
                bad += 1
            continue
        if args.old_file:
            print("REGS %s: %s = %s at %s, %s here" % (name, " / ".join(RECORDS), records(ko[name]), args.rev, records(kn[name])))
        if code(ko[name]) != code(kn[name]):
            print("DIFF %s" % name)
            delta = [l for l in difflib.unified_diff(code(ko[name]), code(kn[name]), args.rev, "working tree", lineterm="", n=0)]
            print("\n".join("    " + l for l in delta[:12]))
            bad += 1
        elif ko[name] != kn[name]:   # e.g. the register allocator's "; implicit-def: $vgpr122" notes in another order
            moved = sum(1 for l in difflib.ndiff(ko[name], kn[name]) if l[:1] in "+-")
            print("SAME %s (%d lines; %d comment-only lines differ)" % (name, len(kn[name]), moved))
        else:
            print("SAME %s (%d lines)" % (name, len(kn[name])))
    print("%s: %d kernels at %s%s, %d in the working tree, %d differ" %
          (rel, len(ko), args.rev, " in " + old_rel if args.old_file else "", len(kn), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
