"""Which KERNELS of two device-assembly files differ?  (tools/device_asm_equal.sh compares whole units; it calls this for a unit
it reports DIFFERENT.)

    python3 tools/device_asm_kernels.py A.s B.s [B2.s ...] [--rename-b PATTERN REPLACEMENT] [--only-b]

Several B files are taken together: a kernel of A is looked up in all of them, so one that moved to another unit (a unit split
by kernel family) is found where it went.  Kernel names carry no file name (_ZN12_GLOBAL__N_1...), so nothing needs renaming.

A kernel is the text from its label to its .Lfunc_end; the ordinal of the function in the file, which the assembler's local
labels and loop comments carry (.LBB12_3, BB12_3, .Lfunc_end12), is taken out, so a kernel that merely moved compares equal;
runs of blanks count as one (the comment behind a label is padded by the label's length, which carries the ordinal's digits).
--rename-b rewrites B's text first (a regular expression), for a kernel whose NAME changed: e.g. a template that gained a
defaulted argument.  Prints one line per kernel: same / DIFFERENT (with the differing lines counted) / only in A / only in B
(the last with one B file only: against several, A's unit is no measure of what B added); exit status 1 when a kernel of A is
missing from B or differs.  --only-b: A may be several units' text in one file; prints just the kernels of B that A lacks, exit
status 1 when there is one."""
import argparse
import difflib
import re
import sys


def kernels(text):
    out, cur = {}, None
    for line in text.splitlines():
        if re.match(r"\s*\.(file|ident|loc)\b", line):
            continue
        line = re.sub(r"__hip_cuid_[0-9a-f]*", "__hip_cuid_X", line)
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is not None:
            line = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", re.sub(r"BB\d+_", "BB_", line))
            line = re.sub(r"[ \t]+", " ", line)
            out[cur].append(line)
            if line.startswith(".Lfunc_end"):
                cur = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a"); ap.add_argument("b", nargs="+")
    ap.add_argument("--rename-b", nargs=2, metavar=("PATTERN", "REPLACEMENT"))
    ap.add_argument("--show", type=int, default=0, help="print this many differing lines per kernel")
    ap.add_argument("--only-b", action="store_true", help="list only the kernels of B that A lacks")
    args = ap.parse_args()
    ta, tb = open(args.a).read(), "\n".join(open(b).read() for b in args.b)
    if args.rename_b:
        tb = re.sub(args.rename_b[0], args.rename_b[1], tb)
    ka, kb = kernels(ta), kernels(tb)
    if args.only_b:
        new = [name for name in kb if name not in ka]
        for name in new:
            print(f"only in B   {name}")
        sys.exit(1 if new else 0)
    rc = 0
    for name, body in ka.items():
        if name not in kb:
            print(f"only in A   {name}"); rc = 1
        elif body == kb[name]:
            print(f"same        {name}")
        else:
            d = [l for l in difflib.unified_diff(body, kb[name], n=0, lineterm="") if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            print(f"DIFFERENT   {name}  ({len(d)} lines of {len(body)})"); rc = 1
            for l in d[:args.show]:
                print("    " + l)
    for name in kb if len(args.b) == 1 else ():
        if name not in ka:
            print(f"only in B   {name}")
    sys.exit(rc)


if __name__ == "__main__":
    main()
