"""Compare kernels' instruction streams between two device assembly files (no GPU needed), for a refactor that
should leave the compiled code as it is:

    hipcc <the Makefile's FLAGS> --cuda-device-only -S -o old.s csrc/bplhip.hip      (once per tree)
    python tools/isa_diff.py old.s new.s OLD_PATTERN=NEW_PATTERN [...] [--out FILE]
    python tools/isa_diff.py old.s new.s --all [--out FILE]

Each pattern is a regular expression that must match exactly one kernel label (mangled name) of its file; a
bare PATTERN stands for PATTERN=PATTERN.  Of each kernel the lines between its label and its .Lfunc_end are
taken, comments and assembler directives dropped and the function number in .LBB labels removed; what is left
is compared line by line.  Prints, per pair, the instruction counts, the differing lines, and the VGPR, SGPR,
LDS and scratch figures of both kernels from the files' amdhsa metadata.  Exits 1 when a pair differs in
length or a pattern does not pick one kernel, 0 otherwise: the differing lines are for the reader to judge.
With --all every kernel is compared with the kernel of the same name in the other file, wherever it stands there:
the kernel count, then one line per kernel, "equal" when lines and figures are; exits 1 unless all are."""
import argparse
import difflib
import re
import sys

LABEL = re.compile(r"^(_Z\w+):")
FIGURES = (("vgpr", r"\.vgpr_count:\s+(\d+)"), ("sgpr", r"\.sgpr_count:\s+(\d+)"),
           ("lds", r"\.group_segment_fixed_size:\s+(\d+)"), ("scratch", r"\.private_segment_fixed_size:\s+(\d+)"))


def kernels(path):
    """{mangled name: [instruction and label lines]} and {mangled name: {figure: value}}."""
    body, name, out = None, None, {}
    with open(path) as f:
        text = f.read()
    for line in text.split("\n"):
        m = LABEL.match(line)
        if m and body is None:
            name, body = m.group(1), []
            continue
        if body is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], body = body, None
            continue
        line = line.split(";")[0].rstrip()
        if not line.strip() or (line[0] in " \t" and line.strip().startswith(".")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    meta = {}
    for block in text.split("- .agpr_count:")[1:]:
        n = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[n] = {k: int(re.search(rx, block).group(1)) for k, rx in FIGURES}
    return out, meta


def pick(names, pattern, path):
    found = [n for n in names if re.search(pattern, n)]
    if len(found) != 1:
        raise SystemExit(f"{pattern!r} matches {len(found)} kernels of {path}: {found}")
    return found[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("pairs", nargs="*", metavar="OLD_PATTERN[=NEW_PATTERN]")
    ap.add_argument("--all", action="store_true", help="every kernel against the kernel of the same name")
    ap.add_argument("--out")
    args = ap.parse_args()
    (old, old_meta), (new, new_meta) = kernels(args.old), kernels(args.new)
    lines, bad = [], False
    if args.all:
        names = sorted(set(old) | set(new))
        same = [n in old and n in new and old[n] == new[n] and old_meta[n] == new_meta[n] for n in names]
        lines = [f"{len(names)} kernels, {sum(same)} equal"] + [f"{'equal  ' if ok else 'DIFFERS'} {n}" for n, ok in zip(names, same)]
        bad = not all(same)
    for pair in args.pairs:
        po, _, pn = pair.partition("=")
        a, b = pick(old, po, args.old), pick(new, pn or po, args.new)
        diff = [d for d in difflib.unified_diff(old[a], new[b], lineterm="", n=0) if d[0] in "+-" and d[:3] not in ("+++", "---")]
        lines.append(f"{a}\n  -> {b}")
        lines.append(f"  lines {len(old[a])} -> {len(new[b])}, differing: {sum(d[0] == '-' for d in diff)} removed, "
                     f"{sum(d[0] == '+' for d in diff)} added")
        lines.append("  " + ", ".join(f"{k} {old_meta[a][k]} -> {new_meta[b][k]}" for k, _ in FIGURES))
        lines.extend("    " + d for d in diff)
        bad = bad or len(old[a]) != len(new[b])
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
