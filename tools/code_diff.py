"""Compare the compiled gfx950 code of two builds, kernel by kernel.

    python tools/code_diff.py OBJDIR_A OBJDIR_B [--source attention] [--rename PATTERN=REPL ...]

OBJDIR_*: the object directories of two builds (picotron_amd/lib/obj of each tree).  For every
kernel symbol of every object (or of --source NAME's object only) the disassembly of the unbundled
code object (llvm-objdump -d --no-show-raw-insn, addresses and encodings stripped) and the kernel's
metadata (VGPR / AGPR / SGPR counts, LDS, scratch and spill counts) are set side by side.  One line
per kernel:

    identical   the same instruction text
    reordered   the same multiset of instruction lines in another order; the moved lines follow
    different   anything else; the unified diff follows

A kernel whose parameter list changed (another mangled name) is paired with its namesake.  A kernel
whose template arguments changed needs --rename: PATTERN (a Python regular expression) is replaced by
REPL in side A's symbols before pairing, e.g. --rename '(gemm_kernelI.*)Li0E(EEv)=\\1\\2' for a
dropped last argument.  Exit 1 if
any kernel is different, missing on one side, or has other metadata.  A text comparison only: what
an instruction does is not looked at."""
import argparse
import collections
import difflib
import glob
import os
import re
import subprocess
import sys

from codeobj import LLVM, code_object, metadata

META = ("vgpr", "agpr", "sgpr", "lds", "scratch", "vspill", "sspill")


def split_name(sym):
    """(path, rest) of an Itanium-mangled nested name: `_ZN12_GLOBAL__N_117attn_delta_kernelENS_8ArgsEPKt` ->
    ("attn_delta_kernel", "ENS_8ArgsEPKt"); names of another form come back whole."""
    m = re.match(r"_ZN?", sym)
    if not m:
        return sym, ""
    i, parts = m.end(), []
    while True:
        n = re.match(r"\d+", sym[i:])
        if not n:
            break
        i += n.end()
        parts.append(sym[i:i + int(n.group())])
        i += int(n.group())
    parts = [p for p in parts if p != "_GLOBAL__N_1"]   # the anonymous namespace
    return ("::".join(parts), sym[i:]) if parts else (sym, "")


def short(sym):
    """A readable label: `attn_fwd_kernel<64,4>` when the template arguments are all integer literals."""
    path, rest = split_name(sym)
    m = re.match(r"I((?:L[ibjlm]\d+E)+)E", rest)
    return path + "<" + ",".join(re.findall(r"L[ibjlm](\d+)E", m.group(1))) + ">" if m else path


def base(sym):
    """What pairs two symbols whose parameter lists differ: the name, and the template arguments' text
    when there are any (then only a changed parameter that the name spells out unpairs them)."""
    path, rest = split_name(sym)
    return path if not rest.startswith("I") else sym


def listing(obj):
    """{kernel symbol: (instruction lines, metadata)} of one object."""
    with code_object(obj) as co:
        if co is None:
            return {}
        meta = {k["name"]: k for k in metadata(co)}
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True,
                             capture_output=True, text=True).stdout
    code, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = code.setdefault(m.group(1), []) if m.group(1) in meta else None
        elif cur is not None and line.strip() == "...":
            pass   # zero padding up to the next symbol's alignment: depends on what follows the kernel
        elif cur is not None and line.startswith("\t"):
            cur.append(re.sub(r"\s*//.*$", "", line).strip())   # the comment: address, encoding, target symbol
    return {n: (code.get(n, []), meta[n]) for n in meta}


def pair_up(a, b):
    """[(label, symbol in a or None, symbol in b or None)]: by symbol, the rest by name without parameters."""
    pairs = [(short(n), n, n) for n in a if n in b]
    rest_a, rest_b = [n for n in a if n not in b], [n for n in b if n not in a]
    for n in rest_a:
        same = [m for m in rest_b if base(m) == base(n)]
        if len(same) == 1 and sum(base(x) == base(n) for x in rest_a) == 1:
            rest_b.remove(same[0])
            pairs.append((short(n) + "  [parameters changed]", n, same[0]))
        else:
            pairs.append((n, n, None))
    return pairs + [(n, None, n) for n in rest_b]


def compare(label, ka, kb):
    """Print the kernel's line (and its detail); True if it passes."""
    if ka is None or kb is None:
        print(f"  different  {label}: only in {'B' if ka is None else 'A'}")
        return False
    (ca, ma), (cb, mb) = ka, kb
    nums = " ".join(f"{k}={ma[k]}" for k in META)
    meta_diff = [f"{k} {ma[k]} -> {mb[k]}" for k in META if ma[k] != mb[k]]
    if ca == cb:
        cls = "identical"
    elif collections.Counter(ca) == collections.Counter(cb):
        cls = "reordered"
    else:
        cls = "different"
    print(f"  {cls:10s} {label}  ({len(ca)} -> {len(cb)} instructions; {nums})")
    if meta_diff:
        print("    metadata differs: " + ", ".join(meta_diff))
    if cls != "identical":
        for line in difflib.unified_diff(ca, cb, "A", "B", n=3 if cls == "different" else 0, lineterm=""):
            print("    " + line)
    return cls != "different" and not meta_diff


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("objdir_a")
    ap.add_argument("objdir_b")
    ap.add_argument("--source", help="compare only this source's object (e.g. attention)")
    ap.add_argument("--rename", action="append", default=[], metavar="PATTERN=REPL",
                    help="re.sub applied to side A's symbols before pairing (repeatable)")
    ns = ap.parse_args(argv)
    renames = [r.split("=", 1) for r in ns.rename]
    dir_a, dir_b, source = ns.objdir_a, ns.objdir_b, ns.source
    objs = sorted({os.path.basename(p) for d in (dir_a, dir_b) for p in glob.glob(os.path.join(d, "*.o"))})
    if source:
        objs = [o for o in objs if o == source + ".o"]
    ok, count = bool(objs), collections.Counter()
    for o in objs:
        pa, pb = os.path.join(dir_a, o), os.path.join(dir_b, o)
        print(o)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"  different  only in {'A' if os.path.exists(pa) else 'B'}")
            ok = False
            continue
        a, b = listing(pa), listing(pb)
        for pat, repl in renames:
            a = {re.sub(pat, repl, n): k for n, k in a.items()}
        if not a and not b:
            print("  (no device code)")
        for label, na, nb in pair_up(a, b):
            good = compare(label, a.get(na), b.get(nb))
            ok &= good
            count["pass" if good else "FAIL"] += 1
    print(f"{count['pass']} kernel(s) pass, {count['FAIL']} fail" + ("" if objs else " (no objects found)"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
