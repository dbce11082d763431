#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 kernels?

    tools/kernel_asm_diff.py OLD NEW [--make VAR=VALUE ...] [--keep DIR] [--map OLD=NEW ...] [--margin N]

OLD and NEW are each a checkout (a directory with bliss_amd/csrc/Makefile) or anything `git archive` accepts
(a commit, a tag, HEAD).  Every bliss_amd/csrc/*.hip file with a __global__ in it is compiled device-only to
assembly with the command line its own Makefile uses for the object (so -ffp-contract=off and the rest are the
tree's, not this script's), and every function of the two sides is compared by name, wherever in the tree it was
defined:

  * the instruction text, with comments, directives and debug/section noise dropped and the local labels renumbered
    in order of appearance (their numbers depend on the position of the function in its file);
  * every .amdhsa_* field of the kernel descriptor (VGPR / AGPR / SGPR granules, LDS, scratch, ...) and the
    compiler's own report behind the kernel: TotalNumSgprs, NumVgprs, NumAgprs, ScratchSize, LDSByteSize, Occupancy.

Prints the kernels that differ or exist on one side only and exits 1 if there are any.  Needs hipcc, no GPU.

--make VAR=VALUE (repeatable) is handed to both Makefiles, so the other builds can be compared too: --make MEASURE=1
is the measurement build (every k_env_windows3 priority table, every k_pairwise root), --make XDEFS=-DBL_AMD_CHECKED_HIST
the one with the range-tested histogram adds.

--map 'OLD=NEW' (repeatable) pairs a kernel that was renamed: OLD is a regular expression that must match the whole
demangled name of a kernel of OLD without its argument list (`k_knn_cross<1, false>`), NEW the name it has in NEW, with
\\1 ... for OLD's groups: --map 'k_knn_cross<(.*)>=k_knn<\\1, true>'.  A mapped pair is not compared line by line (its
arguments differ).  Its line counts, report fields and differing descriptor fields are printed side by side, and the pair
fails when NumVgprs, NumAgprs, ScratchSize, LDSByteSize or Occupancy differ, when TotalNumSgprs rose, or when NEW has
more than --margin lines more than OLD (default 4).  --map 'OLD~NEW' is the same with the line counts only reported.
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("bliss_amd", "csrc")
REPORT = ("TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def materialise(spec, tmp, name):
    if os.path.isfile(os.path.join(spec, CSRC, "Makefile")):
        return os.path.abspath(spec)
    out = os.path.join(tmp, name)
    os.makedirs(out)
    top = subprocess.check_output(["git", "rev-parse", "--show-toplevel"], text=True).strip()
    ar = subprocess.Popen(["git", "-C", top, "archive", spec, "bliss_amd", "include"], stdout=subprocess.PIPE)
    subprocess.check_call(["tar", "-x", "-C", out], stdin=ar.stdout)
    if ar.wait() != 0:
        sys.exit(f"git archive {spec} failed")
    return out


def object_command(csrc, stem, make_vars):
    """the hipcc command line of the Makefile for <stem>.o, as a list (O=o: MEASURE=1 would rename the objects)"""
    out = subprocess.check_output(["make", "-C", csrc, "--no-print-directory", "-n", "-B", "O=o", *make_vars, stem + ".o"],
                                  text=True)
    for line in out.splitlines():
        words = shlex.split(line)
        if words and stem + ".hip" in words and "-c" in words:
            return words
    sys.exit(f"{csrc}/Makefile has no rule that compiles {stem}.hip")


def device_asm(tree, workdir, make_vars):
    """{file stem: assembly text} of the tree's kernel translation units"""
    csrc = os.path.join(tree, CSRC)
    res = {}
    for fn in sorted(os.listdir(csrc)):
        if not fn.endswith(".hip") or "__global__" not in open(os.path.join(csrc, fn)).read():
            continue
        stem = fn[:-4]
        cmd = object_command(csrc, stem, make_vars)
        o = cmd.index("-o")
        dst = os.path.join(workdir, stem + ".s")
        cmd = cmd[:o] + cmd[o + 2:]
        cmd[cmd.index("-c")] = "-S"
        subprocess.check_call(cmd + ["--cuda-device-only", "-Wno-unused-command-line-argument", "-o", dst], cwd=csrc)
        res[stem] = open(dst).read()
    return res


LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def functions(asm):
    """{symbol: {"text": [instructions], "desc": {field: value}, "report": {name: value}}}"""
    fns, cur, last, in_desc = {}, None, None, False
    for raw in asm.splitlines():
        if raw.lstrip().startswith(";"):
            m = re.match(r"\s*;\s*(\w+):\s*(\S+)", raw)
            if m and cur is None and last and m.group(1) in REPORT:
                fns[last]["report"].setdefault(m.group(1), m.group(2))
            continue
        line = re.sub(r"\s+", " ", raw.split(";", 1)[0].strip())
        m = re.match(r"\.type ([\w$.]+),@function", line)
        if m:
            cur = m.group(1)
            fns[cur] = {"text": [], "desc": {}, "report": {}}
        elif cur is None or not line or line == cur + ":":
            pass
        elif line.startswith(".amdhsa_kernel ") or line == ".end_amdhsa_kernel":
            in_desc = line != ".end_amdhsa_kernel"
        elif in_desc:
            field, _, value = line.partition(" ")
            fns[cur]["desc"][field] = value
        elif re.match(r"\.Lfunc_end\d+:", line):
            fns[cur]["text"] = renumber(fns[cur]["text"])
            last, cur = cur, None
        elif not line.startswith(".") or (line.startswith(".L") and line.endswith(":")):
            fns[cur]["text"].append(line)
    return fns


def renumber(body):
    names = {}
    for line in body:
        for lab in LABEL.findall(line):
            names.setdefault(lab, f".L{len(names)}")
    return [LABEL.sub(lambda m: names[m.group(0)], line) for line in body]


def demangle(syms):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(syms), text=True, capture_output=True, check=True).stdout
        return dict(zip(syms, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def short(nice):
    """`void k<1, false>(float4 const*, int)` -> `k<1, false>`"""
    return re.sub(r"^void ", "", nice).split("(", 1)[0].strip()


def mapped_pairs(fo, fn, nice, maps, margin):
    """prints the renamed pairs, takes them out of fo / fn, returns how many fail"""
    by_name = {short(nice[s]): s for s in fn}
    bad, used = 0, set()
    for spec in maps:
        sep = "=" if "=" in spec else "~"
        pat, _, to = spec.partition(sep)
        hits = [s for s in sorted(fo) if fo[s]["desc"] and re.fullmatch(pat, short(nice[s]))]
        if not hits:
            sys.exit(f"--map {spec}: no kernel of OLD matches")
        for so in hits:
            name = re.fullmatch(pat, short(nice[so])).expand(to)
            sn = by_name.get(name)
            if sn is None:
                sys.exit(f"--map {spec}: NEW has no kernel {name}")
            a, b = fo.pop(so), fn[sn]
            used.add(sn)
            why = [f"{k}: {a['report'].get(k)} vs {b['report'].get(k)}" for k in REPORT[1:]
                   if a["report"].get(k) != b["report"].get(k)]
            if int(b["report"]["TotalNumSgprs"]) > int(a["report"]["TotalNumSgprs"]):
                why.append("TotalNumSgprs rose")
            if sep == "=" and len(b["text"]) - len(a["text"]) > margin:
                why.append(f"more than {margin} lines longer")
            desc = [f"{k} {a['desc'].get(k)} -> {b['desc'].get(k)}" for k in sorted(set(a["desc"]) | set(b["desc"]))
                    if a["desc"].get(k) != b["desc"].get(k)]
            print(f"{'FAIL' if why else 'PAIR'} {short(nice[so])} -> {name}\n     lines {len(a['text'])} -> {len(b['text'])}"
                  + "".join(f", {k} {a['report'].get(k)} -> {b['report'].get(k)}" for k in REPORT)
                  + ("\n     " + "; ".join(desc) if desc else "") + ("\n     " + "; ".join(why) if why else ""))
            bad += bool(why)
    for sn in used:  # a NEW kernel may stand for several OLD ones, so it leaves only now
        del fn[sn]
    return bad


def compare(old, new, maps=(), margin=4):
    fo, fn = {}, {}
    for side, dst in ((old, fo), (new, fn)):
        for stem, asm in side.items():
            for sym, f in functions(asm).items():
                f["file"] = stem + ".hip"
                dst[sym] = f
    nice = demangle(sorted(set(fo) | set(fn)))
    bad = mapped_pairs(fo, fn, nice, maps, margin)
    for sym in sorted(set(fo) | set(fn)):
        a, b = fo.get(sym), fn.get(sym)
        why = []
        if a is None or b is None:
            why.append("only in " + ("NEW" if a is None else "OLD"))
        else:
            if a["text"] != b["text"]:
                first = next((i for i, (x, y) in enumerate(zip(a["text"], b["text"])) if x != y),
                             min(len(a["text"]), len(b["text"])))
                why.append(f"instructions differ ({len(a['text'])} vs {len(b['text'])} lines, first at {first}: "
                           f"{a['text'][first:first + 1]} vs {b['text'][first:first + 1]})")
            for part in ("desc", "report"):
                for k in sorted(set(a[part]) | set(b[part])):
                    if a[part].get(k) != b[part].get(k):
                        why.append(f"{k}: {a[part].get(k)} vs {b[part].get(k)}")
        if why:
            bad += 1
            print(f"DIFF {nice[sym]}\n     " + "\n     ".join(why))
    kernels = [s for s in fn if fn[s]["desc"]]
    moved = sum(1 for s in kernels if s in fo and fo[s]["file"] != fn[s]["file"])
    print(f"{len(set(fo) | set(fn))} functions compared ({len(kernels)} kernels in NEW, {moved} of them in another "
          f"file than in OLD): {bad} differ")
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--make", action="append", default=[], metavar="VAR=VALUE", dest="make_vars",
                    help="a make variable for both trees' Makefiles (repeatable), e.g. MEASURE=1")
    ap.add_argument("--keep", metavar="DIR", help="leave the assembly files here")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", dest="maps",
                    help="a renamed kernel: regex on OLD's demangled name = its name in NEW (OLD~NEW: line counts "
                         "reported, not capped); repeatable")
    ap.add_argument("--margin", type=int, default=4, help="lines a mapped kernel of NEW may be longer by (default 4)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        work = a.keep or tmp
        sides = []
        for name, spec in (("old", a.old), ("new", a.new)):
            tree = materialise(spec, tmp, name + "_tree")
            wd = os.path.join(work, name)
            os.makedirs(wd, exist_ok=True)
            sides.append((tree, wd))
        bad = compare(device_asm(*sides[0], a.make_vars), device_asm(*sides[1], a.make_vars), a.maps, a.margin)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
