"""Is the device code of two versions of the HIP sources the same?  (CPU only: hipcc -S, no GPU.)

A refactor that moves kernels between files or folds repeated arithmetic into one function can be held to "the device code does
not change".  Both sides are compiled to gfx950 assembly with the build's flags and cut into functions; comments go, local labels
(.LBB3_7, .Ltmp12, .Lfunc_end3) are renumbered in their order of appearance so that they compare by position, and per function
name the instruction text and the descriptor -- the .amdhsa_ block plus the metadata's register, spill, scratch and LDS counts --
are compared as TEXT.  Prints SAME / DIFF / MISSING per kernel, exits non-zero on anything but SAME.

usage: python tools/measure/isa_same.py --a PATH [PATH ...] --b PATH [PATH ...] [--flags-a="..."] [--flags-b="..."] [--show NAME]
       PATH is a source tree (all of its salve_amd/csrc/*.hip) or one .hip file; a file's flags are the ones the __graft_entry__.py
       of its own tree gives it, unless --flags-a / --flags-b name them.  Kernels may sit in different files on the two sides.
       --show NAME also prints the diff of every differing function whose name contains NAME.  The comparison is of text only: it
       knows no instruction.
       python tools/measure/isa_same.py --flags FILE.hip      prints the build's per-file flags (tools/measure/isa_regs.sh)"""
import argparse, ast, difflib, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

BASE = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17"]   # __graft_entry__.py: build()


def build_flags(hip):
    """The flags build() adds for this file: its entry in the per-file table of the tree's __graft_entry__.py, else the table's default."""
    entry = next((p / "__graft_entry__.py" for p in Path(hip).resolve().parents if (p / "__graft_entry__.py").exists()), None)
    if entry is None:
        sys.exit(f"{hip}: no __graft_entry__.py above it, give the flags")
    table, default = {}, None
    for node in ast.walk(ast.parse(entry.read_text())):
        if isinstance(node, ast.Dict) and node.keys and all(isinstance(k, ast.Constant) and str(k.value).endswith(".hip") for k in node.keys):
            table = ast.literal_eval(node)
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "get" and len(node.args) == 2 and isinstance(node.args[1], ast.List):
            default = ast.literal_eval(node.args[1])
    if default is None:
        sys.exit(f"{entry}: no per-file flag table found")
    return table.get(Path(hip).name, default)


def functions(hip, flags, out):
    """{name: (instruction lines, descriptor lines)} of one translation unit, compiled to the file `out`."""
    subprocess.run(BASE + flags + ["-S", "--cuda-device-only", "-o", str(out), str(hip)], check=True, stderr=subprocess.DEVNULL, cwd=str(Path(hip).parent))
    text = out.read_text()
    found = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        name, body = m.group(1), m.group(2)
        desc = re.search(r"^\t\.amdhsa_kernel .*?^\t\.end_amdhsa_kernel", body, re.M | re.S)
        body = body.replace(desc.group(0), "") if desc else body
        body = re.sub(r"^\t\.section\t.*$", "", re.sub(r";.*", "", body), flags=re.M)
        labels = {}
        body = re.sub(r"\.L[A-Za-z_]+\d[\d_]*", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), body)
        meta = re.search(r"^  - (?:(?!^  - ).)*?^    \.name: +" + re.escape(name) + r"\n(?:(?!^  - ).)*", text, re.M | re.S)
        counts = re.findall(r"^    \.(?:\w+_count|\w+_fixed_size|kernarg_segment_size|max_flat_workgroup_size): .*$", meta.group(0), re.M) if meta else []
        found[name] = ([l.strip() for l in body.split("\n") if l.strip()],
                       [l.strip() for l in (desc.group(0).split("\n")[1:-1] if desc else [])] + [l.strip() for l in counts])
    return found


def side(paths, flags, tmp):
    files = [f for p in (Path(q).resolve() for q in paths) for f in (sorted((p / "salve_amd" / "csrc").glob("*.hip")) if p.is_dir() else [p])]
    with ThreadPoolExecutor(max_workers=4) as pool:
        units = list(pool.map(lambda f: functions(f, flags.split() if flags is not None else build_flags(f), Path(tmp) / f"{files.index(f)}.s"), files))
    twice = {n for i, u in enumerate(units) for n in u if any(n in v for v in units[:i])}   # same name in two anonymous namespaces: told apart by file
    return {name + (f"@{f.name}" if name in twice else ""): v + (f.name,) for f, u in zip(files, units) for name, v in u.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--flags", metavar="FILE.hip")
    ap.add_argument("--a", nargs="+"), ap.add_argument("--b", nargs="+")
    ap.add_argument("--flags-a"), ap.add_argument("--flags-b")
    ap.add_argument("--show", metavar="NAME", help="print the diff of the functions whose name contains NAME")
    args = ap.parse_args()
    if args.flags:
        print(" ".join(build_flags(args.flags)))
        return 0
    if not args.a or not args.b:
        ap.error("--a and --b are required")
    with tempfile.TemporaryDirectory() as tmp:
        (Path(tmp) / "a").mkdir(), (Path(tmp) / "b").mkdir()
        a, b = side(args.a, args.flags_a, Path(tmp) / "a"), side(args.b, args.flags_b, Path(tmp) / "b")
    names = sorted(set(a) | set(b))
    pretty = subprocess.run(["c++filt"] + [n.split("@")[0] for n in names], capture_output=True, text=True, check=True).stdout.split("\n")
    pretty = [re.sub(r"^void |\(anonymous namespace\)::|\(.*", "", q) + n[len(n.split("@")[0]):] for q, n in zip(pretty, names)]   # kernel<8, true>: without the argument list
    bad = 0
    for q, name in sorted(zip(pretty, names)):
        if name not in a or name not in b:
            status, detail = "MISSING", "not in " + ("a" if name not in a else "b")
        else:
            (ia, da, fa), (ib, db, fb) = a[name], b[name]
            status = "SAME" if ia == ib and da == db else "DIFF"
            detail = f"{len(ia):5d} lines, {len(da)} descriptor fields, {fa} -> {fb}" + ("" if ia == ib else ", instructions differ") + ("" if da == db else ", descriptor differs")
            if args.show and args.show in q and status == "DIFF":
                print("\n".join(difflib.unified_diff(ia + da, ib + db, "a", "b", lineterm="", n=2)))
        bad += status != "SAME"
        print(f"{status:8s}{q:40s}{detail}")
    print(f"{len(names)} functions, {bad} not the same")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
