#!/usr/bin/env python3
"""Per-kernel codegen table of two builds made with `make EXTRA=-save-temps=obj`:
    python3 profiles/idioms_codegen.py <parent csrc dir> <new csrc dir> > profiles/idioms_codegen.md
For every device function of kernels / devstar / devforest / devprio: registers, spills, scratch, LDS (kernels: from the
code object's metadata), code length, out-of-line calls, and whether the instruction stream is the same once labels and
comments are gone (branch targets renumbered in order of appearance)."""
import re
import subprocess
import sys

UNITS = ["kernels", "devstar", "devforest", "devprio"]
SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"
META = ["vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size"]


def parse(path):
    funcs, meta = {}, {}
    name, body, cur, last, want = None, [], None, None, None
    for raw in open(path, errors="replace"):
        line = raw.rstrip("\n")
        m = re.match(r"^\s+\.type\s+(\S+),@function", line)
        if m:
            want = m.group(1)
            continue
        if name is None and want is not None and line.startswith(want + ":"):
            name, body, want = want, [], None
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                funcs[name] = {"body": body}
                last, name = name, None
                continue
            code = line.split(";", 1)[0].strip()
            if not code or code.endswith(":") or code.startswith("."):
                continue
            body.append(code)
            continue
        m = re.match(r"^; codeLenInByte = (\d+)", line)
        if m and last in funcs:
            funcs[last]["len"] = int(m.group(1))
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)", line)
        if m:
            if line.lstrip().startswith("- .agpr_count"):
                cur = {}
            if cur is not None:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == "name":
                    meta[m.group(2)] = cur
    for f in funcs.values():
        labels = {}
        canon = []
        for c in f["body"]:
            canon.append(re.sub(r"\.L\w+", lambda mm: labels.setdefault(mm.group(0), ".L%d" % len(labels)), c))
        f["canon"] = canon
        f["calls"] = sum(1 for c in f["body"] if c.startswith("s_swappc_b64"))
    return funcs, meta


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    short = []
    for d in out.splitlines():
        d = re.sub(r"\(.*", "", d.replace("sffk::", "").replace("void ", ""))
        short.append(d)
    return dict(zip(names, short))


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    print("# Shared wavefront idioms: codegen, parent against this tree\n")
    print("gfx950, the Makefile's flags plus `-save-temps=obj`; made by `profiles/idioms_codegen.py`.  `vgpr / sgpr / sspill /"
          " vspill / scratch / lds` are the code object's metadata (kernels only), `len` is codeLenInByte, `calls` counts"
          " out-of-line calls (`s_swappc_b64`).  A cell `a -> b` changed; a single value is the same on both builds."
          "  `stream` = the instruction stream without labels and comments.\n")
    n_same = n_changed = 0
    changed = []
    for u in UNITS:
        fo, mo = parse("%s/%s%s" % (old_dir, u, SUFFIX))
        fn, mn = parse("%s/%s%s" % (new_dir, u, SUFFIX))
        names = sorted(set(fo) | set(fn))
        dm = demangle(names)
        print("## %s\n" % u)
        print("| function | kernel | vgpr | sgpr | sspill | vspill | scratch | lds | len | calls | stream |")
        print("|---|---|---|---|---|---|---|---|---|---|---|")
        for n in names:
            a, b = fo.get(n), fn.get(n)

            def cell(x, y):
                return str(x) if x == y else "%s -> %s" % (x, y)
            ma, mb = mo.get(n, {}), mn.get(n, {})
            is_k = n in mo or n in mn
            cols = [cell(ma.get(k, "-"), mb.get(k, "-")) if is_k else "" for k in META]
            ln = cell(a["len"] if a else "absent", b["len"] if b else "absent")
            calls = cell(a["calls"] if a else "-", b["calls"] if b else "-")
            same = a is not None and b is not None and a["canon"] == b["canon"]
            if is_k:
                n_same += same
                n_changed += not same
                if not same:
                    changed.append(dm[n])
            print("| `%s` | %s | %s | %s | %s | %s |" % (dm[n], "yes" if is_k else "", " | ".join(cols), ln, calls,
                                                       "identical" if same else "changed"))
        print()
    print("Kernels with an identical stream: %d; changed: %d.\n" % (n_same, n_changed))
    if changed:
        print("Changed kernels: " + ", ".join("`%s`" % c for c in changed) + ".")


if __name__ == "__main__":
    main()
