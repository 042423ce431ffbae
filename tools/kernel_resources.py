#!/usr/bin/env python3
"""Resource table of the kernels of one HIP unit, from the compiler alone (needs no GPU).
usage: tools/kernel_resources.py unit.hip [-k kernel-substring] [extra hipcc flags...]
Compiles the device code with the flags of the product build (xz_amd/csrc/Makefile) + `-S
-Rpass-analysis=kernel-resource-usage` and prints one row per kernel: registers, spills, scratch (bytes per lane and
static scratch_* instructions), LDS, occupancy (waves per SIMD) and the static instruction count.  A "failed to meet
occupancy target" warning of the compiler is repeated under the table.  These are compiler reports, not times."""
import os, re, shutil, subprocess, sys, tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BASE = ["--offload-arch=" + os.environ.get("ARCH", "gfx950"), "-O2", "-std=c++17", "-fno-strict-aliasing"]
FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("SGPRs Spill", "sgpr_spill"),
          ("VGPRs Spill", "vgpr_spill"), ("ScratchSize [bytes/lane]", "scratch_B"), ("LDS Size [bytes/block]", "lds_B"),
          ("Occupancy [waves/SIMD]", "occ")]


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    try:
        if not filt:
            raise OSError("no demangler")
        out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    """`void ns::k<1u, true>(args)` -> `k<1u, true>`: no return type, no anonymous namespace, no parameter list."""
    name = re.sub(r"^void ", "", name.replace("(anonymous namespace)::", ""))
    depth = 0
    for i, ch in enumerate(name):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return name[:i]
    return name


def main():
    args = sys.argv[1:]
    if not args or args[0] in ("-h", "--help"):
        sys.exit(__doc__)
    unit, want, extra = args[0], "", []
    rest = args[1:]
    while rest:
        x = rest.pop(0)
        if x == "-k":
            want = rest.pop(0)
        else:
            extra.append(x)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "unit.s")
        cmd = [HIPCC] + BASE + extra + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", unit, "-o", asm]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            sys.stderr.write(r.stderr)
            sys.exit(r.returncode)
        text = open(asm).read()
    # the remarks: "Function Name: X" followed by its fields
    res, cur = {}, None
    for line in r.stderr.split("\n"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        body = m.group(1).strip()
        if body.startswith("Function Name:"):
            cur = res.setdefault(body.split(":", 1)[1].strip(), {})
        elif cur is not None:
            for label, key in FIELDS:
                if body.startswith(label + ":"):
                    cur[key] = body[len(label) + 1:].strip()
    warns = [l for l in r.stderr.split("\n") if "failed to meet occupancy target" in l]
    # the assembly: instructions and scratch instructions per function
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    fn = None
    for line in text.split("\n"):
        t = line.strip()
        if t.startswith(".type") and "@function" in t:
            fn = t.split()[1].split(",")[0]
            if fn in res:
                res[fn].setdefault("instr", 0); res[fn].setdefault("scratch_instr", 0)
            continue
        if t.startswith(".size") or fn not in res:
            continue
        if not t or t[0] in ".;" or t.split(";")[0].strip().endswith(":"):
            continue
        res[fn]["instr"] += 1
        if t.startswith("scratch_"):
            res[fn]["scratch_instr"] += 1
    names = [n for n in res if n in kernels]
    pretty = demangle(names)
    rows = [(short(pretty[n]), res[n]) for n in names if want in pretty[n]]
    rows.sort(key=lambda r: r[0])
    cols = ["vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_B", "scratch_instr", "lds_B", "occ", "instr"]
    print("# %s %s" % (os.path.basename(unit), " ".join(BASE + extra)))
    w = max([len(r[0]) for r in rows] + [6])
    print("%-*s %s" % (w, "kernel", " ".join("%13s" % c for c in cols)))
    for name, d in rows:
        print("%-*s %s" % (w, name, " ".join("%13s" % d.get(c, "?") for c in cols)))
    for l in warns:
        print("WARNING " + l.strip())


if __name__ == "__main__":
    main()
