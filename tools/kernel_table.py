"""Per-kernel resource table of two source trees, side by side (CPU only: compiles, runs no device code).

    python tools/kernel_table.py <parent tree> <new tree> fused_field.hip hashgrid.hip hashgrid4d.hip

Every unit is compiled to device assembly with build.py's FLAGS plus -Rpass-analysis=kernel-resource-usage.  Per kernel: VGPRs, AGPRs,
SGPRs, SGPR spills, VGPR spills, scratch bytes per lane, waves per SIMD, LDS bytes per block, the instruction count, and whether the
instruction text (comments and label numbers removed) equals the other tree's.  It counts and compares; it does not look for opcodes.
"""
import os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "selfsupervised-nvsf_amd"))
from build import FLAGS

COLS = (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r" (?:Total)?SGPRs: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)"),
        ("spill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
        ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def kernels(tree, unit):
    """{demangled name: (row of figures, normalised instruction text)} of one translation unit, in source order"""
    src = os.path.join(tree, "selfsupervised-nvsf_amd", "csrc", unit)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "unit.s")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-Rpass-analysis=kernel-resource-usage"]
        cmd += [f for f in FLAGS if f != "-shared"] + ["--cuda-device-only", "-S", src, "-o", asm]
        remarks = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        text = open(asm).read()
    rows, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
        elif cur is not None:
            for key, pat in COLS:
                m = re.search(pat, line)
                if m:
                    cur.setdefault(key, int(m.group(1)))
    body = {}
    for name in rows:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end" % re.escape(name), text, re.S | re.M)
        lines = [re.sub(r"\s+", " ", re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", ".L", l.split(";")[0])).strip() for l in m.group(1).splitlines()]
        body[name] = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")]
    # c++filt may predate the mangling of _Float16 (DF16_); only the name in front of the argument list is printed, so any built-in type does
    nice = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"] + [n.replace("DF16_", "Dh") for n in rows], capture_output=True, text=True,
                          check=True).stdout.splitlines()
    out = {}
    for name, n in zip(rows, nice):
        n = re.sub(r"\(anonymous namespace\)::", "", n)
        n = re.sub(r"^void ", "", n.split("(")[0])
        out[n] = (dict(rows[name], insts=len(body[name])), body[name])
    return out


def main(parent, new, units):
    keys = [k for k, _ in COLS] + ["insts"]
    for unit in units:
        a, b = kernels(parent, unit), kernels(new, unit)
        print(f"\n{unit}\n{'kernel':60s} " + " ".join(f"{k:>7s}" for k in keys) + "  text")
        diffs = []
        for side, tab, other in (("parent", a, b), ("new", b, a)):
            print(side)
            for n, (row, txt) in tab.items():
                same = "same" if n in other and other[n][1] == txt else ("differs" if n in other else "only here")
                print(f"{n[:60]:60s} " + " ".join(f"{row.get(k, 0):7d}" for k in keys) + f"  {same}")
                if side == "new" and n in other:
                    d = [f"{k} {other[n][0].get(k, 0)}->{row.get(k, 0)}" for k in keys if other[n][0].get(k, 0) != row.get(k, 0)]
                    if d or same != "same":
                        diffs.append(f"{n}: " + (", ".join(d) if d else "order of the instructions only"))
        print("rows that differ" if diffs else "every kernel: equal in every column and text-identical")
        print("\n".join(diffs))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3:])
