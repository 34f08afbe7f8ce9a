#!/usr/bin/env python3
"""Order of issue of the planned rank-1 kernel, read from compiled code (no GPU needed).

  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -S --cuda-device-only kk_spmv.hip -o after.s
  python tools/isa_issue_order.py [--before before.s] after.s > profiles/roundN/<name>_isa.txt

For the pattern-mode instantiations <int|long, double, double, 16, 3> it lists memory instructions, waits, barriers, branches and labels from the
kernel entry to the first barrier, and says what lies between the first and the last vector load of a tile; for every instantiation of
spmv_stream3_kernel it lists the resource lines and the waves per SIMD they allow."""
import argparse
import re
import sys

KEEP = re.compile(r"^\s*(s_load|s_buffer_load|global_|buffer_|flat_|scratch_|ds_|s_waitcnt|s_barrier|s_cbranch|s_branch|s_and_saveexec|s_or_saveexec)")
LABEL = re.compile(r"^\.LBB\d+_\d+:")
RES = ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_vgpr", "next_free_sgpr")
# waves per SIMD by unified VGPR count (512 per SIMD, allocated in eights): the occupancy steps
STEPS = ((64, 8), (72, 7), (80, 6), (96, 5), (128, 4), (168, 3), (256, 2), (512, 1))


def waves(vgpr):
    for lim, w in STEPS:
        if vgpr <= lim:
            return w
    return 0


def demangle(names):
    """template arguments of _ZN2kk19spmv_stream3_kernelI<OffT><AT><YT>Li<NPT>ELi<MODE>EE..., spelled as a demangler would"""
    ty = {"i": "int", "l": "long", "d": "double", "f": "float"}
    out = []
    for n in names:
        m = re.match(r"_ZN2kk19spmv_stream3_kernelI([il])([df])([df])Li(\d+)ELi(\d+)EE", n)
        out.append("spmv_stream3_kernel<%s, %s, %s, %s, %s>" % (ty[m.group(1)], ty[m.group(2)], ty[m.group(3)], m.group(4), m.group(5)))
    return out


def kernels(path):
    """{demangled template arguments: (instruction lines, resources)} of every spmv_stream3_kernel in an assembly file"""
    text = open(path).read().split("\n")
    body, res, cur = {}, {}, None
    for ln in text:
        m = re.match(r"^(_ZN2kk19spmv_stream3_kernel\w+):", ln)
        if m:
            cur = m.group(1); body[cur] = []
            continue
        if cur and ln.startswith(".Lfunc_end"):
            cur = None
        if cur:
            s = ln.split(";")[0].rstrip()
            if s.strip() and not s.strip().startswith("."):
                body[cur].append(s.strip())
            elif LABEL.match(s.strip()):
                body[cur].append(s.strip())
        m = re.match(r"^\s*\.amdhsa_kernel (\w+)", ln)
        if m:
            rk = m.group(1); res[rk] = {}
        m = re.match(r"^\s*\.amdhsa_(\w+) (\d+)", ln)
        if m and m.group(1) in RES:
            res[rk][m.group(1)] = int(m.group(2))
    names = sorted(body)
    out = {}
    for n, d in zip(names, demangle(names)):
        out[re.search(r"<(.*)>", d).group(1)] = (body[n], res[n])
    return out


def entry_to_barrier(ins):
    rows = []
    for i, s in enumerate(ins):
        if LABEL.match(s) or KEEP.match(s):
            rows.append((i, s))
        if s.startswith("s_barrier"):
            break
    return rows


def between_loads(rows):
    """what lies between the first and the last vector load of a tile (x chunks, record, values, row bounds) in front of the first LDS write"""
    stores = [k for k, (_, s) in enumerate(rows) if s.startswith("ds_write")]
    lim = stores[0] if stores else len(rows)
    loads = [k for k, (_, s) in enumerate(rows[:lim]) if s.startswith("global_load")]
    seg = [s for _, s in rows[loads[0]:loads[-1] + 1]]
    loads_before_wait = 0
    for _, s in rows:
        if s.startswith("s_waitcnt") and "vmcnt" in s:
            break
        if s.startswith("global_load"):
            loads_before_wait += 1
    return {"ds_bpermute": sum(s.startswith("ds_bpermute") for s in seg), "vmcnt_waits": sum(s.startswith("s_waitcnt") and "vmcnt" in s for s in seg),
            "lgkmcnt_waits": sum(s.startswith("s_waitcnt") and "lgkmcnt" in s for s in seg), "vector_loads_before_first_vmcnt_wait": loads_before_wait}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before")
    ap.add_argument("after")
    a = ap.parse_args()
    sides = ([("BEFORE (parent commit)", kernels(a.before))] if a.before else []) + [("AFTER", kernels(a.after))]
    w = sys.stdout.write
    w("Rank-1 planned kernel, compiled code%s.\n" % (" before (parent commit) and after this change" if a.before else ""))
    w("hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -ffp-contract=off -S --cuda-device-only kk_spmv.hip; listed by tools/isa_issue_order.py.\n")
    w("Left column: instruction index inside the kernel.  Only memory instructions, waits, barriers, branches and labels are listed.\n")
    for inst in ("int, double, double, 16, 3", "long, double, double, 16, 3"):
        for side, ks in sides:
            ins, res = ks[inst]
            rows = entry_to_barrier(ins)
            w("\n" + "=" * 100 + "\n%s  spmv_stream3_kernel<%s>: %s\n" % (side, inst, res))
            w("between the first and the last vector load in front of the first LDS write: %s\n-- from the kernel entry to the first barrier\n" % between_loads(rows))
            for i, s in rows:
                w("%5d  %s\n" % (i, s))
    w("\n" + "=" * 100 + "\nResource lines of every spmv_stream3_kernel instantiation (waves per SIMD from the VGPR count: 512 registers per SIMD, steps at\n"
      "64 / 72 / 80 / 96 / 128 / 168 / 256)\n")
    for inst in sorted(sides[-1][1]):
        line = "<%s>" % inst
        ws = []
        for side, ks in sides:
            r = ks[inst]
            ws.append(waves(r[1]["next_free_vgpr"]))
            line += "  %s: vgpr %d sgpr %d lds %d scratch %d waves %d;" % (side.split()[0], r[1]["next_free_vgpr"], r[1]["next_free_sgpr"], r[1]["group_segment_fixed_size"],
                                                                         r[1]["private_segment_fixed_size"], ws[-1])
        if len(ws) == 2 and ws[0] != ws[1]:
            line += "  <-- occupancy step crossed, %s" % ("fewer waves" if ws[1] < ws[0] else "more waves")
        w(line + "\n")


if __name__ == "__main__":
    main()
