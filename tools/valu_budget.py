#!/usr/bin/env python3
"""Static instruction budget of k_env_windows3 per phase: cross-compiles bl_env_kernels.hip for
gfx950 to assembly (no GPU needed) and, for the FIR mode 0 / 1 / 2 instantiations of the product priority table
(BL_ENV_PRIO as the source defines it; --all-tables: every table a measurement build instantiates), counts the VALU, f64, DPP and LDS instructions between consecutive s_setprio markers, plus the kernel's VGPR count and
spills.  The compute waves' round is the stretch of segments that starts with phase 0; the setprio value of each
segment is printed beside it so that the phases can be told apart whatever the table.
usage: python tools/valu_budget.py [--src bliss_amd/csrc/bl_env_kernels.hip] [--json] [--all-tables]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


def product_table(src):
    """the value of `#define BL_ENV_PRIO` in the kernel source"""
    m = re.search(r"^#define BL_ENV_PRIO (0x[0-9A-Fa-f]+)", open(src).read(), re.M)
    if not m:
        raise SystemExit(f"no #define BL_ENV_PRIO in {src}")
    return int(m.group(1), 16)


def assemble(src):
    csrc = os.path.dirname(os.path.abspath(src))
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                        "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
                        "-Wno-unused-function", "-I" + os.path.join(csrc, "..", "..", "include"), "-I" + csrc,
                        src, "-o", out], check=True)
        return open(out).read()


def kernels(asm):
    """{mode: (instruction lines, metadata)} of k_env_windows3<mode, product table, false>"""
    out = {}
    for m in re.finditer(r"^(_Z14k_env_windows3ILi(\d)ELi(\d+)ELb0EEv[^:\s]*):", asm, re.M):
        name, mode = m.group(1), int(m.group(2))
        end = asm.index(".Lfunc_end", m.end())
        body = asm[m.end():end]
        meta = {}
        # the AMDGPU metadata lists every kernel's keys in alphabetical order: the counts follow .name
        at = re.search(r"\.name:\s+" + re.escape(name) + r"\n", asm)
        if at:
            nxt = asm.find(".name:", at.end())
            blk = asm[at.end():nxt if nxt > 0 else len(asm)]
            for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count"):
                k = re.search(r"\." + key + r":\s+(\d+)", blk)
                if k:
                    meta[key] = int(k.group(1))
        out.setdefault(mode, []).append((int(m.group(3)), body, meta))
    return out


def classify(line):
    op = line.split()[0]
    c = {"valu": 0, "f64": 0, "dpp": 0, "lds": 0}
    if op.startswith("v_"):
        c["valu"] = 1
        if "f64" in op:
            c["f64"] = 1
        if "_dpp" in op or re.search(r"\b(row_\w+|quad_perm|row_mirror|row_half_mirror)", line):
            c["dpp"] = 1
    elif op.startswith("ds_"):
        c["lds"] = 1
    return c


def segments(body):
    segs, cur = [], None
    for raw in body.splitlines():
        line = raw.split(";")[0].strip()
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        m = re.match(r"s_setprio\s+(\d+)", line)
        if m:
            if cur is not None:
                segs.append(cur)
            cur = {"prio": int(m.group(1)), "valu": 0, "f64": 0, "dpp": 0, "lds": 0, "all": 0}
            continue
        if cur is None:
            continue
        cur["all"] += 1
        for k, v in classify(line).items():
            cur[k] += v
    if cur is not None:
        segs.append(cur)
    return segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "bliss_amd", "csrc", "bl_env_kernels.hip"))
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--all-tables", action="store_true")
    a = ap.parse_args()
    want = product_table(a.src)
    ks = kernels(assemble(a.src))
    res = {}
    for mode in sorted(ks):
        for prio, body, meta in ks[mode]:
            if prio == want:
                res[f"mode{mode}"] = {"prio_table": hex(prio), **meta, "segments": segments(body)}
            elif a.all_tables:
                res[f"mode{mode}_{prio:#x}"] = {"prio_table": hex(prio), **meta, "segments": segments(body)}
    if not any(r["prio_table"] == hex(want) for r in res.values()):
        raise SystemExit(f"no k_env_windows3 instantiation with the product table {want:#x} in the assembly")
    if a.json:
        print(json.dumps(res, indent=1))
        return
    for name, r in res.items():
        print(f"{name}  table {r['prio_table']}  vgpr {r.get('vgpr_count')}  spill {r.get('vgpr_spill_count')}")
        print("   seg prio   all  valu   f64   dpp   lds")
        for i, s in enumerate(r["segments"]):
            print(f"   {i:3d} {s['prio']:4d} {s['all']:5d} {s['valu']:5d} {s['f64']:5d} {s['dpp']:5d} {s['lds']:5d}")


if __name__ == "__main__":
    sys.exit(main())
