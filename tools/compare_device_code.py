#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of conex_amd/csrc, kernel by kernel.

    tools/compare_device_code.py OLD_CSRC_DIR NEW_CSRC_DIR [--lib-old libconex.so --lib-new libconex.so]

Both directories hold the object files of a finished `make`.  The code object of every *.o is pulled out with
`llvm-objdump --offloading`; reported are

  * kernels whose name appears in two objects of one build,
  * per object of the old build, where its kernels live in the new one (added / missing names),
  * per kernel, differences of the metadata (register counts, scratch, LDS, workgroup size, spills),
  * per kernel, whether the disassembly is the same instruction sequence.  Operands that depend on where the
    linker put a function (branch / call targets, literal offsets of pc-relative address arithmetic) are
    masked (the latter only in the scalar adds right behind an s_getpc_b64); kernels that are the same only
    after masking are listed as "same up to offsets",
  * kernels of any object but the split one (--split-object) that changed their object.

With the two libraries given, the defined dynamic symbols (`nm -D --defined-only`) are compared too.
Exit status 0 when nothing but offsets differs.
"""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
             ".max_flat_workgroup_size", ".sgpr_spill_count", ".vgpr_spill_count")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_objects(csrc, work):
    """{object name: path of its gfx950 code object}"""
    out = {}
    for obj in sorted(glob.glob(os.path.join(csrc, "*.o"))):
        name = os.path.basename(obj)
        copy = os.path.join(work, name)
        with open(obj, "rb") as f, open(copy, "wb") as g:
            g.write(f.read())
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], check=True, capture_output=True)
        found = glob.glob(copy + ".*gfx950")
        if found:
            out[name] = found[0]
    return out


def kernel_metadata(co):
    """{kernel name: {key: value}} from the AMDGPU metadata note."""
    text = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    kernels, cur = [], None
    for line in text.splitlines():
        m = re.match(r"^(  - |    )(\.\w+):\s*(.*)$", line)  # a kernel's own keys (its arguments sit deeper)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
            kernels.append(cur)
        if cur is not None and (m.group(2) in META_KEYS or m.group(2) == ".name"):
            cur[m.group(2)] = m.group(3).strip().strip("'")
    return {k[".name"]: k for k in kernels if ".name" in k}


BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+\S+")
CALL = re.compile(r"^(s_call_b64\s+\S+,)\s+\S+")
GETPC = re.compile(r"^s_getpc_b64\s+(s\[\d+:\d+\])")
PCREL = re.compile(r"^(s_add_u32|s_addc_u32|s_sub_u32|s_subb_u32)(\s+\S+,\s+\S+,)\s+\S+")
PCREL_WINDOW = 4  # s_getpc_b64 is followed by the add / addc pair that forms the address, with at most a few between


def mask(lines):
    """The instructions with what depends on function placement replaced: branch and call targets, and the literal of
    the scalar adds right behind an s_getpc_b64 (pc-relative address arithmetic).  Nothing else."""
    out, window = [], 0
    for ins in lines:
        if GETPC.match(ins):
            window = PCREL_WINDOW
        elif window and PCREL.match(ins):
            ins = PCREL.sub(r"\1\2 <pcrel>", ins)
            window -= 1
        elif window:
            window -= 1
        ins = BRANCH.sub(r"\1 <target>", ins)
        ins = CALL.sub(r"\1 <target>", ins)
        out.append(ins)
    return out


def disassembly(co):
    """{function name: (exact instructions, masked instructions)}"""
    text = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co)
    funcs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not line.strip():
            continue
        cur.append(re.sub(r"\s*//.*$", "", line).strip())  # (the comment holds the address and the encoding)
    for ins in funcs.values():  # the padding behind a code object's last function is not part of it
        while ins and ins[-1].split()[0] in ("s_code_end", "s_nop", "v_illegal", "..."):
            ins.pop()
    return {k: (v, mask(v)) for k, v in funcs.items()}


def survey(csrc, work):
    objs = code_objects(csrc, work)
    meta, dis, dup = {}, {}, []
    home = {}
    for name, co in objs.items():
        meta[name] = kernel_metadata(co)
        dis[name] = disassembly(co)
        for k in meta[name]:
            if k in home:
                dup.append((k, home[k], name))
            home[k] = name
    return meta, dis, home, dup


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--split-object", default="kkt_context.o",
                    help="the old object whose kernels may live in other objects now (default: %(default)s)")
    ap.add_argument("--lib-old")
    ap.add_argument("--lib-new")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as w0, tempfile.TemporaryDirectory() as w1:
        m0, d0, h0, dup0 = survey(a.old, w0)
        m1, d1, h1, dup1 = survey(a.new, w1)
    for tag, dup in (("old", dup0), ("new", dup1)):
        for k, x, y in dup:
            print(f"DUPLICATE ({tag}): {k} in {x} and {y}")
            bad += 1
    for obj in sorted(m0):
        names = set(m0[obj])
        homes = sorted({h1[k] for k in names if k in h1})
        print(f"{obj}: {len(names)} kernels -> {', '.join(f'{h} ({sum(1 for k in names if h1.get(k) == h)})' for h in homes)}")
    for k in sorted(set(h0) & set(h1)):  # only the split unit's kernels may change their object
        if h0[k] != h1[k] and h0[k] != a.split_object:
            print(f"MOVED: {k}: {h0[k]} -> {h1[k]}")
            bad += 1
    missing = sorted(set(h0) - set(h1))
    added = sorted(set(h1) - set(h0))
    for k in missing:
        print(f"MISSING in new: {k} (was in {h0[k]})")
    for k in added:
        print(f"ADDED in new: {k} (in {h1[k]})")
    bad += len(missing) + len(added)
    same = offsets = 0
    for k in sorted(set(h0) & set(h1)):
        a0, a1 = m0[h0[k]][k], m1[h1[k]][k]
        for key in META_KEYS:
            if a0.get(key) != a1.get(key):
                print(f"METADATA {k}: {key} {a0.get(key)} -> {a1.get(key)}")
                bad += 1
        f0, f1 = d0[h0[k]].get(k), d1[h1[k]].get(k)
        if f0 is None or f1 is None:
            print(f"NO DISASSEMBLY: {k}")
            bad += 1
        elif f0[0] == f1[0]:
            same += 1
        elif f0[1] == f1[1]:
            offsets += 1
            print(f"same up to offsets: {k}")
        else:
            n = next((i for i, (x, y) in enumerate(zip(f0[1], f1[1])) if x != y), min(len(f0[1]), len(f1[1])))
            print(f"CODE DIFFERS: {k}: {len(f0[1])} -> {len(f1[1])} instructions, first difference at {n}")
            bad += 1
    print(f"kernels: {len(h0)} old, {len(h1)} new; identical code {same}, same up to offsets {offsets}")
    if a.lib_old and a.lib_new:
        def syms(lib):
            return sorted(" ".join(l.split()[1:]) for l in run("nm", "-D", "--defined-only", lib).splitlines())
        s0, s1 = syms(a.lib_old), syms(a.lib_new)
        for s in sorted(set(s0) - set(s1)):
            print(f"SYMBOL gone: {s}")
        for s in sorted(set(s1) - set(s0)):
            print(f"SYMBOL new: {s}")
        # (hipcc gives every HIP translation unit one __hip_cuid_<hash> symbol: their number follows the number of units)
        bad += [x for x in s0 if "__hip_cuid_" not in x] != [x for x in s1 if "__hip_cuid_" not in x]
        print(f"dynamic symbols: {len(s0)} old, {len(s1)} new, {'identical' if s0 == s1 else 'DIFFERENT'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
