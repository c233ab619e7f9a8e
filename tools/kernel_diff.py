"""Which GPU kernels differ between two builds of the library (no GPU needed: the ROCm LLVM tools only).
Extracts the gfx950 code objects of both libraries and compares, per kernel symbol, the disassembly (addresses and encodings removed;
branch targets are pc-relative, so they compare as they are; the pc-relative literal behind s_getpc_b64 that addresses a __device__
variable changes with every kernel added to or taken from the translation unit, so it is masked) and the metadata note (register, spill, LDS, scratch, kernarg and workgroup
figures).  One line per kernel that was added, lost, defined twice or changed; exit status 1 if there is any.  A refactor that moves
kernels between translation units should print nothing; a kernel change should print only the kernels it meant to touch.
usage: python tools/kernel_diff.py OLD/libstitch_gfx950.so NEW/libstitch_gfx950.so"""
import os, re, shutil, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
META = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size",
        "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def _run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def kernels(lib):
    """{kernel symbol: (instruction lines, {metadata key: value})} over all code objects of `lib`, and the symbols defined more than once"""
    out, twice = {}, set()
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(lib, os.path.join(td, "lib.so"))
        _run(os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so", cwd=td)          # writes lib.so.N.hipv4-amdgcn-... beside it
        for co in sorted(f for f in os.listdir(td) if "amdgcn" in f):
            path = os.path.join(td, co)
            meta = {}
            for m in re.finditer(r"^  - \.agpr_count.*?(?=^  - \.agpr_count|^amdhsa\.)", _run(os.path.join(LLVM, "llvm-readelf"), "--notes", path), re.S | re.M):
                kv = dict(re.findall(r"^\s+(?:- )?\.(\w+):\s+(\S+)$", m.group(0), re.M))
                meta[kv["name"]] = {k: kv.get(k) for k in META}
            text = _run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", path)
            for m in re.finditer(r"^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)", text, re.S | re.M):
                if m.group(1) not in meta:
                    continue                                                                   # (a device function that was not inlined: part of no kernel's symbol)
                ins = [l.split("//")[0].strip() for l in m.group(2).splitlines() if l.strip()]
                while ins and not ins[-1].startswith("s_endpgm"):
                    ins.pop()                                                                  # alignment padding behind the kernel's last instruction
                for i in range(1, len(ins)):                                                   # the address of a __device__ variable: pc + a literal that
                    if ins[i - 1].startswith("s_getpc_b64") and ins[i].startswith("s_add_u32"):   # says where the kernel lies in its code object, not what it does
                        ins[i] = re.sub(r"0x[0-9a-f]+$", "<pc-relative>", ins[i])
                if m.group(1) in out:
                    twice.add(m.group(1))
                out[m.group(1)] = (ins, meta[m.group(1)])
    return out, twice


def main(old, new):
    (a, a2), (b, b2) = kernels(old), kernels(new)
    lines = [f"twice in {w}: {k}" for w, t in (("old", a2), ("new", b2)) for k in sorted(t)]
    lines += [f"lost: {k}" for k in sorted(set(a) - set(b))] + [f"added: {k}" for k in sorted(set(b) - set(a))]
    for k in sorted(set(a) & set(b)):
        what = [f"{key} {a[k][1][key]} -> {b[k][1][key]}" for key in META if a[k][1][key] != b[k][1][key]]
        if a[k][0] != b[k][0]:
            first = next((i for i, (x, y) in enumerate(zip(a[k][0], b[k][0])) if x != y), min(len(a[k][0]), len(b[k][0])))
            what.append(f"code {len(a[k][0])} -> {len(b[k][0])} instructions, first difference at {first}")
        if what:
            lines.append(f"changed: {k}: " + "; ".join(what))
    print("\n".join(lines + [f"{len(a)} kernels in old, {len(b)} in new, {len(lines)} differences"]))
    return 1 if lines else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
