"""Are the gfx950 kernels of two builds of an object file the same machine code?

    python tools/compare_device_code.py [--allow-new] OLD_DIR NEW_DIR [name.o ...]        (default: fgw.o fgw_small.o fgw_bapg.o fgw_grad.o)

For every object file, built with the Makefile's flags in both directories, the gfx950 code object is extracted (llvm-objdump --offloading)
and three things are compared per kernel symbol, whatever the order of the kernels in the file: the set of kernel names, each kernel's
metadata (llvm-readelf --notes: VGPRs, SGPRs, LDS, scratch, kernarg size) and each kernel's disassembly with addresses stripped.  A change
that touches host code only must leave all three identical: that is the proof that no kernel and no set of template instantiations moved.
--allow-new: a change that ADDS kernels (new instantiations, new templates) — symbols that only the new build has are counted, not reported as
differences; every symbol of the old build must still be there with the same metadata and code.  The padding behind the last instruction of a
symbol (s_nop up to the next alignment boundary, or the end of the section) belongs to the layout of the file, not to the symbol, and is dropped.
Prints one line per object file and exits 1 on any difference.  Needs no GPU."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size")


def run(*cmd, cwd=None):
    return subprocess.run(cmd, cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """Copy `obj` into `tmp`, extract its offload bundle there and return the gfx950 code object's path."""
    local = shutil.copy(obj, tmp)
    run(os.path.join(LLVM, "llvm-objdump"), "--offloading", os.path.basename(local), cwd=tmp)
    found = [f for f in os.listdir(tmp) if f.endswith("gfx950")]
    assert len(found) == 1, f"{obj}: expected one gfx950 code object, found {found}"
    return os.path.join(tmp, found[0])


def metadata(co):
    """kernel name -> {field: value} from the amdhsa.kernels note."""
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    kernels = {}
    for entry in re.split(r"^  - (?=\.)", notes.split("amdhsa.kernels:", 1)[1].split("amdhsa.target:", 1)[0], flags=re.M)[1:]:
        top = {m.group(1): m.group(2).strip("'") for m in re.finditer(r"^(?:    )?(\.\w+):\s+(\S+)$", entry, flags=re.M)}
        kernels[top[".name"]] = {f: top[f] for f in FIELDS}
    return kernels


PCREL = (re.compile(r"\ts_getpc_b64 s\[(\d+):(\d+)\]"), re.compile(r"\ts_add_u32 s(\d+), s\1, (0x[0-9a-f]+|-?\d+)\s+// ([0-9A-F]+):"),
         re.compile(r"\ts_addc_u32 s(\d+), s\1, (0x[0-9a-f]+|-?\d+)\s"))


def disassembly(co):
    """symbol -> instruction text, addresses stripped.  A call of an out-of-line device function is s_getpc_b64 + s_add_u32 + s_addc_u32 with
    the distance to the callee as a literal, which moves with the order of the kernels in the file: it is rewritten as the callee's symbol +
    offset (the callee itself is compared like every other symbol)."""
    lines = run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co).splitlines()
    heads = [(int(m.group(1), 16), m.group(2)) for m in (re.match(r"^([0-9a-f]+) <(.+)>:$", l) for l in lines) if m]
    starts = sorted(heads)

    def symbol_at(addr):
        inside = [(a, n) for a, n in starts if a <= addr]
        return f"<{inside[-1][1]}+{addr - inside[-1][0]:#x}>" if inside else None

    num = lambda t: int(t, 0) & 0xFFFFFFFF
    for k in range(len(lines) - 2):
        g, a, c = PCREL[0].match(lines[k]), PCREL[1].match(lines[k + 1]), PCREL[2].match(lines[k + 2])
        if g and a and c and (a.group(1), c.group(1)) == (g.group(1), g.group(2)):
            target = symbol_at((int(a.group(3), 16) + (num(c.group(2)) << 32 | num(a.group(2)))) & (2 ** 64 - 1))
            if target:
                lines[k + 1] = f"\ts_add_u32 s{a.group(1)}, s{a.group(1)}, lo(pc-relative {target})"
                lines[k + 2] = f"\ts_addc_u32 s{c.group(1)}, s{c.group(1)}, hi(pc-relative {target})"
    out, name = {}, None
    for line in lines:
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None:
            out[name].append(re.sub(r"// [0-9A-F]+: ", "// ", line.rstrip()))          # (every line carries its own address in a comment)
    for v in out.values():
        while v and (not v[-1].strip() or v[-1].strip() == "..." or re.match(r"^\ts_nop 0\s", v[-1])):
            v.pop()
    return {k: "\n".join(v) for k, v in out.items()}


def compare(old, new, allow_new=False):
    """List of differences between two object files (empty: identical device code), the number of kernels of the old one and of symbols only the
    new one has (counted instead of listed with allow_new)."""
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        ca, cb = code_object(old, ta), code_object(new, tb)
        ma, mb, da, db = metadata(ca), metadata(cb), disassembly(ca), disassembly(cb)
    diffs = [f"kernel only in old: {k}" for k in sorted(set(ma) - set(mb))] + [f"symbol only in old: {k}" for k in sorted(set(da) - set(db))]
    added = [f"kernel only in new: {k}" for k in sorted(set(mb) - set(ma))] + [f"symbol only in new: {k}" for k in sorted(set(db) - set(da))]
    if not allow_new:
        diffs += added
    for k in sorted(set(ma) & set(mb)):
        if ma[k] != mb[k]:
            diffs.append(f"metadata differs: {k}: {ma[k]} -> {mb[k]}")
    for k in sorted(set(da) & set(db)):
        if da[k] != db[k]:
            diffs.append(f"disassembly differs: {k}")
    missing = sorted(set(ma) - set(da))
    assert not missing, f"kernels without disassembly: {missing}"
    return diffs, len(ma), (len(set(mb) - set(ma)), len(set(db) - set(da)))


def main(argv):
    allow_new = "--allow-new" in argv
    argv = [a for a in argv if a != "--allow-new"]
    old_dir, new_dir = argv[1], argv[2]
    names = argv[3:] or ["fgw.o", "fgw_small.o", "fgw_bapg.o", "fgw_grad.o"]
    bad = 0
    for n in names:
        diffs, count, (new_k, new_s) = compare(os.path.join(old_dir, n), os.path.join(new_dir, n), allow_new)
        plus = f" (+ {new_k} new kernels, {new_s} new symbols)" if allow_new and new_s else ""
        print(f"{n}: {count} kernels, " + ("names, metadata and disassembly identical" if not diffs else f"{len(diffs)} DIFFERENCES") + plus)
        for d in diffs:
            print("   ", d)
        bad += bool(diffs)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
