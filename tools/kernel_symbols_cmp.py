"""Per-kernel comparison of the gfx950 code of two builds of one object file:
for every kernel whose name matches the pattern, the machine code of its
function symbol in build A against build B, and the kernel descriptor
(registers, LDS, scratch).  For changes that add kernels to a translation unit
and must leave the existing ones as they were: the object's code object then
differs as a whole (tools/kernel_dups.py prints its sha256), the kernels it
already held need not.

Code bytes are compared as they are.  A kernel that differs only in the
pc-relative literals by which it reaches the object's device globals (they move
when kernels are added) is compared again as disassembly with those literals
masked, and reported as "equal_but_for_global_offsets".
  python tools/kernel_symbols_cmp.py A/ce_abi_frames.o B/ce_abi_frames.o [regex] [--json out.json]"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"


def code_object(obj, d, tag):
    fat, co = os.path.join(d, tag + ".fat"), os.path.join(d, tag + ".co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return co


def sections(co):
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-W", co], capture_output=True, text=True, check=True).stdout
    sec = {}
    for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", out):
        sec[int(m.group(1))] = (m.group(2), int(m.group(3), 16), int(m.group(4), 16))
    return sec


def symbols(co):
    """name -> (address, size, section index) of the FUNC and OBJECT symbols"""
    out = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
    syms = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            syms[f[7]] = (int(f[1], 16), int(f[2]), int(f[6]))
    return syms


def sym_bytes(blob, sec, sym):
    addr, size, ndx = sym
    _, saddr, soff = sec[ndx]
    return blob[soff + addr - saddr: soff + addr - saddr + size]


def masked_disasm(co, name):
    """the kernel's instructions, addresses dropped and the literal of every
    s_add_u32 / s_addc_u32 that follows an s_getpc_b64 (a global's pc-relative
    offset) replaced by a mark"""
    out = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr",
                          f"--disassemble-symbols={name}", co], capture_output=True, text=True, check=True).stdout
    lines, after_getpc = [], 0
    for ln in out.splitlines():
        t = ln.split("//")[0].strip()
        if not t or t.endswith(":") or t.startswith("Disassembly") or "file format" in t or t == "...":  # (zero padding)
            continue
        if t.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc and re.match(r"s_addc?_u32 ", t):
            t = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pcrel>", t)
            after_getpc -= 1
        t = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<label>", t)  # branch targets: symbol + offset text
        lines.append(t)
    return "\n".join(lines)


def main(a_obj, b_obj, pattern, json_out):
    rx = re.compile(pattern)
    with tempfile.TemporaryDirectory() as d:
        ca, cb = code_object(a_obj, d, "a"), code_object(b_obj, d, "b")
        ba, bb = open(ca, "rb").read(), open(cb, "rb").read()
        sa, sb, seca, secb = symbols(ca), symbols(cb), sections(ca), sections(cb)
        names = sorted(n for n in sa if n + ".kd" in sa and rx.search(n))
        rows, bad = {}, 0
        for n in names:
            if n not in sb:
                rows[n] = {"state": "missing_in_b"}
                bad += 1
                continue
            xa, xb = sym_bytes(ba, seca, sa[n]), sym_bytes(bb, secb, sb[n])
            ka, kb = sym_bytes(ba, seca, sa[n + ".kd"]), sym_bytes(bb, secb, sb[n + ".kd"])
            # the descriptor's entry offset (bytes 16..23) is relative to the descriptor: it moves with the layout
            kd_equal = ka[:16] == kb[:16] and ka[24:] == kb[24:]
            if xa == xb:
                state = "byte_equal"
            elif len(xa) == len(xb) and masked_disasm(ca, n) == masked_disasm(cb, n):
                state = "equal_but_for_global_offsets"
            else:
                state = "different"
            if state == "different" or not kd_equal:
                bad += 1
            rows[n] = {"state": state, "code_bytes": len(xa), "code_sha256_a": hashlib.sha256(xa).hexdigest(),
                       "code_sha256_b": hashlib.sha256(xb).hexdigest(), "descriptor_equal": kd_equal}
        new = sorted(n for n in sb if n + ".kd" in sb and n not in sa)
        res = {"a": a_obj, "b": b_obj, "pattern": pattern, "kernels_compared": len(names), "not_equal": bad,
               "kernels_only_in_b": len(new), "kernels": rows, "only_in_b": new}
        for n, r in rows.items():
            print(f"{r['state']:30s} kd_equal={r.get('descriptor_equal')}  {n[:100]}")
        print(f"{len(names)} kernels compared, {bad} not equal, {len(new)} only in B")
        if json_out:
            with open(json_out, "w") as f:
                json.dump(res, f, indent=1)
        return 1 if bad else 0


if __name__ == "__main__":
    args = [x for x in sys.argv[1:]]
    jo = None
    if "--json" in args:
        i = args.index("--json")
        jo = args[i + 1]
        del args[i:i + 2]
    sys.exit(main(args[0], args[1], args[2] if len(args) > 2 else ".", jo))
