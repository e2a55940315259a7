"""Compares the gfx950 code of two builds of the library kernel by kernel: python tools/compare_kernels.py OLD.so NEW.so [name ...]
Unbundles each library's code object, disassembles it, and compares per function the instruction encodings (the hex words llvm-objdump
prints; addresses and branch-target comments are dropped).  Prints which kernels whose name contains one of the given substrings (default:
rt_render_kernel, rt_query_kernel, rt_occlusion_kernel) are identical, differ, or exist on one side only, with both sides' VGPR counts for a
kernel that differs, and the register notes of the kernels only NEW has.  A kernel template is matched across a change of its argument
block's type (the mangled name ends in it); behind the summary, every kernel that differs is tabulated, OLD -> NEW: VGPRs, SGPRs,
instructions, spilled VGPRs, scratch bytes, AGPRs, and the waves per SIMD its VGPR count allows (512 / count in granules of 8, at most 8).
Exit status 1 if any compared kernel differs or is missing."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(lib, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fat"), os.path.join(tmp, tag + ".co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, tag + ".discard")])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    return co


def encodings(co):
    """function name -> the list of its instructions' encodings (hex words after `//`)"""
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co], text=True)
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None:
            m = re.search(r"// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)", line)
            if m:
                cur.append(m.group(1).strip())
    # the s_nop padding up to the next function's alignment is listed with the function before it, and changes with what follows: not its code
    for words in out.values():
        while words and words[-1] == "BF800000":
            words.pop()
    return out


def notes(co):
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for blk in txt.split("- .agpr_count:")[1:]:
        def g(k):
            return re.search(r"\." + k + r":\s*(\S+)", blk).group(1)
        out[g("name")] = dict({k: int(g(k)) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}, agpr_count=int(blk.split()[0]))
    return out


def by_shape(table):
    """the same table with a kernel template's argument-block type dropped from its mangled name: ..EEv15rt_nearest_args -> ..EEv"""
    return {re.sub(r"Ev\d+rt_\w+_args$", "Ev", name): v for name, v in table.items()}


def waves(vgprs):
    return min(8, 512 // ((vgprs + 7) // 8 * 8)) if vgprs else 8


def main():
    old, new = sys.argv[1], sys.argv[2]
    wanted = sys.argv[3:] or ["rt_render_kernel", "rt_query_kernel", "rt_occlusion_kernel"]
    with tempfile.TemporaryDirectory() as tmp:
        co_old, co_new = code_object(old, tmp, "old"), code_object(new, tmp, "new")
        e_old, e_new = by_shape(encodings(co_old)), by_shape(encodings(co_new))
        n_old, n_new = by_shape(notes(co_old)), by_shape(notes(co_new))
    bad = 0
    differing = []
    for w in wanted:
        names = sorted(n for n in set(e_old) | set(e_new) if w in n)
        same = [n for n in names if n in e_old and n in e_new and e_old[n] == e_new[n] and e_old[n]]
        print("%s: %d kernels, %d identical (%d instructions in all)" % (w, len(names), len(same), sum(len(e_new[n]) for n in same)))
        for n in names:
            if n not in same:
                bad += 1
                differing.append(n)
                print("  DIFFERS or missing: %s (old %s, new %s instructions; old %s, new %s VGPRs)" % (
                    n, len(e_old.get(n, [])) or "-", len(e_new.get(n, [])) or "-", n_old.get(n, {}).get("vgpr_count", "-"), n_new.get(n, {}).get("vgpr_count", "-")))
    for n in sorted(set(n_new) - set(e_old)):
        print("  new: %s %s, %d instructions" % (n, n_new[n], len(e_new.get(n, []))))
    if differing:
        print("kernel (old -> new): VGPRs, SGPRs, instructions, spilled VGPRs, scratch bytes, AGPRs, waves per SIMD")
    for n in differing:
        o, w = n_old.get(n), n_new.get(n)
        if o and w:
            cols = ["%d -> %d" % (o[k], w[k]) for k in ("vgpr_count", "sgpr_count")] + ["%d -> %d" % (len(e_old[n]), len(e_new[n]))]
            cols += ["%d -> %d" % (o[k], w[k]) for k in ("vgpr_spill_count", "private_segment_fixed_size", "agpr_count")]
            print("  %s: %s, %d -> %d" % (n, ", ".join(cols), waves(o["vgpr_count"]), waves(w["vgpr_count"])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
