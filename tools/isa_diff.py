"""Do two builds of a kernel object hold the same device code? Compares the gfx950 kernels of two objects by body, not by name.

    python3 tools/isa_diff.py old/mvx_slab.o new/mvx_slab.o [old/mvx_pair.o new/mvx_pair.o ...]

Every kernel's disassembly is hashed with comments and <symbol> references stripped, and the two MULTISETS of hashes are
compared: a kernel that was renamed, or became another instantiation of a template, still matches. Prints the kernel counts
and the number of bodies without a partner per pair of objects, then the demangled names of the kernels those bodies belong
to ("-" old object, "+" new object); exit status 1 if any pair differs.
"""
import collections, hashlib, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from regs import LLVM


def kernel_bodies(obj):
    """Counter of the body hashes of the kernels (functions with a .kd descriptor) in obj's gfx950 code object, and the
    kernels' (mangled) names by hash."""
    with tempfile.TemporaryDirectory() as td:
        co, fat = os.path.join(td, "k.co"), os.path.join(td, "fat.bin")
        subprocess.check_call([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(td, "ignored")])
        subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", f"--output={co}",
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], stderr=subprocess.DEVNULL)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
        text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    kernels = set(re.findall(r"\.symbol:\s*(\S+)\.kd", notes))
    bodies, names = collections.Counter(), collections.defaultdict(list)
    for chunk in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:\n)", text):
        head, _, body = chunk.partition("\n")
        m = re.match(r"[0-9a-f]+ <([^>]+)>:$", head)
        if m and m.group(1) in kernels:
            lines = [re.sub(r"\s*<[^>]*>", "", re.sub(r"\s*//.*", "", line)).strip() for line in body.splitlines()]
            h = hashlib.sha256("\n".join(filter(None, lines)).encode()).hexdigest()
            bodies[h] += 1
            names[h].append(m.group(1))
        else:
            assert not m, (obj, m.group(1))  # (device code outside the kernels: nothing here is built that way)
    assert sum(bodies.values()) == len(kernels), (obj, sum(bodies.values()), len(kernels))
    return bodies, names


def demangle(mangled):
    """(c++filt does not know __bf16's mangling: tools/regs.py)"""
    out = subprocess.run(["c++filt"], input="\n".join(n.replace("DF16b", "Dh") for n in mangled), capture_output=True, text=True).stdout
    return [re.sub(r"^void mvx::|\(.*$", "", line) for line in out.replace("half", "__bf16").splitlines()]


if __name__ == "__main__":
    if len(sys.argv) < 3 or len(sys.argv) % 2 != 1:
        sys.exit(__doc__)
    differ = False
    for old, new in zip(sys.argv[1::2], sys.argv[2::2]):
        (a, a_names), (b, b_names) = kernel_bodies(old), kernel_bodies(new)
        unmatched = sum(((a - b) + (b - a)).values())
        differ |= unmatched != 0 or sum(a.values()) != sum(b.values())
        print(f"{os.path.basename(new):22s} kernels {sum(a.values()):4d} -> {sum(b.values()):4d}   distinct bodies {len(a):4d} -> {len(b):4d}   unmatched {unmatched}")
        for sign, left, names in (("-", a - b, a_names), ("+", b - a, b_names)):
            for name in sorted(demangle([n for h in left for n in names[h]])):  # (all kernels that share an unmatched body)
                print(f"    {sign} {name}")
    sys.exit(1 if differ else 0)
