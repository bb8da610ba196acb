"""Per-kernel ISA comparison of two builds of a library (the method of
profiles/rollout_split/kernels.txt): every clang offload bundle of each .so -> its gfx950 code
object -> llvm-objdump -d; per kernel symbol the instruction text with the address and encoding
columns stripped.  n = instructions up to and including the last s_endpgm; sha = the first 16 hex
digits of the sha256 of that text after the two allowed normalisations: the literal of an
s_add_u32 / s_addc_u32 that follows an s_getpc_b64 (the pc-relative distance to a constant table)
and the padding after the last s_endpgm.  "identical" = equal before any normalisation.  It only
hashes instruction text: it looks for no particular instruction.

usage: python tools/kernel_diff.py parent.so head.so [parent2.so head2.so ...]   (exit 0 always; read the table)"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_asm_rd  # noqa: E402


def kernels(lib):
    """{symbol: [instruction text lines]} over the gfx950 code objects of lib (kernel symbols only)."""
    out = {}
    for co in check_asm_rd.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            dis = subprocess.run([check_asm_rd.OBJDUMP, "-d", "--mcpu=gfx950", f.name], capture_output=True,
                                 text=True, check=True).stdout
            syms = subprocess.run([check_asm_rd.OBJDUMP, "-t", f.name], capture_output=True, text=True,
                                  check=True).stdout
        funcs = {ln.split()[-1] for ln in syms.splitlines() if " F " in ln and ".text" in ln}
        for fn in re.split(r"\n(?=[0-9a-f]+ <)", dis):
            m = re.match(r"[0-9a-f]+ <(.+)>:", fn)
            if not m or m.group(1) not in funcs:
                continue
            text = [ln.split("//")[0].strip() for ln in fn.split("\n")[1:]]
            name, k = m.group(1), 2
            while name in out:  # the same anonymous-namespace kernel in another translation unit
                name, k = f"{m.group(1)}#{k}", k + 1
            out[name] = [t for t in text if t and not t.endswith(":")]
    return out


def cut_padding(text):
    last = max((i for i, t in enumerate(text) if t.startswith("s_endpgm")), default=len(text) - 1)
    return text[:last + 1]


def mask_getpc(text):
    out, after = [], 0
    for t in text:
        if t.startswith("s_getpc_b64"):
            after = 4
        elif after and t.startswith(("s_add_u32", "s_addc_u32")):
            t = re.sub(r",\s*(0x[0-9a-f]+|-?\d+)\s*$", ", <pcrel>", t)
        after = max(0, after - 1)
        out.append(t)
    return out


def sha(text):
    return hashlib.sha256("\n".join(text).encode()).hexdigest()[:16]


def verdict(a, b):
    if a == b:
        return "identical"
    for name, f in (("padding", cut_padding), ("getpc offset", mask_getpc),
                    ("getpc offset + padding", lambda t: mask_getpc(cut_padding(t)))):
        if f(a) == f(b):
            return f"identical after normalisation ({name})"
    return "DIFFERS"


def compare(parent, head):
    ka, kb = kernels(parent), kernels(head)
    print(f"== {os.path.basename(head)}: parent {len(ka)} kernels, head {len(kb)} kernels")
    print(f"{'kernel':100s} {'n_par':>6s} {'n_head':>6s} {'sha_parent':16s} {'sha_head':16s} verdict")
    for name in sorted(set(ka) | set(kb)):
        a, b = ka.get(name), kb.get(name)
        na, nb = (len(cut_padding(x)) if x else "-" for x in (a, b))
        sa, sb = (sha(mask_getpc(cut_padding(x))) if x else "-" for x in (a, b))
        v = verdict(a, b) if a and b else ("ONLY-PARENT" if a else "ONLY-HEAD")
        print(f"{name:100s} {na!s:>6s} {nb!s:>6s} {sa:16s} {sb:16s} {v}")


if __name__ == "__main__":
    if len(sys.argv) < 3 or len(sys.argv) % 2 == 0:
        sys.exit(__doc__)
    for i in range(1, len(sys.argv), 2):
        compare(sys.argv[i], sys.argv[i + 1])
