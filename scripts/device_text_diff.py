#!/usr/bin/env python3
"""Device code of two builds, kernel by kernel: device_text_diff.py PARENT_CSRC CHANGE_CSRC > table.md (both built with the Makefile).
Per object file present in both: sha256 of the gfx950 .text. Per kernel of either build: size and sha256 of its function bytes and of its
64-byte descriptor (.kd) with bytes 16-23, the entry offset, zeroed, and the object that holds it. Exit status 1 when a kernel differs."""
import glob, hashlib, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
sha = lambda b: hashlib.sha256(b).hexdigest()[:16]

def code_object(obj, tmp):                                   # -> (.text bytes, {kernel: (function bytes, masked descriptor)})
    dst = os.path.join(tmp, os.path.basename(obj))
    subprocess.check_call(["cp", obj, dst])
    subprocess.check_output([f"{LLVM}/llvm-objdump", "--offloading", dst], cwd=tmp)
    co = glob.glob(dst + ".*gfx950")
    if not co: return None, {}
    data = open(co[0], "rb").read()
    run = lambda *a: subprocess.check_output([f"{LLVM}/llvm-readelf", *a, co[0]]).decode()
    sec = {int(m[1]): (m[2], int(m[3], 16), int(m[4], 16), int(m[5], 16)) for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+(\w+)\s+(\w+)\s+(\w+)", run("-SW"))}
    text = next((data[off:off + size] for name, _, off, size in sec.values() if name == ".text"), b"")
    body = {}
    for m in re.finditer(r"^\s*\d+:\s+(\w+)\s+(\d+)\s+(FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", run("-sW"), re.M):
        _, addr, off, _ = sec[int(m[4])]
        body[m[5]] = data[off + int(m[1], 16) - addr:][:int(m[2])]
    mask = lambda kd: kd[:16] + bytes(8) + kd[24:]
    return text, {k: (body[k], mask(body[k + ".kd"])) for k in body if k + ".kd" in body}

parent, change, where, bad = {}, {}, {}, 0
with tempfile.TemporaryDirectory() as tmp:
    print("| object | parent .text | change .text | bytes |\n|---|---|---|---|")
    for d, kernels in ((sys.argv[1], parent), (sys.argv[2], change)):
        for obj in sorted(glob.glob(os.path.join(d, "*.o"))):
            text, ks = code_object(obj, tmp)
            where.setdefault(os.path.basename(obj), {})[d] = ("no device code", "-") if text is None else (sha(text), str(len(text)))
            for k, v in ks.items(): kernels[k] = (os.path.basename(obj), *v)
    for name, t in sorted(where.items()):
        p, c = (t.get(d, ("(no such file)", "-")) for d in sys.argv[1:3])
        print(f"| {name} | {p[0]} | {c[0]} | {p[1] if p[1] == c[1] else p[1] + ' / ' + c[1]} |")
print("\n| kernel | parent object | change object | bytes | function sha256 | descriptor | same |\n|---|---|---|---|---|---|---|")
for k in sorted(set(parent) | set(change)):
    p, c = parent.get(k), change.get(k)
    if p and c and p[0] == c[0]: continue                    # stayed in its object: covered by the first table
    same = bool(p and c and p[1:] == c[1:])
    bad += not same
    print(f"| `{k}` | {p[0] if p else '-'} | {c[0] if c else '-'} | {len((p or c)[1])} | {sha((p or c)[1])} / {sha((c or p)[1])} | {'equal' if p and c and p[2] == c[2] else 'DIFFERS'} | {'yes' if same else 'NO'} |")
sys.exit(1 if bad else 0)
