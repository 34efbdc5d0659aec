#!/usr/bin/env python3
"""dev tool (no GPU needed): one line per build job with the sha256 of the device code's .text and .rodata sections.

A host-side change must leave every line as it was.  The whole device ELF differs between two identical compiles; these two
sections do not.  The tool hashes sections, it does not look at instructions.

    python tools/device_code_digest.py > after.txt             # digests of this tree (run it on the parent tree for before.txt)
    python tools/device_code_digest.py --compare before.txt after.txt
"""
import argparse, hashlib, os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mop_amd import build as b

SECTIONS = (".text", ".rodata")


def digest(job, tmp):
    src, defs, obj = job
    elf = os.path.join(tmp, obj)
    subprocess.run([b._hipcc()] + b.FLAGS + defs + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", elf,
                                                   os.path.join(b.CSRC, src)], check=True, capture_output=True)
    objcopy = os.path.join(os.path.dirname(os.path.realpath(b._hipcc())), "..", "llvm", "bin", "llvm-objcopy")
    out = [obj]
    for sec in SECTIONS:
        raw = elf + sec
        subprocess.run([objcopy, "-O", "binary", f"--only-section={sec}", elf, raw], check=True, capture_output=True)
        data = open(raw, "rb").read() if os.path.exists(raw) else b""
        out.append(f"{sec}={hashlib.sha256(data).hexdigest()}:{len(data)}")
        if os.path.exists(raw):
            os.remove(raw)
    os.remove(elf)
    return " ".join(out)


def compare(before, after):
    rows = [{ln.split()[0]: ln.split()[1:] for ln in open(f) if ln.strip()} for f in (before, after)]
    names = sorted(set(rows[0]) | set(rows[1]))
    bad = [n for n in names if rows[0].get(n) != rows[1].get(n)]
    for n in bad:
        print("DIFFERS", n, rows[0].get(n), rows[1].get(n))
    print(f"{len(names) - len(bad)} of {len(names)} jobs match")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("BEFORE", "AFTER"))
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=args.workers) as ex:
        for line in ex.map(lambda j: digest(j, tmp), b._jobs()):
            print(line, flush=True)
