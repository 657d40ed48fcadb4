#!/usr/bin/env python3
"""Per-kernel comparison of the gfx950 device code of two builds of the library: for every kernel its
instruction text (llvm-objdump -d of the code object, addresses and encodings stripped, hashed) and the
resources the code object's metadata states (VGPRs, SGPRs, scratch, static LDS, kernel-argument bytes).
Prints one JSON object: the kernels only one build has, and those whose text or resources differ.

    python tools/kernel_compare.py parent/libdragg_mi355x.so dragg_amd/libdragg_mi355x.so
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
META = {".vgpr_count": "vgprs", ".sgpr_count": "sgprs", ".private_segment_fixed_size": "scratch_bytes",
        ".group_segment_fixed_size": "lds_bytes", ".kernarg_segment_size": "kernarg_bytes"}


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(lib, tmp, tag):
    fat, co = os.path.join(tmp, tag + ".fatbin"), os.path.join(tmp, tag + ".co")
    run("objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}")
    return co


def kernels(co):
    """{kernel: {"text_sha": ..., "instructions": n, vgprs, sgprs, ...}}"""
    out, cur, pending, sym = {}, None, {}, None
    notes = run(os.path.join(LLVM, "llvm-readelf"), "--notes", co)
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        k, v = m.groups()
        if k in META:
            pending[META[k]] = int(v)
        elif k == ".symbol":                     # ('<name>.kd')
            sym = v.strip("'\"")[:-3]
        elif k == ".wavefront_size":             # (a kernel's keys are sorted: this one closes its entry)
            out[sym], pending = pending, {}
    text = {}
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            cur = m.group(1)
            text[cur] = []
        elif cur and line.strip():
            text[cur].append(re.sub(r"\s*//.*$", "", line).strip())
    for k in list(out):
        body = text.get(k, [])
        out[k].update(text_sha=hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], instructions=len(body))
    return out


def short(name):
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if m:
        n = int(m.group(1))
        return name[len(m.group(0)):][:n] + ("<...>" if len(name) > len(m.group(0)) + n + 2 else "")
    return name


def main():
    a, b = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as tmp:
        ka, kb = kernels(code_object(a, tmp, "a")), kernels(code_object(b, tmp, "b"))
    # a kernel whose parameter types changed has a new mangled name: it is the same kernel if exactly one
    # kernel of that function name is left over on either side
    left_a, left_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    resigned = {}
    for k in left_a:
        twins = [j for j in left_b if short(j) == short(k)]
        if len(twins) == 1 and [short(j) for j in left_a].count(short(k)) == 1:
            resigned[k] = twins[0]
            kb[k] = kb.pop(twins[0])
    both = sorted(set(ka) & set(kb))
    text = [k for k in both if ka[k]["text_sha"] != kb[k]["text_sha"]]
    resources = [k for k in both if any(ka[k].get(f) != kb[k].get(f) for f in META.values())]
    res = {"how": "llvm-objdump -d of the gfx950 code object of both libraries (addresses and encodings stripped, "
                  "compared per kernel) and the resources in the code object's metadata",
           "kernels_first": len(ka), "kernels_second": len(kb),
           "only_in_first": sorted(short(k) for k in set(ka) - set(kb)),
           "new_in_second": {short(k): kb[k] for k in sorted(set(kb) - set(ka))},
           "kernels_whose_signature_changed": sorted(short(k) for k in resigned),
           "kernels_whose_instruction_text_changed": [short(k) for k in text],
           "kernels_whose_resources_changed": [short(k) for k in resources],
           "changed_kernels_in_second": {short(k): kb[k] for k in sorted(set(text) | set(resources))},
           "common_kernels": {f"{short(k)}#{i}": ka[k] for i, k in enumerate(both)}}
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
