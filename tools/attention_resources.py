#!/usr/bin/env python3
"""Resource table of every attention kernel instantiation (csrc/attention.hip, csrc/attention_bwd.hip) as markdown: registers, LDS,
occupancy and scratch as the compiler reports them (`-Rpass-analysis=kernel-resource-usage`; device code only, needs no GPU).

    python tools/attention_resources.py            # compiles the two files for gfx950 into a temporary directory"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "segdino3d_amd", "csrc")
FIELDS = ["VGPRs", "AGPRs", "ScratchSize", "VGPRs Spill", "Occupancy", "LDS Size"]


def remarks(src, tmp):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(CSRC, src), "-o", os.path.join(tmp, src + ".o")]
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


def parse(text):
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def pretty(mangled):
    """_Z16attention_kernelILi1ELi2ELb0EEv10AttnParams -> attention_kernel<1, 2, fp32> (<W, NSRC, dtype>; the dropout forward has its own
    kernel name; the backward kernels are <W, NSRC, DROP>: attn_bwd_q_kernel<1, 2, drop> regenerates the keep mask)"""
    m = re.match(r"_Z\d+([a-z_0-9]+?)(?:I((?:L[ib]\d+E)+)E)?v?\d", mangled)
    if not m:
        return mangled
    args = re.findall(r"L([ib])(\d)E", m.group(2) or "")
    words = ("plain", "drop") if m.group(1).startswith("attn_bwd") else ("fp32", "bf16")
    names = [words[int(v)] if t == "b" else v for t, v in args]
    return m.group(1) + (f"<{', '.join(names)}>" if names else "")


def main():
    texts = [open(p).read() for p in sys.argv[1:]]
    if not texts:
        with tempfile.TemporaryDirectory() as tmp:
            texts = [remarks(s, tmp) for s in ("attention.hip", "attention_bwd.hip")]
    print("| kernel | VGPR | AGPR | scratch B/lane | VGPR spill | waves/SIMD | static LDS B |")
    print("|---|---|---|---|---|---|---|")
    for text in texts:
        for name, f in parse(text).items():
            if "attention" in name or "attn" in name:
                print(f"| `{pretty(name)}` | " + " | ".join(f.get(k, "?") for k in FIELDS) + " |")


if __name__ == "__main__":
    main()
