#!/usr/bin/env python3
"""Resource table of the kernels that share csrc/depth_pixel.h (fuse_views, tsdf, track, transfer, lift_queries, lift2d) as markdown:
registers, scratch, LDS and occupancy as the compiler reports them (device code only, needs no GPU; see attention_resources.py).

    python tools/depth_pixel_resources.py                     # this tree
    python tools/depth_pixel_resources.py other/csrc this/csrc   # two trees side by side, e.g. a checkout of the parent commit"""
import subprocess
import sys
import tempfile

import attention_resources as A

FILES = ("fuse_views.hip", "tsdf.hip", "track.hip", "transfer.hip", "lift_queries.hip", "lift2d.hip")
FIELDS = ["VGPRs", "TotalSGPRs", "ScratchSize", "Occupancy", "LDS Size"]


def table(csrc):
    A.CSRC = csrc
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in FILES:
            for name, f in A.parse(A.remarks(src, tmp)).items():
                out[f"{src[:-4]}: {name}"] = [f.get(k, "?") for k in FIELDS]
    return out


def main():
    trees = [table(p) for p in (sys.argv[1:] or [A.CSRC])]
    names = subprocess.run(["c++filt", "-p"], input="\n".join(k.split(": ")[1] for k in trees[-1]), capture_output=True, text=True).stdout.split("\n")
    print("| kernel | VGPR | SGPR | scratch B/lane | waves/SIMD | static LDS B |")                # with two trees every cell is `first -> second`
    print("|---" * (len(FIELDS) + 1) + "|")
    for (key, _), name in zip(trees[-1].items(), names):
        cells = [" -> ".join(t.get(key, ["?"] * len(FIELDS))[i] for t in trees) for i in range(len(FIELDS))]
        print(f"| `{key.split(': ')[0]}: {name}` | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
