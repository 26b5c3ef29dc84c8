#!/usr/bin/env python3
"""Golden vector for 64-channel attention heads: the REFERENCE decoder with the ScanNet200 kwargs and `num_heads=4` at
`d_model=256` (nn.MultiheadAttention(256, 4) and the per-head [content | positional] concatenation of
`instance_seg_3d_decoder.py:681-687` on 64-wide slices), on the inputs of `decoder_s96_q16`.

    python tests/golden/make_golden_heads.py          (build container only: imports /root/reference)"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402


def main():
    G.install_stand_ins()
    sys.path.insert(0, G.REFERENCE)
    import segdino3d as seg  # noqa: F401 - the reference package
    from segdino3d.models.decoder import instance_seg_3d_decoder as dec_mod
    G.golden_decoder(dec_mod, "decoder_h4_s96_q16", dict(G.DECODER_KW_SCANNET200, num_heads=4), S=96, M=7, query_subset=16)


if __name__ == "__main__":
    main()
