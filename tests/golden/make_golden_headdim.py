"""Golden vectors for the Stage-C classifiers at head dims other than 64 (32, 96, 128): the same generators as
make_golden.py (`gen_postln`: the reference's own TransformerNoduleClassifier) and make_golden_bimodal.py (`gen`: its
own TransformerNoduleBimodalClassifier), called with new tags.  Run once where the reference is present:

    python tests/golden/make_golden_headdim.py

* ``postln_hd96``  — D 192 / 2 heads (gen_postln stores the classifier head in full, 2D x D fp32: at D 384 the fixture
  would exceed a megabyte; D 384 / 4 heads -- DINOv2-small features at the configured num_heads -- is ``bimodal_hd``'s
  CT encoder)
* ``postln_hd32``  — D 256 / 8 heads (MedSAM-width features)
* ``postln_hd128`` — D 256 / 2 heads
* ``bimodal_hd``   — D 384, CT 4 heads (dh 96), PET 3 heads (dh 128); both cross-attention layers take num_heads_ct
  (dh 96)

Provenance: the reference's own classes, imported, on CPU fp32 in eval() / no_grad (torch 2.10.0+rocm7.0, numpy 2.2.6).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from make_golden import gen_postln  # noqa: E402
from make_golden_bimodal import gen as gen_bimodal  # noqa: E402

if __name__ == "__main__":
    torch.set_num_threads(8)
    gen_postln("hd96", 192, 2, 2, 768, 2, 50, wseed=51, xseed=52, wscale=0.05)
    gen_postln("hd32", 256, 8, 2, 1024, 2, 50, wseed=53, xseed=54, wscale=0.05)
    gen_postln("hd128", 256, 2, 2, 1024, 2, 50, wseed=55, xseed=56, wscale=0.05)
    gen_bimodal("hd", 384, 4, 2, 4, 3, 2, 2, 2, batch=3, s_ct=40, s_pet=23, seed=57)
