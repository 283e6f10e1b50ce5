"""GPU: the weight slots of a handle -- vdr_weight_name(h, i) for i < vdr_num_weights(h), name by name and in order.

The sequence is observable (Engine.load_weights iterates it, callers list it to learn what a config wants) and is built in
one place, build_slots() of vdr_api.hip, from the config alone.  Each config below is the smallest one that reaches a branch
of it: a plain ViT, SwiGLU + LayerScale, the input LayerNorm of an image model (CLIP), no CLS token (SigLIP), register tokens
with and without a pos_embed (DINOv2-with-registers, DINOv3: RoPE), a post-LN token model, the SAM encoder (rel-pos tables,
neck) and a patch-embedding-only model without blocks.  Creating a handle takes no weights, so this runs in milliseconds
(it is marked gpu because vdr_create refuses to run without a device).

tests/ledger/weight_slot_names.json is a RECORD of the library at the commit its header names, never of the code under test:
    python tests/test_weight_slots_gpu.py --record tests/ledger/weight_slot_names.json --lib path/to/libvdr.so --commit <sha>
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RECORD = os.path.join(HERE, "ledger", "weight_slot_names.json")

if __name__ == "__main__":  # (--record: the paths tests/conftest.py sets up under pytest)
    for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "vit-deep-radiomics_amd"), HERE):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from handle_configs import P16, POSTLN, SAM, SWIGLU, reg_cfg, sam_config, vit_config  # noqa: E402

pytestmark = pytest.mark.gpu


def _tiny_tower(family):
    import clip_ref as cr
    return vit_config(cr.tiny_cfg(np.load(os.path.join(HERE, "golden", family + "_hf_tiny.npz"), allow_pickle=False), family))


def _registers(name):
    import dinov3_ref as dr
    return dr.vdr_config(reg_cfg(name))


def _patch_only():
    import vdr  # ARCHS["dinov2"] (the patch embedding alone: no blocks, no cls / pos / norm) shrunk
    return vdr.VdrConfig(56, 14, 3, 64, 1, 0, 256, pre_ln=False, has_cls=False, has_pos=False)


CONFIGS = {
    "p16_d128": lambda: vit_config(P16),
    "dinov2_swiglu_ls": lambda: vit_config(SWIGLU),
    "clip_hf_tiny": lambda: _tiny_tower("clip"),
    "siglip_hf_tiny": lambda: _tiny_tower("siglip"),
    "dinov2reg_hf_tiny": lambda: _registers("dinov2reg_hf_tiny"),
    "dinov3_hf_tiny": lambda: _registers("dinov3_hf_tiny"),
    "postln": lambda: vit_config(POSTLN),
    "sam": lambda: sam_config(SAM),
    "patch_only": _patch_only,
}


def _names(config):
    import vdr
    e = vdr.Engine(config)
    try:
        return e.weight_names()
    finally:
        e.close()


@pytest.fixture(scope="module")
def record():
    with open(RECORD) as f:
        return json.load(f)


def test_the_record_holds_exactly_the_configs(record):
    assert sorted(record["configs"]) == sorted(CONFIGS)
    assert len(record["recorded_at_commit"]) == 40


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_weight_names_match_the_record(record, name):
    got, want = _names(CONFIGS[name]()), record["configs"][name]
    print(f"{name}: {len(got)} slots, record {len(want)}")
    assert got == want


def _record(argv):
    import argparse
    ap = argparse.ArgumentParser(description="record the weight slot names from a build of libvdr.so")
    ap.add_argument("--record", required=True, metavar="NAMES.json")
    ap.add_argument("--lib", help="the libvdr.so to record from (default: the package's own)")
    ap.add_argument("--commit", required=True, help="the commit that library was built at (the record's header)")
    a = ap.parse_args(argv)
    from vdr import _lib as L
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)  # before the first load(): every Engine of this process uses it
    out = {name: _names(CONFIGS[name]()) for name in sorted(CONFIGS)}
    for name, names in out.items():
        print(name, len(names), flush=True)
    with open(a.record, "w") as f:
        json.dump({"recorded_at_commit": a.commit, "configs": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    _record(sys.argv[1:])
