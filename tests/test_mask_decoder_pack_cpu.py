"""CPU: the host half of the mask decoder object (csrc/mask_decoder_pack.h: weight table, typed device weights, md_pack) walked by
a host program with its own main, tests/mask_decoder_pack_cases.cpp -- see its header for what it checks."""
import pytest

import host_program


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_packed_arena_publishes_every_field_once_in_disjoint_aligned_extents(tmp_path, sanitize):
    """the second build runs under the address and undefined-behaviour sanitizers (host code, stand-alone)"""
    lines = host_program.run("mask_decoder_pack_cases", tmp_path, sanitize).splitlines()
    assert lines[-1] == "cases 8 fails 0"
    # 98 fields with both optional groups, 2 fewer (pt_emb, nap) without the points', 1 fewer (mask_w) without the mask's;
    # 124 required names (6 + 2 blocks of 36 + 10 + 6 + 24 + 6), 3 of the points' group, 10 of the mask's
    for mlp_dim in (128, 2048):
        for support, fields in ((0, 95), (1, 97), (2, 96), (3, 98)):
            assert any(ln.startswith(f"mlp_dim {mlp_dim} support {support}: weights 124 + 3 + 10, fields {fields},") for ln in lines)
