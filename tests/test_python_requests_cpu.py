"""CPU: every row of tests/golden/python_requests.json (README_requests.md: recorded on the commit BEFORE vdr/engine.py and
vdr/model.py got one owner for the image path, the output buffers, the call tail, the descriptor request, the saliency and the
dense map) replays identically on the tree of the day -- the C symbol and every argument of an engine call, the
request a model method makes of its engine, what it hands the descriptor ops and what it returns, the type and the message of
every refusal and that nothing was called before it -- except for the messages whose wording the unification changed on
purpose, listed below with their new text.  The rows are computed by the generator itself (tests/golden/make_golden_requests.py,
imported from its file), so the table and its replay cannot drift apart.  No device: the engine is a stub over a fake library."""
import importlib.util
import json
import os

import pytest

# old message -> new message.  The model's own SAM refusal of a size change gave way to the engine's, which also says where the
# size of a SAM encoder is chosen.  (Nothing else is reworded: the "x must be [B, 3, H, W]" copies already agreed word for word,
# and the "needs a facet" sentences are matched by the CPU tests of their methods, so facet_args takes the sentence from its caller.)
REWORDED = {
    "set_input_size: the SAM encoder's position tables and window partition are tied to its 1024x1024 input":
        "set_input_size: the SAM encoder's position tables and window partition are tied to its 1024x1024 input; its size is "
        "chosen at load time (load_model(..., img_size=...))",
}


@pytest.fixture(scope="module")
def generator(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden_requests", os.path.join(golden_dir, "make_golden_requests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def table(golden_dir):
    with open(os.path.join(golden_dir, "python_requests.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed(generator):
    import vdr
    return json.loads(json.dumps(generator.rows(vdr)))  # (through JSON, as the table went: tuples are lists there)


def expected(row):
    if "raises" in row and row["message"] in REWORDED:
        return dict(row, message=REWORDED[row["message"]])
    return row


def test_every_recorded_row_replays(table, replayed):
    assert len(table) >= 800 and sum("raises" in r for r in table.values()) >= 250
    assert list(replayed) == list(table)  # the same cases in the same order: none dropped, none added
    seen = set()
    for key, row in table.items():
        got = replayed[key]
        # a refusal stays a refusal of the same type, an acceptance an acceptance, whatever else is compared
        assert got.get("raises") == row.get("raises"), (key, got)
        assert got == expected(row), (key, got, expected(row))
        if "raises" in row:
            # "before any device work": no forward had been asked for (an after row may refuse its second batch)
            assert row["calls"] == 0 or key.startswith("after/fit_anomaly/"), key
            seen.add(row["message"])
    assert set(REWORDED) <= seen  # (no stale entry in the list)


def test_the_table_pins_what_it_is_meant_to_pin(table):
    """spot checks of the table itself, so that a generator that records nothing cannot pass for a replay"""
    row = table["engine/vit_tiny16_224/B3/forward_descriptors"]
    assert row["symbol"] == "vdr_forward_facets" and row["args"][1] == "x" and row["args"][2:4] == [0, 3]  # own pointer, f32, B
    assert [f["hierarchy"] for f in row["args"][8]] == [0, 0, 2] and row["args"][-3:] == ["ws", 4096 + 64 * 3, 0]
    assert table["engine/tiny/forward/in_f64"]["args"][1:3] == ["other", 0]  # any other dtype: a float32 copy
    assert table["engine/tiny/forward/in_bf16"]["args"][1:3] == ["x", 1]
    assert table["engine/vit_tiny16_224/B3/forward_layers"]["args"][4][0]["ld"] == 3 * 192  # a column slice: its row stride
    assert table["engine/vit_tiny16_224/B3/forward_layers"]["owned"] == [[0]]  # the caller's buffer comes back itself
    symbols = {r["symbol"] for r in table.values() if "symbol" in r}
    assert symbols == {"vdr_forward", "vdr_forward_layers", "vdr_forward_attn_maps", "vdr_forward_facets", "vdr_forward_tokens",
                       "vdr_forward_tokens_varlen"}
    # find_correspondences: ONE forward over the 2B batch, one FacetOut and the saliency map; nn_cosine gets the two halves of
    # that one buffer as views
    row = table["after/find_correspondences/{}"]
    (req,) = row["requests"]
    assert req["x"] == [4, 3, 224, 224] and len(req["args"][0]) == 1 and len(req["kwargs"]["maps"]) == 1
    (nn,) = [h for h in row["handed"] if h["fn"] == "nn_cosine"]
    assert [a["buffer_offset"] for a in nn["args"]] == [0, 2 * 196 * 17 * 192]
    assert table["model/vit_tiny16_224/cosegment/dynamic_other_size"]["library"] == [["vdr_set_input_size", 160, 96]]
