"""Nothing a user of `chromoformer_amd.predict` sees has moved: the parser, the defaults, the option -> output table of the refusals,
predict()'s parameters and what main() hands to predict() against tests/golden/predict_cli.json, which
tests/golden/make_predict_cli_golden.py recorded before the options and outputs were gathered into one table.  No device, no data."""
import inspect
import json
import os

import pytest

from tests import predict_cli_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "predict_cli.json")) as f:
        return json.load(f)


def test_parser_actions_and_help_texts(golden):
    from chromoformer_amd import predict
    rows = cases.parser_rows(predict)
    assert [r["dest"] for r in rows] == [r["dest"] for r in golden["parser"]]      # (the order of --help)
    for row, want in zip(rows, golden["parser"]):
        assert row == want, want["dest"]


def test_defaults(golden):
    from chromoformer_amd import predict
    assert cases.plain(predict._DEFAULTS) == golden["defaults"]


def test_needs_rows(golden):
    """The flags in order and the message word for word; the owners as a set (main() asks whether any of them is given)."""
    from chromoformer_amd import predict
    rows = cases.needs_rows(predict)
    assert len(rows) == len(golden["needs"]) == 25
    for row, want in zip(rows, golden["needs"]):
        assert (row["flags"], row["message"]) == (want["flags"], want["message"])
        assert sorted(row["owners"]) == sorted(want["owners"]) and len(row["owners"]) == len(want["owners"]), want["message"]


def test_an_option_applies_per_output_not_per_writer():
    """--mark-interactions-out and --mark-shapley-out share one writer call; --interaction-index applies to the former alone."""
    from chromoformer_amd import predict
    owners = {flag: set(row[1]) for row in predict._NEEDS for flag in row[0]}
    assert "mark_interactions_out" in owners["interaction_index"] and "mark_shapley_out" not in owners["interaction_index"]
    assert "contact_interactions_out" in owners["interaction_index"] and "contact_shapley_out" not in owners["interaction_index"]
    assert "mark_donor_shapley_out" in owners["mark_players"] and "mark_donor_shapley_out" not in owners["mark_scale"]


def test_predict_parameters(golden):
    """The accepted names and their defaults; the leading twelve by position, in order; an unknown name is a TypeError naming it."""
    from chromoformer_amd import predict
    rows = cases.signature_rows(predict)
    assert len(rows) == len(golden["signature"]) and dict((n, json.dumps(d)) for n, d in rows) == dict((n, json.dumps(d)) for n, d in golden["signature"])
    leading = ["meta_path", "npy_dir", "weights", "regression", "bsz", "seed", "i_max", "w_prom", "w_max", "binsizes", "progress", "store_path"]
    assert [n for n, _ in golden["signature"]][:12] == leading
    assert [n for n in inspect.signature(predict.predict).parameters][:12] == leading
    with pytest.raises(TypeError, match="no_such_out"):
        predict.predict("meta.csv", "npy", no_such_out="x.npz")


def test_main_hands_predict_the_same_arguments(golden, tmp_path):
    from chromoformer_amd import predict
    rows = cases.call_rows(predict, cases.write_bed(tmp_path / "c.bed"))
    assert [r["line"] for r in rows] == [r["line"] for r in golden["calls"]] == cases.plain(cases.LINES)
    for row, want in zip(rows, golden["calls"]):
        assert row["args"] == want["args"], want["line"]
        assert row["kwargs"] == want["kwargs"], want["line"]
    seen = {k: {json.dumps(r["kwargs"][k]) for r in golden["calls"]} for k in golden["calls"][0]["kwargs"]}
    once = [k for k, v in seen.items() if len(v) < 2 and k != "progress"]      # (progress: main() always asks for it)
    assert not once, "LINES give these no value other than the default: %s" % once
    by_line = {" ".join(r["line"]): r["kwargs"] for r in golden["calls"]}
    conv = by_line["--transplant-bed {bed} --transplant-out t.npz --transplant-freq 1,2.5 --transplant-slot 2"]
    assert conv["transplant_freq"] == [1.0, 2.5] and conv["transplant_slot"] == 2 and isinstance(conv["transplant_slot"], int)
    assert by_line["--mark-sampled-interactions-out b.npz --mark-focal 3"]["mark_focal"] == 3
    assert any(r["kwargs"]["mark_focal"] == ["mark3@pcre0", "mark0@promoter"] for r in golden["calls"])
    assert any(r["kwargs"]["fine_scan_region"] == 3 for r in golden["calls"])
