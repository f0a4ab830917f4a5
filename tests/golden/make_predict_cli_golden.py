"""Generate tests/golden/predict_cli.json: what `chromoformer_amd.predict` shows its users (tests/predict_cli_cases.py) -- every
action of the parser with its help text, _DEFAULTS, the rows of _NEEDS, predict()'s parameters and the arguments main() hands to
predict() for the command lines of predict_cli_cases.LINES.  Settings and names only; no device, no data, no reference.  Run on the
commit whose behaviour is to be pinned, before predict.py is edited:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_predict_cli_golden.py
"""
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from chromoformer_amd import predict  # noqa: E402
from tests import predict_cli_cases as cases  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        snap = cases.snapshot(predict, cases.write_bed(os.path.join(tmp, "c.bed")))
    path = os.path.join(HERE, "predict_cli.json")
    with open(path, "w") as f:
        json.dump(snap, f, indent=1)
        f.write("\n")
    print("wrote %s: %d actions, %d defaults, %d needs rows, %d parameters, %d calls, %.1f KB" % (
        path, len(snap["parser"]), len(snap["defaults"]), len(snap["needs"]), len(snap["signature"]), len(snap["calls"]),
        os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
