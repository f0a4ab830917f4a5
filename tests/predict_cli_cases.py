"""What `chromoformer_amd.predict` shows its users, as plain data: the parser's actions, the defaults, the option -> output table of the
refusals, predict()'s parameters and the arguments main() hands to predict() for a set of command lines.  make_predict_cli_golden.py
records these (tests/golden/predict_cli.json), test_predict_cli_cpu.py compares them with the code.  No device, no data."""
import inspect
import json

BASE = ["-m", "m.csv", "-d", "npy", "-o", "out.csv"]
BED = "{bed}"      # (stands for the BED file that snapshot() is given)
_DONOR = ["--donor-npy-dir", "dn", "--donor-meta", "dm.csv"]
LINES = [      # appended to BASE; together every option takes a value other than its default at least once
    [],
    ["-w", "w.pt", "--regression", "--store", "s.cfstore", "--attention-dir", "att", "--embeddings-out", "e.npy", "--pcre-ablation-out", "ab.npy",
     "--pcre-shapley-out", "ps.npz", "--pcre-epistasis-out", "pe.npy", "--pcre-interactions-out", "pi.npy", "--interaction-index", "sti",
     "--pcre-dividends-out", "pd.npz"],
    ["--ig-dir", "ig", "--ig-steps", "7", "--ig-method", "riemann_trapezoid", "--ig-target", "0", "--raw-ig-dir", "rig", "--raw-saliency-dir", "sal",
     "--raw-saliency-target", "1", "--raw-saliency-times-input"],
    ["--scan-out", "s.npz", "--scan-scale", "2", "--scan-width", "3", "--scan-regions", "all", "--fine-scan-out", "fs.npz", "--fine-scan-region", "3",
     "--fine-scan-width", "2", "--fine-scan-stride", "4", "--fine-scan-zoom", "2", "--fine-scan-scale", "0.5"],
    ["--mark-shapley-out", "ms.npz", "--mark-epistasis-out", "me.npy", "--mark-interactions-out", "mi.npy", "--mark-dividends-out", "md.npz",
     "--mark-players", "compartments", "--mark-scale", "0.5"],
    _DONOR + ["--donor-store", "ds.cfstore", "--mark-donor-shapley-out", "a.npz", "--mark-donor-epistasis-out", "b.npy",
              "--mark-donor-interactions-out", "c.npy", "--mark-donor-dividends-out", "d.npz", "--mark-players", "regions",
              "--mark-donor-sampled-shapley-out", "e.npz", "--mark-sampled-players", "marks", "--mark-perms", "8", "--mark-seed", "3",
              "--mark-donor-sampled-interactions-out", "f.npz", "--mark-focal", "3", "--mark-donor-backselect-out", "g.npz",
              "--mark-backselect-players", "compartments", "--backselect-mode", "forward", "--backselect-frac", "0.5",
              "--contact-donor-shapley-out", "h.npz", "--contact-players", "pcres", "--contact-donor-marks", "donor",
              "--window-donor-shapley-out", "i.npz", "--window-players", "regions", "--window-width", "4", "--window-perms", "8", "--window-seed", "2",
              "--fine-window-donor-shapley-out", "j.npz", "--fine-window-region", "2", "--fine-window-width", "4", "--fine-window-players", "cells",
              "--fine-window-zoom", "2", "--fine-window-perms", "8", "--fine-window-seed", "5"],
    _DONOR + ["--raw-donor-ig-dir", "rd"],
    ["--mark-sampled-shapley-out", "a.npz", "--mark-sampled-interactions-out", "b.npz", "--mark-focal", "mark3@pcre0,mark0@promoter",
     "--mark-backselect-out", "c.npz", "--mark-scale", "2", "--window-shapley-out", "d.npz", "--window-scale", "0.5",
     "--fine-window-shapley-out", "e.npz", "--fine-window-scale", "0.25", "--contact-shapley-out", "f.npz", "--contact-interactions-out", "g.npy",
     "--contact-dividends-out", "h.npz", "--contact-players", "pcres_and_contacts", "--contact-scale", "-1.5", "--interaction-index", "sii"],
    ["--transplant-bed", BED, "--transplant-out", "t.npz", "--transplant-freq", "1,2.5", "--transplant-slot", "2"],
    ["--mark-sampled-interactions-out", "b.npz", "--mark-focal", "3"],
]


class Called(Exception):
    """Raised in predict()'s place: nothing after main()'s call runs."""


def plain(x):
    """x as JSON holds it (tuples become lists)."""
    return json.loads(json.dumps(x))


def parser_rows(predict):
    return plain([dict(option_strings=a.option_strings, dest=a.dest, type=getattr(a.type, "__name__", a.type), default=a.default,
                       choices=None if a.choices is None else list(a.choices), required=a.required, nargs=a.nargs, const=a.const, help=a.help)
                  for a in predict.build_parser()._actions])


def needs_rows(predict):
    return plain([dict(flags=flags, owners=owners, message=message) for flags, owners, message in predict._NEEDS])


def signature_rows(predict):
    """[name, default] of everything predict() accepts: its named parameters, then the keyword arguments its table declares."""
    named = [[name, "<required>" if p.default is p.empty else p.default] for name, p in inspect.signature(predict.predict).parameters.items()
             if p.kind is not p.VAR_KEYWORD]
    return plain(named + [[name, default] for name, default in getattr(predict, "KEYWORDS", {}).items()])


def call_rows(predict, bed):
    """Per line of LINES: the positional and the keyword arguments main() hands to predict()."""
    rows = []

    def recorder(*args, **kwargs):
        raise Called(args, kwargs)

    real = predict.predict
    predict.predict = recorder
    try:
        for line in LINES:
            try:
                predict.main(BASE + [bed if word == BED else word for word in line])
            except Called as e:
                args, kwargs = e.args
                rows.append(dict(line=line, args=list(args), kwargs={k: (BED if v == bed else v) for k, v in kwargs.items()}))
            else:
                raise AssertionError("main() did not call predict() for %r" % (line,))
    finally:
        predict.predict = real
    return plain(rows)


def write_bed(path):
    with open(path, "w") as f:
        f.write("# candidates\nchr1\t100\t2000\tfirst\nchr2 5 900\n")
    return str(path)


def snapshot(predict, bed):
    return dict(parser=parser_rows(predict), defaults=plain(predict._DEFAULTS), needs=needs_rows(predict), signature=signature_rows(predict),
                calls=call_rows(predict, bed))
