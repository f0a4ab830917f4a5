"""predict.main refuses an option given without the output it applies to: one row per such check, the message word for word.  Every
one of these refusals fires before predict() is called, so nothing here needs a device or a file."""
import pytest

DONOR_NEEDS_DIR = ("--mark-donor-shapley-out / --mark-donor-epistasis-out / --mark-donor-sampled-shapley-out / --window-donor-shapley-out / "
                   "--fine-window-donor-shapley-out / --mark-donor-interactions-out / --mark-donor-sampled-interactions-out / "
                   "--mark-donor-dividends-out need --donor-npy-dir")
DONOR_DIR_NEEDS = ("--donor-npy-dir / --donor-meta / --donor-store need --mark-donor-shapley-out, --mark-donor-epistasis-out or "
                   "--mark-donor-sampled-shapley-out (or --window-donor-shapley-out, --fine-window-donor-shapley-out, "
                   "--mark-donor-interactions-out, --mark-donor-sampled-interactions-out, --mark-donor-dividends-out)")
MARK_NEEDS = ("--mark-players / --mark-scale need --mark-shapley-out, --mark-epistasis-out, --mark-interactions-out or --mark-dividends-out"
              " (--mark-players also applies to --mark-donor-shapley-out / --mark-donor-epistasis-out, --mark-scale to"
              " --mark-sampled-shapley-out)")
SAMPLED_NEEDS = ("--mark-sampled-players / --mark-perms / --mark-seed need --mark-sampled-shapley-out or --mark-donor-sampled-shapley-out"
                 " (or --mark-sampled-interactions-out, --mark-donor-sampled-interactions-out)")
FINE_SCAN_NEEDS = "--fine-scan-region / --fine-scan-width / --fine-scan-stride / --fine-scan-zoom / --fine-scan-scale need --fine-scan-out"
FINE_WINDOW_NEEDS = ("--fine-window-region / --fine-window-width / --fine-window-players / --fine-window-zoom / --fine-window-perms / "
                     "--fine-window-seed need --fine-window-shapley-out or --fine-window-donor-shapley-out")
WINDOW_NEEDS = "--window-players / --window-width / --window-perms / --window-seed need --window-shapley-out or --window-donor-shapley-out"
IG_NEEDS = "--ig-steps / --ig-method / --ig-target need --ig-dir or --raw-ig-dir (or --raw-donor-ig-dir)"
INDEX_NEEDS = ("--interaction-index needs --pcre-interactions-out, --mark-interactions-out or --mark-donor-interactions-out"
               " (or --mark-sampled-interactions-out, --mark-donor-sampled-interactions-out)")

ROWS = [
    (["--raw-saliency-target", "1"], "--raw-saliency-target / --raw-saliency-times-input need --raw-saliency-dir"),
    (["--raw-saliency-times-input"], "--raw-saliency-target / --raw-saliency-times-input need --raw-saliency-dir"),
    (["--ig-steps", "10"], IG_NEEDS),
    (["--ig-method", "riemann_left"], IG_NEEDS),
    (["--ig-target", "0"], IG_NEEDS),
    (["--scan-scale", "2"], "--scan-scale / --scan-width / --scan-regions need --scan-out"),
    (["--scan-width", "2"], "--scan-scale / --scan-width / --scan-regions need --scan-out"),
    (["--scan-regions", "all"], "--scan-scale / --scan-width / --scan-regions need --scan-out"),
    (["--fine-scan-region", "3"], FINE_SCAN_NEEDS),
    (["--fine-scan-width", "2"], FINE_SCAN_NEEDS),
    (["--fine-scan-stride", "2"], FINE_SCAN_NEEDS),
    (["--fine-scan-zoom", "2"], FINE_SCAN_NEEDS),
    (["--fine-scan-scale", "2"], FINE_SCAN_NEEDS),
    (["--interaction-index", "sti"], INDEX_NEEDS),
    (["--mark-shapley-out", "x.npz", "--interaction-index", "sii"], INDEX_NEEDS),
    (["--mark-focal", "3"], "--mark-focal needs --mark-sampled-interactions-out or --mark-donor-sampled-interactions-out"),
    (["--mark-sampled-shapley-out", "x.npz", "--mark-focal", "mark0@promoter"],
     "--mark-focal needs --mark-sampled-interactions-out or --mark-donor-sampled-interactions-out"),
    (["--raw-donor-ig-dir", "d"], "--raw-donor-ig-dir needs --donor-npy-dir"),
    (["--mark-donor-shapley-out", "x.npz"], DONOR_NEEDS_DIR),
    (["--mark-donor-epistasis-out", "x.npy"], DONOR_NEEDS_DIR),
    (["--mark-donor-interactions-out", "x.npy"], DONOR_NEEDS_DIR),
    (["--mark-donor-dividends-out", "x.npz"], DONOR_NEEDS_DIR),
    (["--mark-donor-sampled-shapley-out", "x.npz"], DONOR_NEEDS_DIR),
    (["--mark-donor-sampled-interactions-out", "x.npz"], DONOR_NEEDS_DIR),
    (["--window-donor-shapley-out", "x.npz"], DONOR_NEEDS_DIR),
    (["--fine-window-donor-shapley-out", "x.npz"], DONOR_NEEDS_DIR),
    (["--donor-npy-dir", "d"], DONOR_DIR_NEEDS),
    (["--donor-meta", "m.csv"], DONOR_DIR_NEEDS),
    (["--donor-store", "s.cfstore"], DONOR_DIR_NEEDS),
    (["--mark-shapley-out", "x.npz", "--donor-npy-dir", "d"], DONOR_DIR_NEEDS),
    (["--mark-sampled-players", "marks"], SAMPLED_NEEDS),
    (["--mark-perms", "8"], SAMPLED_NEEDS),
    (["--mark-seed", "1"], SAMPLED_NEEDS),
    (["--mark-shapley-out", "x.npz", "--mark-perms", "8"], SAMPLED_NEEDS),
    (["--mark-scale", "0.5"], MARK_NEEDS),
    (["--mark-players", "regions"], MARK_NEEDS),
    (["--window-shapley-out", "x.npz", "--mark-scale", "0.5"], MARK_NEEDS),
    (["--mark-donor-shapley-out", "x.npz", "--donor-npy-dir", "d", "--mark-scale", "0.5"], MARK_NEEDS),      # (the donor rule has no scale)
    (["--mark-sampled-shapley-out", "x.npz", "--mark-players", "regions"], MARK_NEEDS),      # (the sampled game has its own players)
    (["--window-players", "regions"], WINDOW_NEEDS),
    (["--window-width", "2"], WINDOW_NEEDS),
    (["--window-perms", "8"], WINDOW_NEEDS),
    (["--window-seed", "1"], WINDOW_NEEDS),
    (["--window-scale", "0.5"], "--window-scale needs --window-shapley-out (the donor rule has no scale)"),
    (["--window-donor-shapley-out", "x.npz", "--donor-npy-dir", "d", "--window-scale", "0.5"],
     "--window-scale needs --window-shapley-out (the donor rule has no scale)"),
    (["--fine-window-region", "2"], FINE_WINDOW_NEEDS),
    (["--fine-window-width", "4"], FINE_WINDOW_NEEDS),
    (["--fine-window-players", "cells"], FINE_WINDOW_NEEDS),
    (["--fine-window-zoom", "2"], FINE_WINDOW_NEEDS),
    (["--fine-window-perms", "8"], FINE_WINDOW_NEEDS),
    (["--fine-window-seed", "1"], FINE_WINDOW_NEEDS),
    (["--fine-window-scale", "0.5"], "--fine-window-scale needs --fine-window-shapley-out (the donor rule has no scale)"),
    (["--fine-window-donor-shapley-out", "x.npz", "--donor-npy-dir", "d", "--fine-window-scale", "0.5"],
     "--fine-window-scale needs --fine-window-shapley-out (the donor rule has no scale)"),
]


@pytest.mark.parametrize("extra, message", ROWS, ids=[" ".join(a for a in extra if a.startswith("--")) for extra, _ in ROWS])
def test_an_option_without_its_output_is_refused_by_name(extra, message, capsys):
    from chromoformer_amd import predict
    with pytest.raises(SystemExit) as e:
        predict.main(["-m", "meta.csv", "-d", "npy", "-o", "out.csv"] + extra)
    assert e.value.code == 2
    assert capsys.readouterr().err.endswith("error: %s\n" % message)
