"""Perturbation scan of several regions per call, host side (no GPU): the C ABI declares, exports and mirrors
cf_perturbation_scan_regions; the (region, set, window) <-> row helper round-trips; the named region lists expand as documented."""
import ctypes as C
import os
import re

import pytest

from chromoformer_amd import _lib
from chromoformer_amd.attribution import scan_regions_expand, scan_row, scan_row_inverse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_symbol_struct_and_null_handle():
    hdr = open(os.path.join(ROOT, "include", "chromoformer_hip.h")).read()
    assert re.search(r"int cf_perturbation_scan_regions\(cf_handle\* h, const cf_batch\* batch, const cf_scan_regions_opts\* opts, "
                     r"float\* logits, void\* stream\);", hdr)
    assert "cf_perturbation_scan_regions" in _lib.SYMBOLS
    # unsigned regions; int width, n_sets; (pad) const unsigned*; float scale; (pad) const uint8_t*
    o = _lib.cf_scan_regions_opts
    assert C.sizeof(o) == 16 + 8 + 8 + 8 == 40
    assert [o.regions.offset, o.width.offset, o.n_sets.offset, o.mark_sets.offset, o.scale.offset, o.flip.offset] == [0, 4, 8, 16, 24, 32]
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct cf_scan_regions_opts \{(.*?)\} cf_scan_regions_opts;", hdr, re.S).group(1), flags=re.S)
    assert re.findall(r"(\w+)[;,]", body) == [n for n, _ in o._fields_]
    L = _lib.lib()      # (raises AttributeError if the library does not export the symbol)
    assert L.cf_perturbation_scan_regions(None, None, None, None, None) != 0
    assert L.cf_last_error() == b"cf_perturbation_scan_regions: null handle"


@pytest.mark.parametrize("S", [1, 8, 16])
@pytest.mark.parametrize("n_sets", [1, 2, 8])
def test_row_helper_round_trips(S, n_sets):
    W = 20
    V = 1 + n_sets * W
    seen = []
    for q in range(S + 1):
        assert scan_row(q, None, None, n_sets, W) == q * V
        assert scan_row_inverse(q * V, n_sets, W) == (q, None, None)
        seen.append(q * V)
        for k in range(n_sets):
            for g in range(W):
                row = scan_row(q, k, g, n_sets, W)
                assert row == q * V + 1 + k * W + g
                assert scan_row_inverse(row, n_sets, W) == (q, k, g)
                seen.append(row)
    assert seen == list(range((S + 1) * V))      # every row of [n_reg, V] exactly once, in order
    for row in range((S + 1) * V):
        assert scan_row(*scan_row_inverse(row, n_sets, W), n_sets, W) == row
    for k, g in ((n_sets, 0), (0, W), (-1, 0), (0, -1)):
        with pytest.raises(ValueError, match="scan_row"):
            scan_row(0, k, g, n_sets, W)


@pytest.mark.parametrize("S", [1, 8, 16])
def test_named_region_lists(S):
    assert scan_regions_expand("all", S) == list(range(S + 1))
    assert scan_regions_expand("pcres", S) == list(range(1, S + 1))
    assert scan_regions_expand("promoter", S) == [0]
    assert scan_regions_expand([S, 0, S], S) == [0, S]
    assert scan_regions_expand(iter((1,)), S) == [1]
    for bad in ("some", [], [-1], [S + 1]):
        with pytest.raises(ValueError, match="regions"):
            scan_regions_expand(bad, S)
