"""Host-only half of the batch-size dispatch tests (tests/batch_dispatch_cases.py): the dispatch rule gives the kernel every case names,
the inputs keep the regions of a ragged last workgroup alive, and the criteria test_batch_dispatch_gpu.py applies can see a dropped
tail -- shown with the oracle alone, no GPU."""
import pytest
import torch

from chromoformer_amd import _lib
from tests import batch_dispatch_cases as bd
from tests import helpers


@pytest.mark.parametrize("name", bd.LAUNCH)
def test_dispatch_rule_gives_the_table(name):
    c, S = bd.CASES[name], bd.config(name)["i_max"]
    L = _lib.lib()
    N = c.B * S
    ag = L.cf_attc_regions(None, N)
    assert ag == c.ag == bd.regions_per_wg(N)
    assert (-(-N // ag), N % ag) == (c.wgs, c.tail)
    assert L.cf_attc_regions(None, c.B) == 1      # the Embedding launch of every case: one region per workgroup


def test_dispatch_rule_thresholds():
    """The rule at its edges with the default cap of 64 workgroups: 1 up to 64 sequences, 2 up to 128, 4 up to 256, 8 beyond."""
    L = _lib.lib()
    for N, ag in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8), (513, 8), (100000, 8)):
        assert L.cf_attc_regions(None, N) == ag == bd.regions_per_wg(N), N
    assert sorted({c.ag for c in bd.CASES.values() if not c.fused}) == [2, 4, 8]
    assert sorted({c.ag for c in bd.CASES.values() if c.tail}) == [2, 4, 8]      # a ragged last workgroup of every width


@pytest.mark.parametrize("name", sorted(bd.CASES))
def test_inputs_keep_the_tail_alive(name):
    c = bd.CASES[name]
    b = bd.batch(name)      # (asserts the table's arithmetic, a live region at every index mod AG, a live and unmasked tail)
    assert b["interaction_freq"].shape[0] == c.B
    lv = bd.live_slots(b)
    assert bool(lv.any()) and (c.B < 9 or not bool(lv.all())), "live regions, and dummy slots from 9 genes on"
    if c.tail:
        assert bool(lv[-1].all())


@pytest.mark.parametrize("name", ["R1", "R3"])
def test_criteria_reject_a_dropped_tail(name):
    """The fp32 oracle stands in for the implementation.  As it is, every criterion accepts it.  With the regions of the last workgroup
    turned into dummy slots -- what a tail guard that dropped them would compute -- the per-tensor referee criterion
    (helpers.assert_within_referee) and both per-region checks reject it.

    Measured: the dropped regions move the last gene's logits by 4.3e-3 (R1) and 6.5e-3 (R3) against a bound of 1e-4, so the
    per-tensor criterion sees them by itself.  Its gradient bounds alone see them too: every one of the tensors is off by 3.0e-4
    (R1) / 5.5e-4 (R3) of its norm or more, up to 5.5e-2 / 9.1e-2, where the fp32 oracle is within 5e-6 and the floor is 2e-5.
    Per region the dropped ones are off by 0.82 / 0.57 entry-wise in the forward rows and by their whole norm in the gradient."""
    o32, o64 = bd.referee(name, torch.float32), bd.referee(name, torch.float64)
    r32 = bd.regions(name, torch.float32)
    helpers.assert_within_referee(o32, o32, o64)
    assert bd.check_regions_forward(name, r32[0]) == 1.0 and bd.check_regions_backward(name, r32[1]) == 1.0
    cut = bd.without_tail(name)
    bad = bd.run_referee(name, torch.float32, cut)
    with pytest.raises(AssertionError, match="logits"):
        helpers.assert_within_referee(bad, o32, o64)
    # ... and with the logits and the loss of the intact run, so that the gradient bounds speak
    with pytest.raises(AssertionError, match="embed.2000.lin_proj.weight"):      # (the first tensor it looks at)
        helpers.assert_within_referee((o32[0], o32[1], bad[2]), o32, o64)
    for k, ref in o64[2].items():
        assert (bad[2][k].double() - ref).norm().item() > max(2 * (o32[2][k].double() - ref).norm().item(), 2e-5 * ref.norm().item()), k
    rows, grads = bd.run_regions(name, torch.float32, cut)
    with pytest.raises(AssertionError, match="gene, slot"):
        bd.check_regions_forward(name, rows)
    with pytest.raises(AssertionError, match="gene, slot"):
        bd.check_regions_backward(name, grads)
    # the rejections are about the tail and nothing else: every other region of the corrupted run passes as before
    c, lv = bd.CASES[name], bd.live_slots(bd.batch(name))
    for bs in rows:
        keep = lv.clone()
        keep[-1, -c.tail:] = False
        e = bd._forward_err(rows[bs], bd.regions(name, torch.float64)[0][bs], keep)
        e32 = bd._forward_err(r32[0][bs], bd.regions(name, torch.float64)[0][bs], keep)
        assert e.max().item() <= 2 * e32.max().item()
