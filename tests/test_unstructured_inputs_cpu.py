"""The unstructured inputs themselves (tests/unstructured_inputs.py), on the CPU:

  * the fp32 oracle reproduces the reference's results on them (tests/golden/unstructured.npz, tolerances of tests/test_oracle_golden.py);
  * the generator's properties: unsymmetric masks, pairwise different resolutions, dense frequencies, every planted case present;
  * the inputs can detect what they are meant to detect: each indexing fault of ui.CORRUPTIONS moves the fp64 oracle's logits by at
    least 10 x the logit tolerance of the GPU tests -- a condition on the inputs (the seed is chosen to meet it), not on any code;
  * what the GPU tests rely on holds in the fp64 oracle exactly: garbage where the reference cannot look and other non-centre mask
    rows change neither logits nor gradients by one bit, input gradients are exactly zero in dead bins and non-zero in a fully padded
    slot whose token is visible;
  * the GPU tests' comparison functions trip when they are handed the oracle's result for a corrupted input in place of the HIP result."""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests import test_unstructured_inputs_gpu as gpu
from tests import unstructured_inputs as ui
from tests.ablation_oracle import oracle_ablation
from tests.attn_oracle import oracle_maps
from tests.helpers import GOLDEN, assert_within_referee, perturbed_params, referee_oracle
from tests.test_embed_dense_gpu import CFG2

B = 6
MOVE = 1e-3                  # 10 x the GPU tests' logit tolerance (1e-4)
FAULTS = ("mask_transposed", "resolution_0_mask_everywhere", "freq_rows_above_0_zeroed")


@pytest.fixture(scope="module", autouse=True)
def _run_time():
    t0 = time.time()
    yield
    print("\ntests/test_unstructured_inputs_cpu.py: %.1f s added to the CPU suite" % (time.time() - t0))


@functools.lru_cache(maxsize=None)
def _case():
    return ui.unstructured_batch(B), perturbed_params(False)


@functools.lru_cache(maxsize=None)
def _ref(dtype):
    batch, P = _case()
    return referee_oracle(P, batch, False, dtype)


@functools.lru_cache(maxsize=None)
def _corrupted(kind, dtype):
    batch, P = _case()
    return referee_oracle(P, ui.corrupt(batch, kind), False, dtype)


def _identical(a, b):
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and set(a[2]) == set(b[2])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_oracle_reproduces_the_reference_golden(regression):
    z = np.load(GOLDEN + "/unstructured.npz")
    head = "reg" if regression else "clf"
    batch = ui.unstructured_batch(int(z["B"]), seed=int(z["seed"]), regression=regression)
    assert int(z["seed"]) == ui.SEED
    P = orc.init_params(None, 42, regression)
    names = list(z["names"])
    assert list(P) == names
    logits, loss, grads = referee_oracle(P, batch, regression, torch.float32)
    assert abs(loss - float(z[head + ".loss"])) < 1e-6
    assert np.abs(logits.numpy() - z[head + ".logits"]).max() < 1e-6
    norms, n_full = z[head + ".grad_norms"], 0
    for i, k in enumerate(names):
        if np.isnan(norms[i]):
            assert orc.never_trained(k) and k not in grads
            continue
        assert abs(grads[k].double().norm().item() - norms[i]) <= 5e-4 * norms[i] + 1e-18, k      # (1e-3 of the sum of squares)
        assert norms[i] > 0, k
        if head + ".grad." + k in z.files:
            ref = z[head + ".grad." + k]
            assert np.abs(grads[k].numpy() - ref).max() <= 5e-4 * (np.abs(ref).max() + 1e-12), k
            n_full += 1
    assert n_full == 18 + 9 + 4      # every Regulation gamma_f, the lin_proj* weights, fc_head
    fr = batch["interaction_freq"].clone().requires_grad_(True)
    orc.forward(P, dict(batch, interaction_freq=fr))[:, 0 if regression else 1].sum().backward()
    ref = z[head + ".freq_grad"]
    assert np.abs(fr.grad.numpy() - ref).max() <= 5e-4 * np.abs(ref).max()


@pytest.mark.parametrize("name", ["default", "i_max4", "i_max16_unfused", "odd_lengths"])
def test_generator_properties(name):
    cfg = orc._cfg(gpu.CONFIGS[name])
    batch = ui.unstructured_batch(B, cfg)
    S, T = cfg["i_max"], cfg["i_max"] + 1
    g_row, g_row0, g_all = ui.planted_genes(B)
    masks = [batch["interaction_masks"][b][:, 0] for b in cfg["binsizes"]]
    for g in range(B):
        if g == g_all:      # (the one mask that cannot be unsymmetric)
            assert all(bool(m[g].all()) for m in masks)
            continue
        assert all(not torch.equal(m[g], m[g].t()) for m in masks), g
        assert all(not torch.equal(masks[r][g], masks[q][g]) for r in range(3) for q in range(r)), g
        assert all(not bool(m[g, 0, 0]) for m in masks) or g == g_row0
    for m in masks:
        assert bool(m[g_row, ui.ROW].all()) and not bool(m[g_row, 0, ui.ROW])            # a fully masked row that row 0 attends to
        assert bool(m[g_row0, 0].all()) and not bool(m[g_row0, 1:].all())
        assert 0.3 < m[:g_row].float().mean().item() < 0.5
    fr = batch["interaction_freq"]
    assert fr.shape == (B, T, T) and bool((fr != 0).all()) and bool((fr < 0).any()) and 1.2 < fr.std().item() < 1.8
    assert bool((fr[:, 1:].abs().sum(-1) > 0).all())
    for b in cfg["binsizes"]:
        L = cfg["w_max"] // b
        pm, cm = batch["promoter_pad_masks"][b], batch["pcre_pad_masks"][b]
        assert pm.shape == (B, 1, 1, L, L) and cm.shape == (B, S, 1, L, L) and pm.dtype == cm.dtype == torch.bool
        seen = set()
        for g in range(B):
            for s in range(S):
                kind, row = ui.pcre_pattern(g, s, S), ~cm[g, s, 0, L // 2]
                seen.add(kind)
                want = {"first": [0], "last": [L - 1], "centre_only": [L // 2], "none_valid": [],
                        "centre_masked": [i for i in range(L) if i != L // 2]}.get(kind)
                if want is None:
                    v = row.nonzero().view(-1)
                    assert len(v) >= 2 and not bool(row[v[0]:v[-1]].all())      # holes inside the valid range
                else:
                    assert row.nonzero().view(-1).tolist() == want, (g, s, kind)
        assert seen == set(ui.PCRE_PATTERNS)
        rows = [~pm[g, 0, 0, L // 2] for g in range(B)]
        assert int(rows[0].sum()) == 0 and int(rows[2].sum()) == 1 and not bool(rows[3][L // 2]) and int(rows[3].sum()) == L - 1 and bool(rows[4].all())
        assert 1 < int(rows[1].sum()) < L
        # non-centre rows are their own bits; features are drawn everywhere
        assert not torch.equal(cm[:, :, 0, 0], cm[:, :, 0, L // 2]) and not torch.equal(pm[:, :, 0, 0], pm[:, :, 0, L // 2])
        assert bool((batch["pcre_feats"][b] != 0).all()) and bool((batch["promoter_feats"][b] != 0).all())
        rep = ui.unstructured_batch(B, cfg, rows="repeat")
        assert torch.equal(rep["pcre_pad_masks"][b], cm[:, :, :, L // 2:L // 2 + 1].expand_as(cm))
        assert torch.equal(ui.centre_rows(batch)["pcre_pad_masks"][b], cm[:, :, 0, L // 2])
    again, other = ui.unstructured_batch(B, cfg), ui.unstructured_batch(B, cfg, rows_seed=1)
    for k in gpu.ARGS:
        for b in (cfg["binsizes"] if isinstance(batch[k], dict) else [None]):
            x, y, o = (t[k] if b is None else t[k][b] for t in (batch, again, other))
            assert torch.equal(x, y), k                                                   # deterministic from the seed
            assert torch.equal(x, o) != k.endswith("pad_masks"), k                         # rows_seed moves the pad masks alone ...
    for key in ("promoter_pad_masks", "pcre_pad_masks"):
        assert all(torch.equal(ui.centre_rows(batch)[key][b], ui.centre_rows(other)[key][b]) for b in cfg["binsizes"])      # ... off the centre row
    # garbage goes only where the reference cannot look, and somewhere
    dirty = ui.with_garbage(batch)
    pd, cd = ui.dead_bins(batch)
    for b in cfg["binsizes"]:
        L = cfg["w_max"] // b
        assert bool(cd[b].any()) and bool(pd[b].any()) and not bool(pd[b][..., L // 2].any())
        assert bool((dirty["pcre_feats"][b][cd[b]] == ui.GARBAGE_FEAT).all()) and torch.equal(dirty["pcre_feats"][b][~cd[b]], batch["pcre_feats"][b][~cd[b]])
        assert not bool((cd[b] & ~batch["pcre_pad_masks"][b][:, :, 0, L // 2]).any())
    dead = ui.masked_everywhere(batch)
    assert bool(dead.any()) and bool((dirty["interaction_freq"][dead] == ui.GARBAGE_FREQ).all())
    assert torch.equal(dirty["interaction_freq"][~dead], fr[~dead])


@pytest.mark.parametrize("kind", ui.CORRUPTIONS)
def test_the_inputs_detect_each_indexing_fault(kind):
    moved = (_corrupted(kind, torch.float64)[0] - _ref(torch.float64)[0]).abs().max().item()
    print("%s moves the fp64 oracle's logits by %.3e" % (kind, moved))
    assert moved >= MOVE, (kind, moved)


def test_garbage_and_non_centre_rows_change_no_bit_of_the_fp64_oracle():
    batch, P = _case()
    ref = _ref(torch.float64)
    _identical(referee_oracle(P, ui.with_garbage(batch), False, torch.float64), ref)
    _identical(referee_oracle(P, ui.unstructured_batch(B, rows_seed=1), False, torch.float64), ref)
    _identical(referee_oracle(P, ui.unstructured_batch(B, rows="repeat"), False, torch.float64), ref)
    assert all(float(g.norm()) > 0 for g in ref[2].values()) and len(ref[2]) == 334


def test_with_all_embedding_rows_read_the_dead_bins_are_still_dead():
    """embed.n_layers = 2: the oracle reads every row of the 5-d promoter mask -- other non-centre rows DO move it, and the garbage
    of with_garbage(all_promoter_rows=True) does not."""
    cfg = orc._cfg(CFG2)
    batch, P = ui.unstructured_batch(B, cfg), perturbed_params(False, cfg)
    pd, _ = ui.dead_bins(batch, True)
    assert all(bool(m.any()) for m in pd.values())
    ref = referee_oracle(P, batch, False, torch.float64, cfg)
    _identical(referee_oracle(P, ui.with_garbage(batch, True), False, torch.float64, cfg), ref)
    other = referee_oracle(P, ui.unstructured_batch(B, cfg, rows_seed=1), False, torch.float64, cfg)
    assert (other[0] - ref[0]).abs().max().item() > 1e-4


def test_fp32_oracle_against_the_fp64_oracle():
    o32, o64 = _ref(torch.float32), _ref(torch.float64)
    e = (o32[0].double() - o64[0]).abs().max().item()
    worst = max(((o32[2][k].double() - g).norm().item() / g.norm().item(), k) for k, g in o64[2].items())
    print("fp32 oracle against the fp64 oracle: logits %.2e, worst gradient tensor %.2e relative Frobenius (%s)" % (e, worst[0], worst[1]))
    assert e < 1e-5 and worst[0] < 1e-4
    assert_within_referee(o32, o32, o64)      # the referee's criterion accepts the fp32 oracle itself


def test_input_gradients_of_the_oracle_have_the_structure_the_gpu_test_asserts():
    batch, P = _case()
    g32, g64 = (gpu.oracle_input_grads(P, batch, None, 1, dt) for dt in (torch.float32, torch.float64))
    gpu.check_input_grads(g32, g32, g64)
    gpu.check_input_grad_structure(g32, g32, g64, batch, ui.dead_bins(batch))
    slots = gpu._visible_padded_slots(batch, g64)
    print("fully padded pCRE slots the oracle's gradient reaches:", slots)
    dirty = gpu.oracle_input_grads(P, ui.with_garbage(batch), None, 1, torch.float64)
    assert all(torch.equal(dirty[k], g64[k]) for k in g64)


# ----------------------------------------------------------------------------- the GPU tests' comparisons can fail
@pytest.mark.parametrize("kind", FAULTS)
def test_the_referee_rejects_the_result_of_a_faulty_kernel(kind):
    """In place of the HIP result: the fp32 oracle on the corrupted input, i.e. a kernel that is exact except for that fault."""
    with pytest.raises(AssertionError):
        assert_within_referee(_corrupted(kind, torch.float32), _ref(torch.float32), _ref(torch.float64))


@pytest.mark.parametrize("kind", FAULTS)
def test_the_input_gradient_map_and_deletion_checks_reject_it_too(kind):
    batch, P = _case()
    bad = ui.corrupt(batch, kind)
    g32, g64 = (gpu.oracle_input_grads(P, batch, None, 1, dt) for dt in (torch.float32, torch.float64))
    with pytest.raises(AssertionError):
        gpu.check_input_grads(gpu.oracle_input_grads(P, bad, None, 1, torch.float32), g32, g64)
    _, ref = oracle_maps(P, batch)
    gpu.compare_maps(ref, ref)
    gpu.check_map_structure(ref, batch, orc._cfg(None))
    with pytest.raises(AssertionError):
        gpu.compare_maps(oracle_maps(P, bad)[1], ref)
    assert (oracle_ablation(P, bad) - oracle_ablation(P, batch)).abs().max().item() >= 10 * gpu.ABLATION_TOL


def test_the_exact_checks_reject_a_leak():
    """A kernel that lets one masked key through with weight 1e-6, or gives a fully masked row almost uniform weights."""
    batch, P = _case()
    cfg = orc._cfg(None)
    _, ref = oracle_maps(P, batch)
    k = "regulation.2000"
    leak = {n: t.clone() for n, t in ref.items()}
    mask = batch["interaction_masks"][2000][:, 0, 0]
    g = next(g for g in range(B) if bool(mask[g].any()) and not bool(mask[g].all()))
    leak[k][g, 0, 0, int(mask[g].nonzero()[0])] = 1e-6
    with pytest.raises(AssertionError, match="masked key"):
        gpu.check_map_structure(leak, batch, cfg)
    tilt = {n: t.clone() for n, t in ref.items()}
    tilt[k][ui.planted_genes(B)[1], 0, 0, 0] += 1e-7
    with pytest.raises(AssertionError, match="not uniform"):
        gpu.check_map_structure(tilt, batch, cfg)
    g32, g64 = (gpu.oracle_input_grads(P, batch, None, 1, dt) for dt in (torch.float32, torch.float64))
    wet = {n: t.clone() for n, t in g32.items()}
    wet["pcre_feats.500"][ui.dead_bins(batch)[1][500]] = 1e-12
    with pytest.raises(AssertionError):
        gpu.check_input_grad_structure(wet, g32, g64, batch, ui.dead_bins(batch))
