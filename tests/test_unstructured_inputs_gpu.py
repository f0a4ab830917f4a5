"""The HIP path on unstructured inputs (tests/unstructured_inputs.py): dense signed interaction frequencies, unsymmetric interaction
masks that differ per resolution, fully masked Regulation rows that other rows attend to, pad masks with holes / one valid bin /
a masked centre bin / nothing valid, features non-zero under the masks -- through the public Python surface (and so the C ABI).

  (a) forward, loss and all parameter gradients against the fp64 referee (tests/helpers.py), B = 6 per configuration, the regressor
      and B = 64 on the default one; the logits also against the reference's own (tests/golden/unstructured.npz);
  (b) 5-d masks, compact centre rows, other non-centre rows, the centre row repeated: bit-equal results;
  (c) the mask alone decides: large values where the reference cannot look change no bit;
  (d) input gradients against the oracle's autograd: exact zeros in dead bins and at entries masked at every resolution, non-zero
      oracle-matching gradients in fully padded slots whose token is visible; interaction_freq.grad against the reference's;
  (e) attention maps against tests/attn_oracle.py: masked keys exactly 0, fully masked rows exactly uniform;
  (f) pCRE deletion against tests/ablation_oracle.py on per-resolution base masks;
  (g) integrated gradients against tests/ig_oracle.py, the frequency-only path bit-equal to the general one on a dense baseline;
  (h) Trainer.step(trainer.stage(batch)) against model.train_step(...): bit-identical parameters and loss.

Each configuration is a different set of kernels reading the masks (CONFIGS).  With embed.n_layers = 2 every row of the 5-d promoter
mask is read, by the oracle and by the library: that configuration is compared on the masks as drawn and is left out of (b), whose
edits are not invariances there, and of (h), where a Slot refuses such promoter masks by name (tests/test_embed_dense_gpu.py asserts
that refusal).  What the library refuses by name there -- promoter input gradients, the `embed` map -- is asserted to raise."""
import functools

import numpy as np
import pytest
import torch

from oracle import chromoformer_oracle as orc
from tests import unstructured_inputs as ui
from tests.ablation_oracle import oracle_ablation, variant_masks
from tests.attn_oracle import oracle_maps
from tests.helpers import GOLDEN, assert_within_referee, build_model, perturbed_params, referee_hip, referee_oracle
from tests.ig_oracle import oracle_ig
from tests.test_attention_maps_gpu import EMB_TOL, MAP_TOL
from tests.test_attention_maps_gpu import _compare as compare_maps
from tests.test_attention_maps_gpu import _flat as flat_maps
from tests.test_config_variants_gpu import VARIANTS
from tests.test_embed_dense_gpu import CFG2
from tests.test_input_grads_gpu import _check_referee as check_input_grads
from tests.test_input_grads_gpu import _hip as hip_input_grads
from tests.test_input_grads_gpu import _oracle as oracle_input_grads
from tests.test_pcre_ablation_gpu import TOL as ABLATION_TOL

pytestmark = pytest.mark.gpu
B = 6
ARGS = ("promoter_feats", "promoter_pad_masks", "pcre_feats", "pcre_pad_masks", "interaction_masks", "interaction_freq")
CONFIGS = {"default": None}
CONFIGS.update({k: VARIANTS[k] for k in ("i_max4", "i_max16_unfused", "four_heads", "reg_4_heads", "odd_lengths", "long_rows", "d_emb_64")})
CONFIGS["embed_2_layers"] = CFG2
NAMES = list(CONFIGS)
CENTRE_ROW_ONLY = [n for n in NAMES if n != "embed_2_layers"]


def all_rows(name):
    return orc._cfg(CONFIGS[name])["embed"]["n_layers"] > 1


def _args(batch):
    return [batch[k] for k in ARGS]


@functools.lru_cache(maxsize=None)
def case(name, regression=False, n=B):
    """-> (cfg, batch, P) of a configuration: the unstructured batch and perturbed parameters."""
    cfg = orc._cfg(CONFIGS[name])
    return cfg, ui.unstructured_batch(n, cfg, regression=regression), perturbed_params(regression, cfg)


@functools.lru_cache(maxsize=None)
def referee(name, regression=False, n=B):
    cfg, batch, P = case(name, regression, n)
    return referee_oracle(P, batch, regression, torch.float32, cfg), referee_oracle(P, batch, regression, torch.float64, cfg)


def _model(name, regression=False, max_batch=B):
    cfg, _, P = case(name, regression)
    model = build_model(cfg, regression, max_batch)
    model.load_state_dict(P)
    return model


def _step(model, batch):
    """Fused forward + loss + backward -> (logits, loss, the flat gradient buffer), copies on the CPU."""
    logits, loss = model.forward_backward(model.pack_batch(batch), batch["label"])
    torch.cuda.synchronize()
    return logits.cpu().clone(), loss.cpu().clone(), model._gflat.cpu().clone()


def _same_bits(a, b, what):
    for x, y, part in zip(a, b, ("logits", "loss", "gradients")):
        assert torch.equal(x, y), (what, part, (x - y).abs().max().item())


# ----------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name,regression,n", [(k, False, B) for k in NAMES] + [("default", True, B), ("default", False, 64)])
def test_a_forward_loss_and_gradients_against_the_fp64_referee(name, regression, n):
    cfg, batch, P = case(name, regression, n)
    o32, o64 = referee(name, regression, n)
    got = referee_hip(functools.partial(build_model, cfg, regression), batch, P)
    worst = assert_within_referee(got, o32, o64)
    print("%s%s B = %d: worst err(HIP) / err(fp32 oracle) against the fp64 referee: %.2f (%s); logits %.2e (fp32 oracle %.2e)" % (
        name, " regressor" if regression else "", n, worst[0], worst[1], (got[0].double() - o64[0]).abs().max().item(),
        (o32[0].double() - o64[0]).abs().max().item()))


@pytest.mark.parametrize("regression", [False, True], ids=["classifier", "regressor"])
def test_a_logits_and_loss_match_the_reference_golden(regression):
    z = np.load(GOLDEN + "/unstructured.npz")
    head = "reg" if regression else "clf"
    batch = ui.unstructured_batch(int(z["B"]), seed=int(z["seed"]), regression=regression)
    P = orc.init_params(None, 42, regression)
    logits, loss, _ = referee_hip(functools.partial(build_model, None, regression), batch, P)
    d = (logits - torch.from_numpy(z[head + ".logits"])).abs().max().item()
    print("%s: HIP logits against the reference's %.2e, loss %.2e" % (head, d, abs(loss - float(z[head + ".loss"]))))
    assert d < 1e-4 and abs(loss - float(z[head + ".loss"])) < 1e-4 * max(1.0, abs(float(z[head + ".loss"])))


# ----------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", CENTRE_ROW_ONLY)
def test_b_mask_layouts_give_the_same_bits(name):
    cfg, batch, _ = case(name)
    model = _model(name)
    ref = _step(model, batch)
    _same_bits(_step(model, ui.centre_rows(batch)), ref, "compact centre rows")
    _same_bits(_step(model, ui.unstructured_batch(B, cfg, rows_seed=1)), ref, "other non-centre rows")
    _same_bits(_step(model, ui.unstructured_batch(B, cfg, rows="repeat")), ref, "the centre row repeated")
    _same_bits(_step(model, batch), ref, "run to run")


# ----------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("name", NAMES)
def test_c_the_mask_alone_decides(name):
    """Features of 37.0 in dead bins, frequencies of 1e3 at entries masked at every resolution: a masked key of a row with a valid key
    has p = 0 exactly, and 0 x finite added to a sum is exact -- so not one bit of logits, loss or gradients may move."""
    cfg, batch, P = case(name)
    dirty = ui.with_garbage(batch, all_rows(name))
    pd, cd = ui.dead_bins(batch, all_rows(name))
    assert all(bool(m.any()) for m in pd.values()) and all(bool(m.any()) for m in cd.values()) and bool(ui.masked_everywhere(batch).any())
    o32, o64 = referee(name)
    assert_within_referee(referee_hip(functools.partial(build_model, cfg, False), dirty, P), o32, o64)
    model = _model(name)
    _same_bits(_step(model, dirty), _step(model, batch), "garbage where the reference cannot look")


# ----------------------------------------------------------------------------- (d)
def _visible_padded_slots(batch, g64):
    """Fully padded pCRE slots whose features the fp64 oracle's gradient reaches (through the uniform softmax row)."""
    S = batch["pcre_feats"][next(iter(batch["pcre_feats"]))].shape[1]
    return [(g, s) for g in range(len(batch["label"])) for s in range(S) if ui.pcre_pattern(g, s, S) == "none_valid"
            and all(float(g64["pcre_feats.%d" % b][g, s].norm()) > 0 for b in batch["pcre_feats"])]


def check_input_grad_structure(gh, g32, g64, batch, everywhere_dead):
    """Exact zeros in dead bins and at frequency entries masked at every resolution; in the visible fully padded slots non-zero
    gradients within the referee rule of tests/test_input_grads_gpu.py, slot by slot."""
    pd, cd = everywhere_dead
    for b in batch["pcre_feats"]:
        assert bool((gh["pcre_feats.%d" % b][cd[b]] == 0).all()), ("pcre_feats", b)
        if gh.get("promoter_feats.%d" % b) is not None:
            assert bool((gh["promoter_feats.%d" % b][pd[b]] == 0).all()), ("promoter_feats", b)
    assert bool((gh["interaction_freq"][ui.masked_everywhere(batch)] == 0).all())
    slots = _visible_padded_slots(batch, g64)
    assert slots, "the batch must hold a fully padded pCRE slot whose token is visible"
    for g, s in slots:
        for b in batch["pcre_feats"]:
            k = "pcre_feats.%d" % b
            ref = g64[k][g, s]
            n = ref.norm().item()
            err_h, err_32 = (gh[k][g, s].double() - ref).norm().item(), (g32[k][g, s].double() - ref).norm().item()
            assert float(gh[k][g, s].abs().max()) > 0 and err_h <= max(2 * err_32, 2e-5 * n) + 1e-12, (k, g, s, err_h / n, err_32 / n)


@pytest.mark.parametrize("name", NAMES)
def test_d_input_gradients_against_the_oracle(name):
    cfg, batch, P = case(name)
    model = _model(name)
    want = ("promoter_feats", "pcre_feats", "interaction_freq")
    if all_rows(name):
        with pytest.raises(RuntimeError, match="promoter_feats.*embed.n_layers"):
            hip_input_grads(model, batch, 1, want=want)
        want = want[1:]
    _, gh, _ = hip_input_grads(model, batch, 1, want=want)
    g32, g64 = (oracle_input_grads(P, batch, cfg, 1, dt) for dt in (torch.float32, torch.float64))
    keys = [k for k, v in gh.items() if v is not None]
    assert len(keys) == (4 if all_rows(name) else 7)
    check_input_grads(gh, {k: g32[k] for k in keys}, {k: g64[k] for k in keys})
    check_input_grad_structure(gh, g32, g64, batch, ui.dead_bins(batch, all_rows(name)))


def test_d_interaction_freq_gradient_matches_the_reference_golden():
    z = np.load(GOLDEN + "/unstructured.npz")
    for regression, head, col in ((False, "clf", 1), (True, "reg", 0)):
        batch = ui.unstructured_batch(int(z["B"]), seed=int(z["seed"]), regression=regression)
        model = build_model(None, regression, int(z["B"]))
        model.load_state_dict(orc.init_params(None, 42, regression))
        _, gh, _ = hip_input_grads(model, batch, col, want=("interaction_freq",))
        ref = torch.from_numpy(z[head + ".freq_grad"])
        assert (gh["interaction_freq"] - ref).norm().item() <= 1e-4 * ref.norm().item() + 1e-7, head


# ----------------------------------------------------------------------------- (e)
def check_map_structure(got, batch, cfg, skip=()):
    """Masked keys of a row with a valid key: exactly 0.  Fully masked rows (Regulation row 0 of the planted genes, fully padded
    pCRE slots and promoters): every entry the same bits, 1 / n within the maps' tolerance."""
    Bn, S = len(batch["label"]), cfg["i_max"]
    _, g_row0, g_all = ui.planted_genes(Bn)
    for b in cfg["binsizes"]:
        L = cfg["w_max"] // b
        rows = {"regulation": (batch["interaction_masks"][b][:, 0, 0][:, None, None, :], got["regulation.%d" % b]),                       # [B, 1, 1, T]
                "pairwise_interaction": (batch["pcre_pad_masks"][b][:, :, 0, L // 2][:, None, :, None, :], got["pairwise_interaction.%d" % b])}
        if "embed" not in skip:
            rows["embed"] = (batch["promoter_pad_masks"][b][:, 0, 0, L // 2][:, None, :], got["embed.%d" % b])
        for k, (mask, g) in rows.items():
            mask = mask.expand(g.shape)
            full = mask.all(-1, keepdim=True).expand(g.shape)
            assert bool((mask & ~full).any()) and bool(full.any()), (k, b)
            assert bool((g[mask & ~full] == 0).all()), (k, b, "a masked key has weight")
            n = g.shape[-1]
            uniform = g[full].view(-1, n)
            assert bool((uniform == uniform[:, :1]).all()) and (uniform - 1.0 / n).abs().max().item() < MAP_TOL, (k, b, "fully masked row not uniform")
            assert (g.sum(-1) - 1).abs().max().item() < 1e-5, (k, b)
        assert bool(batch["interaction_masks"][b][[g_row0, g_all], 0, 0].all())


@pytest.mark.parametrize("name", NAMES)
def test_e_attention_maps_against_the_oracle(name):
    cfg, batch, P = case(name)
    model = _model(name)
    which = model.MAP_KEYS
    skip = ()
    if all_rows(name):
        with pytest.raises(RuntimeError, match=r"embed: .*embed\.n_layers = 1"):
            model.attention_maps(*_args(batch), which=("embed",))
        which, skip = which[1:], ("embed",)
    logits, maps = model.attention_maps(*_args(batch), which=which)
    ref_logits, ref = oracle_maps(P, batch, cfg)
    got = flat_maps(maps, cfg["binsizes"])
    compare_maps(got, ref, skip=skip)
    assert (logits.cpu() - ref_logits).abs().max().item() < EMB_TOL
    for k, r in ref.items():
        if k != "regulatory_embedding" and k.split(".")[0] not in skip:
            assert bool((got[k][r == 0] == 0).all()), k
    check_map_structure(got, batch, cfg, skip)
    with torch.enable_grad():
        assert torch.equal(model(*_args(batch)).detach().cpu(), logits.cpu())      # the maps' forward is the forward


# ----------------------------------------------------------------------------- (f)
@pytest.mark.parametrize("name", NAMES)
def test_f_pcre_deletion_on_per_resolution_masks(name):
    cfg, batch, P = case(name)
    S = cfg["i_max"]
    model = _model(name, max_batch=16)      # (several chunks)
    got = model.pcre_ablation(*_args(batch)).cpu()
    ref = oracle_ablation(P, batch, cfg)
    assert got.shape == ref.shape and (got - ref).abs().max().item() < ABLATION_TOL, (got - ref).abs().max().item()
    with torch.no_grad():
        for v in (0, 1, ui.ROW, S + 1):      # v = 0: cf_forward(save = 0) on the batch as given
            assert torch.equal(got[:, v], model(*_args(variant_masks(batch, v, S))).cpu()), v
    g_all = ui.planted_genes(B)[2]
    assert torch.equal(got[g_all, 1:], got[g_all, :1].expand(S + 1, -1))      # everything masked already: every deletion is the baseline
    # slot j of gene 0 masked (row and column) at every resolution: deleting it changes nothing; of gene 1 at one resolution only: it does
    j = 1
    edited = ui.copy_batch(batch)
    for r, m in enumerate(edited["interaction_masks"].values()):
        for g in ((0, 1) if r == 0 else (0,)):
            m[g, 0, j + 1, :] = True
            m[g, 0, :, j + 1] = True
    got = model.pcre_ablation(*_args(edited)).cpu()
    assert torch.equal(got[0, 1 + j], got[0, 0])
    assert not torch.equal(got[1, 1 + j], got[1, 0])
    assert (got - oracle_ablation(P, edited, cfg)).abs().max().item() < ABLATION_TOL


# ----------------------------------------------------------------------------- (g)
def _flat_attr(attr):
    out = {}
    for k, v in attr.items():
        if isinstance(v, dict):
            out.update({"%s.%d" % (k, b): t.detach().cpu() for b, t in v.items()})
        else:
            out[k] = v.detach().cpu()
    return out


def check_ig(attr, info, o32, o64, t):
    """The criteria of tests/test_integrated_gradients_gpu.py::test_matches_the_oracle_default_config."""
    (a32, _, _, _), (a64, lx64, lb64, d64) = o32, o64
    check_input_grads(_flat_attr(attr), _flat_attr(a32), _flat_attr(a64))
    assert (info["logits"].cpu().double() - lx64).abs().max().item() < 1e-4
    assert (info["baseline_logits"].cpu().double() - lb64).abs().max().item() < 1e-4
    gap = (lx64[:, t] - lb64[:, t]).abs()
    err = (info["delta"].cpu().double() - d64).abs()
    assert bool((err <= 1e-5 * gap + 1e-6).all()), (err, gap)


@pytest.mark.parametrize("name", NAMES)
def test_g_integrated_gradients_against_the_oracle(name, monkeypatch):
    from chromoformer_amd.attribution import ig_quadrature
    cfg, batch, P = case(name)
    n, t = 4, 1
    a, w = ig_quadrature("gausslegendre", n)
    model = _model(name, max_batch=16)
    # interaction_freq alone (the trunk runs once), from a dense per-gene baseline
    base = {"interaction_freq": torch.from_numpy(np.random.default_rng(3).normal(0.0, 1.0, size=batch["interaction_freq"].shape).astype(np.float32))}
    inp = ("interaction_freq",)
    attr, info = model.integrated_gradients(*_args(batch), n_steps=n, inputs=inp, baselines=base)
    check_ig(attr, info, *(oracle_ig(P, batch, a, w, t, inputs=inp, baselines=base, cfg=cfg, dtype=dt) for dt in (torch.float32, torch.float64)), t)
    assert bool((attr["interaction_freq"].cpu()[ui.masked_everywhere(batch)] == 0).all())
    monkeypatch.setenv("CF_IG_TRUNK_ONCE", "0")      # (read at cf_create)
    general = _model(name, max_batch=16)
    monkeypatch.delenv("CF_IG_TRUNK_ONCE")
    gen, gi = general.integrated_gradients(*_args(batch), n_steps=n, inputs=inp, baselines=base)
    assert torch.equal(attr["interaction_freq"], gen["interaction_freq"]) and all(torch.equal(info[k], gi[k]) for k in info)
    # pcre_feats alone
    inp = ("pcre_feats",)
    attr, info = model.integrated_gradients(*_args(batch), n_steps=n, inputs=inp)
    check_ig(attr, info, *(oracle_ig(P, batch, a, w, t, inputs=inp, cfg=cfg, dtype=dt) for dt in (torch.float32, torch.float64)), t)
    cd = ui.dead_bins(batch, all_rows(name))[1]
    for b in cfg["binsizes"]:
        assert bool((attr["pcre_feats"][b].cpu()[cd[b]] == 0).all()), b


# ----------------------------------------------------------------------------- (h)
@pytest.mark.parametrize("name", CENTRE_ROW_ONLY)
def test_h_the_training_loop_equals_the_separate_launches(name):
    from chromoformer_amd.engine import Trainer
    cfg, batch, P = case(name)
    model = _model(name)
    logits, loss = model.train_step(model.pack_batch(batch), batch["label"], 3e-5)
    torch.cuda.synchronize()
    logits, loss = logits.cpu().clone(), loss.cpu().clone()
    model2 = _model(name)
    trainer = Trainer(model2, lr=3e-5)
    logits2, loss2 = trainer.step(trainer.stage(batch))      # (one staged mask per resolution)
    torch.cuda.synchronize()
    assert torch.equal(logits2.cpu(), logits) and torch.equal(loss2.cpu().view(-1), loss.view(-1))
    sd, sd2 = model.state_dict(), model2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd), [k for k in sd if not torch.equal(sd[k], sd2[k])][:5]
    moved = sum(float((sd[k].cpu() - P[k]).abs().max()) > 0 for k in P)
    assert moved == sum(not orc.never_trained(k) for k in P), moved      # (the step did train: every trainable tensor moved)
